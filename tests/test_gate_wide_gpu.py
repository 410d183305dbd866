"""The router for more than 256 experts on the GPU (mxmoe_moe_gate_wide through moe.gate / moe.MoEBlock) against
tests/_gate_ref.py and tests/_gate_modes_ref.py.

Exact data (tests/_gate_ref.exact_data): the logits equal the f64 GEMM bit for bit, so softmax routing's ids equal
the f64 reference's, ties at the top-k boundary included (they occur in a quarter of the rows and are what the merge
of the column slices' candidate lists has to get right). Sigmoid routing selects on f32 scores: they are held to the
f64 sigmoid, and ids and weights to the reference routing run in numpy f32 on the kernel's own scores. The
by-construction cases compare end to end against f64 on the rows whose margins exceed the scores' error bound
(tests/test_gate_wide.py holds those to <= 20 %). Every case with E > 256 fails without the entry point.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16
from tests import _gate_modes_ref as mref
from tests import _gate_ref as ref
from tests import _gate_wide_ref as wref
from tests.test_gate_modes_gpu import _assert_close, _assert_logits_exact, _bits, _check_sigmoid, _dev, _np, _run

DEV = "cuda"


@pytest.fixture()
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k,shared,renorm", [
    (40, 256, 384, 8, False, True),    # Kimi-K2's width: 24 column blocks, 3 slices of 8
    (100, 64, 512, 10, True, True),    # Qwen3-Next: 513 columns, 33 blocks, 4 slices of 9; the shortest K loops
    (33, 256, 257, 16, False, False),  # the smallest wide case (2 slices of 9, K split 4), the full-row sum, topk 16
    (17, 2048, 320, 6, True, False),   # 21 blocks, 3 slices of 7, the shared gate mid-slice, a long K loop
    (20, 128, 448, 7, False, False),   # 28 blocks, 4 slices of 7
    (20, 128, 432, 5, False, True),    # 27 blocks, 3 slices of 9
    (20, 128, 500, 9, True, False),    # 32 blocks, 4 slices of 8, E no multiple of 16
    # 32 rows per workgroup (from 256 such workgroups on; narrow H keeps them quick), the last workgroup ragged
    (8192 + 17, 32, 384, 8, False, False),  # 3 slices of 8; one K step: the second K part idle
    (8192 + 5, 64, 512, 10, True, True),    # 4 slices of 9; the last workgroup's second token block past T
    (8192 + 40, 96, 302, 16, False, False),  # 3 slices of 7; E % 4 != 0: the outputs' scalar stores
])
def test_softmax_exact_data(gpu, T, H, E, k, shared, renorm):
    hidden, w, sg = ref.exact_data(T, H, E, seed=0, shared=shared)
    ids, wts, sw, logits = _run(hidden, w, k, sg, renormalize=renorm)
    x = _assert_logits_exact(logits, hidden, w)
    rids = ref.select(x, k)
    srt = -np.sort(-x, axis=1)
    print(f"rows with a tie at the top-k boundary: {(srt[:, k - 1] == srt[:, k]).mean():.2f}")
    assert (ids == rids).all(), "topk_ids"
    _assert_close(wts, ref.weights(logits, rids, renorm), "weights", rtol=wref.WIDE_SOFTMAX_RTOL)
    if shared:
        _assert_close(sw, ref.sigmoid(hidden.astype(np.float64) @ sg.astype(np.float64)), "shared_w",
                      rtol=wref.WIDE_SOFTMAX_RTOL)
    else:
        assert sw is None


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k,shared", [(40, 256, 384, 8, False), (50, 128, 512, 10, False), (24, 64, 512, 10, True),
                                            (8192 + 33, 64, 448, 7, False)])  # the last: 32 rows per workgroup
@pytest.mark.parametrize("renorm", [True, False])
def test_sigmoid_exact_data(gpu, T, H, E, k, shared, renorm):
    hidden, w, sg = ref.exact_data(T, H, E, seed=8, shared=shared)
    bias = mref.bias_data(E, np.random.default_rng(9))
    got = _run(hidden, w, k, sg, bias, scoring="sigmoid", renormalize=renorm, routed_scaling_factor=2.827, return_scores=True)
    x = ref.logits_f64(hidden, w)
    assert (np.abs(got[4] - ref.sigmoid(x)) <= mref.SCORE_ABS_ERR).all(), "scores"
    _check_sigmoid(hidden, w, sg, bias, k, 1, 1, 1, renorm, 2.827, got)
    # and without a bias: selection on the scores themselves
    if renorm and not shared:
        got = _run(hidden, w, k, None, None, scoring="sigmoid", renormalize=True, return_scores=True)
        _check_sigmoid(hidden, w, None, None, k, 1, 1, 1, True, 1.0, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case", wref.WIDE_ONEHOT_CASES, ids=str)
def test_by_construction_against_f64(gpu, case):
    """One-hot hidden rows: the logits are w_gate's entries, so ids and weights are compared with the f64 reference
    from the inputs alone (the weights' bound: tests/test_gate_modes_gpu.py's, 3 * SOFTMAX_RTOL)."""
    T, E, k, n_group, topk_group, seed = case
    (hidden, w, bias), (rids, rwts, rs, x), ok = mref.onehot_rows(T, E, k, n_group, topk_group, seed=seed)
    assert (~ok).sum() <= mref.ONEHOT_MAX_DROPPED * T
    ids, wts, sw, logits, scores = _run(hidden, w, k, None, bias, scoring="sigmoid", renormalize=True,
                                        routed_scaling_factor=2.5, return_scores=True)
    assert (_bits(logits) == _bits(x.astype(np.float32) + 0.0)).all(), "logits bits"
    assert (np.abs(scores - rs) <= mref.SCORE_ABS_ERR).all(), "scores"
    _assert_close(scores, rs, "scores")
    assert (ids[ok] == rids[ok]).all(), "topk_ids"
    _assert_close(wts[ok], rwts[ok], "weights", rtol=3 * ref.SOFTMAX_RTOL)


@pytest.mark.gpu
def test_ties_across_slices(gpu):
    E, H, T = 512, 64, 16
    w = ref.exact_data(T, H, E, seed=1)[1]
    zero = np.zeros((T, H), dtype=np.float16)
    for k in (10, 16):
        first = np.arange(k, dtype=np.int32)[None, :]
        ids, wts, _, _ = _run(zero, w, k)
        assert (ids == first).all() and (wts == np.float32(1.0 / 512)).all()
        ids, wts, _, _ = _run(zero, w, k, renormalize=True)
        want = np.float32(1.0 / k)
        assert (ids == first).all() and (np.abs(wts - want) <= np.spacing(want)).all()
        ids, wts, _, _, scores = _run(zero, w, k, scoring="sigmoid", return_scores=True)
        assert (scores == np.float32(0.5)).all() and (ids == first).all() and (wts == np.float32(0.5)).all()
    # one-hot rows: equal maxima in different slices (E = 512: 4 slices of 8 blocks, edges at 128, 256, 384), the rest
    # lower and equal among themselves, so the order is the maxima ascending, then the lowest other indices
    hidden = np.eye(H, dtype=np.float16)[:T]
    for cols in ([5, 200, 300, 511], [127, 128, 255, 256], [383, 384, 0, 129], [143, 144, 287, 288]):
        wt = np.zeros((E, H), dtype=np.float16)
        wt[:, :T] = -1.0
        wt[cols, :T] = 2.0
        rest = [e for e in range(E) if e not in cols][:2]
        want = np.array(sorted(cols) + rest, dtype=np.int32)[None, :]
        for kw in (dict(), dict(renormalize=True), dict(scoring="sigmoid")):
            ids = _run(hidden, wt, 6, **kw)[0]
            assert (ids == want).all(), (cols, kw)
        assert (_run(hidden, wt, 3)[0] == want[:, :3]).all()  # an equal maximum left out: the highest index
    # E = 384 (3 slices of 8 blocks) and 513 columns (4 slices of 9: edges at 144, 288, 432)
    for E2, shared, cols in ((384, False, [127, 128, 255, 256]), (512, True, [143, 144, 287, 288, 431, 432])):
        wt = np.zeros((E2, H), dtype=np.float16)
        wt[cols, :T] = 1.0
        sg = np.ones(H, dtype=np.float16) if shared else None
        ids = _run(hidden, wt, len(cols) + 1, sg, renormalize=True)[0]
        assert (ids == np.array(cols + [0], dtype=np.int32)[None, :]).all(), (E2, cols)


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k", [(48, 7168, 384, 8), (48, 96, 512, 10), (20, 2080, 288, 6)])
def test_long_and_odd_k(gpu, T, H, E, k):
    hidden, w = ref.random_data(T, H, E, seed=5)
    ids, wts, _, logits = _run(hidden, w, k)
    x = ref.logits_f64(hidden, w)
    bar = 1e-3 * np.abs(x) + 1e-3 * np.sqrt(np.mean(x ** 2))  # tests/test_gate_gpu.py's bound for random data
    print(f"logits: worst |err| / bar {float((np.abs(logits - x) / bar).max()):.3f}")
    assert (np.abs(logits - x) <= bar).all()
    rids, rwts, _, _ = ref.gate(hidden, w, k, logits=logits)  # selection / softmax of the kernel's own logits
    assert (ids == rids).all()
    _assert_close(wts, rwts, "weights", rtol=wref.WIDE_SOFTMAX_RTOL)
    # the sum is the same from run to run
    again = _run(hidden, w, k)
    assert all((_bits(a) == _bits(b)).all() for a, b in zip((ids, wts, logits), (again[0], again[1], again[3])))


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 15, 17, 33, 8192 + 17])  # (the last: 32 rows per workgroup)
def test_ragged_token_counts_leave_the_padding_alone(gpu, T):
    H, E, k, pad = 256, 384, 8, 64
    hidden, w, sg = ref.exact_data(T, H, E, seed=2, shared=True)
    bias = mref.bias_data(E, np.random.default_rng(3))
    nan_bits = int(np.int32(0x7FC12345))
    ids = torch.full((T + pad, k), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    wts, sw, logits, scores = (torch.full(shape, nan_bits, dtype=torch.int32, device=DEV)
                               for shape in ((T + pad, k), (T + pad,), (T + pad, E), (T + pad, E)))
    out = (ids[:T],) + tuple(t[:T].view(torch.float32) for t in (wts, sw, logits, scores))
    moe.gate(_dev(hidden), _dev(w), k, w_shared_gate=_dev(sg), return_logits=True, out=out, scoring="sigmoid",
             e_bias=_dev(bias), renormalize=True, routed_scaling_factor=2.827, return_scores=True)
    torch.cuda.synchronize()
    got = (_np(ids[:T]),) + tuple(_np(t[:T].view(torch.float32)) for t in (wts, sw, logits, scores))
    _check_sigmoid(hidden, w, sg, bias, k, 1, 1, 1, True, 2.827, got)
    assert (ids[T:] == 0x7FFFFFFF).all()
    for t in (wts, sw, logits, scores):
        assert (t[T:] == nan_bits).all()
    # softmax over the whole row (the per-slice sums) on the same buffers
    out = (ids[:T],) + tuple(t[:T].view(torch.float32) for t in (wts, sw, logits))
    moe.gate(_dev(hidden), _dev(w), k, w_shared_gate=_dev(sg), return_logits=True, out=out)
    torch.cuda.synchronize()
    x = _assert_logits_exact(_np(logits[:T].view(torch.float32)), hidden, w)
    assert (_np(ids[:T]) == ref.select(x, k)).all()
    _assert_close(_np(wts[:T].view(torch.float32)), ref.weights(x, ref.select(x, k), False), "weights",
                  rtol=wref.WIDE_SOFTMAX_RTOL)
    assert (ids[T:] == 0x7FFFFFFF).all()
    for t in (wts, sw, logits):
        assert (t[T:] == nan_bits).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["sigmoid", "softmax"])
def test_non_finite_rows(gpu, scoring):
    T, H, E, k = 48, 256, 320, 6
    hidden, w, _ = ref.exact_data(T, H, E, seed=6)
    hidden[5] = np.inf
    hidden[17, 100] = np.nan
    hidden[30] = 65504
    w[7] = 65504  # row 30: an f32 logit of 256 * 65504^2; every other row: logit 7 = 65504 * an integer, exact
    special = [5, 17, 30]
    others = np.setdiff1d(np.arange(T), special)
    with np.errstate(all="ignore"):
        if scoring == "sigmoid":
            bias = mref.bias_data(E, np.random.default_rng(7))
            got = _run(hidden, w, k, None, bias, scoring="sigmoid", renormalize=True, return_scores=True)
            _check_sigmoid(hidden, w, None, bias, k, 1, 1, 1, True, 1.0, got, rows=others)
        else:
            got = _run(hidden, w, k, renormalize=True)
            _assert_logits_exact(got[3], hidden, w, others)
            rids, rwts, _, _ = ref.gate(hidden, w, k, renormalize=True)
            assert (got[0][others] == rids[others]).all()
            _assert_close(got[1][others], rwts[others], "weights", rtol=wref.WIDE_SOFTMAX_RTOL)
    ids = got[0]
    for t in special:
        assert len(set(ids[t].tolist())) == k and ids[t].min() >= 0 and ids[t].max() < E
    r = moe.route(torch.from_numpy(ids).to(DEV), E)
    assert sum(r.counts) == T * k


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["softmax", "sigmoid"])
def test_logit_bias(gpu, scoring):
    """The returned logits, the selection and the weights all see x + logit_bias; the shared column does not."""
    T, H, E, k = 40, 128, 384, 8
    hidden, w, sg = ref.exact_data(T, H, E, seed=12, shared=True)
    lb = (np.random.default_rng(13).integers(-64, 65, size=E) / 16.0).astype(np.float32)  # exact sums with the logits
    kw = dict(scoring="sigmoid", return_scores=True) if scoring == "sigmoid" else {}
    out = moe.gate(_dev(hidden), _dev(w), k, renormalize=True, w_shared_gate=_dev(sg), return_logits=True,
                   logit_bias=_dev(lb), **kw)
    base = moe.gate(_dev(hidden), _dev(w), k, renormalize=True, w_shared_gate=_dev(sg), return_logits=True, **kw)
    torch.cuda.synchronize()
    got, base = tuple(_np(t) for t in out), tuple(_np(t) for t in base)
    x = ref.logits_f64(hidden, w) + lb.astype(np.float64)[None, :]
    assert (_bits(got[3]) == _bits(x.astype(np.float32) + 0.0)).all(), "logits bits"
    assert (_bits(got[2]) == _bits(base[2])).all(), "the shared gate sees no bias"
    assert (np.sort(got[0], axis=1) != np.sort(base[0], axis=1)).any(), "the bias must change some row's routing"
    if scoring == "softmax":
        rids = ref.select(x, k)
        assert (got[0] == rids).all()
        _assert_close(got[1], ref.weights(x, rids, True), "weights", rtol=wref.WIDE_SOFTMAX_RTOL)
    else:
        _assert_close(got[4], ref.sigmoid(x), "scores")
        rids = mref.select(got[4], k)
        assert (got[0] == rids).all()
        _assert_close(got[1], mref.sigmoid_weights(got[4], rids, True, 1.0), "weights")


def _abi(fn, h, w, sg, k, renorm, scoring, e_bias, n_group, topk_group, group_top, scale, lb):
    """One direct call of a 21-argument router entry point on fresh, poisoned buffers -> the five outputs."""
    T, H = h.shape
    E = w.shape[0]
    ids = torch.full((T, k), -1, dtype=torch.int32, device=DEV)
    wts, logits, scores = (torch.full(s, float("nan"), device=DEV) for s in ((T, k), (T, E), (T, E)))
    sw = torch.full((T,), float("nan"), device=DEV) if sg is not None else None
    p = lambda t: None if t is None else t.data_ptr()
    nat.check(nat.symbol(fn)(p(h), p(w), p(sg), T, H, E, k, renorm, scoring, p(e_bias), n_group, topk_group, group_top,
                             scale, p(lb), p(ids), p(wts), p(sw), p(logits), p(scores) if scoring else None,
                             torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return ids, wts, sw, logits, scores


@pytest.mark.gpu
@pytest.mark.parametrize("E,k,scoring,n_group,topk_group,group_top,shared,with_lb", [
    (64, 6, 0, 1, 1, 1, True, False), (64, 6, 1, 8, 3, 2, False, True),
    (256, 8, 1, 8, 4, 2, False, False), (256, 8, 0, 1, 1, 1, True, True),
])
def test_forwards_to_gate_ex2_up_to_256_experts(gpu, E, k, scoring, n_group, topk_group, group_top, shared, with_lb):
    T, H = 70, 256
    hidden, w, sg = ref.random_data(T, H, E, seed=20) + (None,)
    if shared:
        sg = (np.random.default_rng(21).standard_normal(H) * H ** -0.5).astype(np.float16)
    e_bias = _dev(mref.bias_data(E, np.random.default_rng(22))) if scoring else None
    lb = _dev(mref.bias_data(E, np.random.default_rng(23))) if with_lb else None
    args = (_dev(hidden), _dev(w), _dev(sg), k, 1, scoring, e_bias, n_group, topk_group, group_top, 2.5, lb)
    wide, ex2 = _abi("mxmoe_moe_gate_wide", *args), _abi("mxmoe_moe_gate_ex2", *args)
    for a, b in zip(wide, ex2):
        assert (a is None and b is None) or torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert (wide[0] >= 0).all() and not torch.isnan(wide[3]).any()


@pytest.mark.gpu
def test_stream_and_preallocated_outputs(gpu):
    T, H, E, k = 70, 256, 384, 8
    hidden, w, _ = ref.exact_data(T, H, E, seed=7)
    h, wd = _dev(hidden), _dev(w)
    kw = dict(return_logits=True, scoring="sigmoid", renormalize=True, routed_scaling_factor=2.827, return_scores=True,
              e_bias=_dev(mref.bias_data(E, np.random.default_rng(8))))
    first = moe.gate(h, wd, k, **kw)
    torch.cuda.synchronize()
    assert len(first) == 5 and first[2] is None
    want = [None if t is None else t.clone() for t in first]
    st = torch.cuda.Stream()
    out = tuple(None if t is None else torch.zeros_like(t) for t in first)
    torch.cuda.synchronize()
    for _ in range(2):
        got = moe.gate(h, wd, k, stream=st, out=out, **kw)
        st.synchronize()
        assert all(g is o for g, o in zip(got, out))
        for g, wnt in zip(got, want):
            assert g is None or torch.equal(g.view(torch.int32), wnt.view(torch.int32))
    with pytest.raises(ValueError):
        moe.gate(h, wd, k, out=out[:4], **kw)


def _captured(gf, static_hidden):
    """GraphForward.launch captured once on a side stream, as one linear chain (tests/test_dynamic_plan_gpu.py)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gf.launch(static_hidden)  # warm-up outside the capture (module loading)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gf.launch(static_hidden)
    torch.cuda.current_stream().wait_stream(side)
    return graph


@pytest.mark.gpu
def test_moe_block_layer_and_graph(gpu):
    """A layer of 272 experts from hidden states: MoEBlock equals moe.gate followed by MoEFFN.forward bit for bit, and
    the same layer captured once (GraphForward: launches only) equals the eager call bit for bit."""
    T, topk, E, H, N = 70, 4, 272, 256, 128
    g = torch.Generator().manual_seed(22)
    gate_up = [((torch.rand(2 * N, H, generator=g) * 2 - 1) * 0.2).half().to(DEV) for _ in range(E)]
    down = [((torch.rand(H, N, generator=g) * 2 - 1) * 0.2).half().to(DEV) for _ in range(E)]
    ffn = moe.MoEFFN(gate_up, down, [(FP16, FP16)] * E, num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    e_bias = ((torch.randint(-64, 65, (E,), generator=g)).float() / 256).to(DEV)
    hiddens = [((torch.rand(T, H, generator=g) * 2 - 1) * 3).half().to(DEV) for _ in range(2)]
    routing = dict(renormalize=True, scoring="sigmoid", e_bias=e_bias, routed_scaling_factor=2.827)
    block = moe.MoEBlock(ffn, w_gate, topk, **routing)
    out, mid = block.forward(hiddens[0], return_intermediates=True)
    ids, wts, sw = moe.gate(hiddens[0], w_gate, topk, **routing)
    want = ffn.forward(hiddens[0], ids, wts, sw)
    torch.cuda.synchronize()
    assert sw is None and int(ids.max()) >= 256  # experts beyond the older entry points' limit are in use
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.isfinite(out.float()).all()
    assert torch.equal(mid["topk_ids"], ids) and torch.equal(mid["topk_weights"], wts)
    gf = moe.GraphForward(block, T)
    static_hidden = hiddens[0].clone()
    graph = _captured(gf, static_hidden)
    for h in hiddens:
        eager = block.forward(h)
        static_hidden.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(gf.out.view(torch.int16), eager.view(torch.int16)), "graph replay != eager"
        assert gf.status() == 0
