"""The router's other routing rules on the GPU (mxmoe_moe_gate_ex through moe.gate / moe.MoEBlock: sigmoid
scores, selection bias, group-limited top-k, scaling factor) against tests/_gate_modes_ref.py.

Exact data (tests/_gate_ref.exact_data): the logits equal the f64 GEMM bit for bit. Softmax routing
selects on those, so its ids equal the f64 reference's, ties included. Sigmoid routing selects on f32
scores: they are held to the f64 sigmoid within _gate_ref.SOFTMAX_RTOL (the shared gate's arithmetic
and derivation), and the ids to the reference routing run in numpy f32 on the kernel's own scores
(one f32 add for v, one for a top-2 group sum: exactly reproducible), no row left out. The
by-construction cases compare end to end against f64, independent of the kernel's scores, on the rows
whose f64 margins exceed the scores' error bound (tests/test_gate_modes.py holds those to <= 20 %).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W8A8
from tests import _gate_modes_ref as mref
from tests import _gate_ref as ref

DEV = "cuda"


@pytest.fixture()
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _run(hidden, w, k, sg=None, bias=None, **kw):
    """(ids, weights, shared_w, logits[, scores]) as numpy."""
    out = moe.gate(_dev(hidden), _dev(w), k, w_shared_gate=_dev(sg), e_bias=_dev(bias), return_logits=True, **kw)
    torch.cuda.synchronize()
    return tuple(_np(t) for t in out)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_close(got, want, what, rtol=ref.SOFTMAX_RTOL):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    big = want > 1e-30
    worst = float((err[big] / want[big]).max()) if big.any() else 0.0
    print(f"{what}: worst relative error {worst:.3e}")
    assert (err <= rtol * want + ref.SOFTMAX_ATOL).all(), f"{what}: worst relative error {worst:.3e} > {rtol}"


def _assert_logits_exact(logits, hidden, w, rows=slice(None)):
    x = ref.logits_f64(hidden, w)
    assert (x.astype(np.float32).astype(np.float64)[rows] == x[rows]).all()  # the data is exact in f32
    assert (_bits(logits)[rows] == _bits(x.astype(np.float32) + 0.0)[rows]).all(), "logits bits"
    return x


def _check_sigmoid(hidden, w, sg, bias, k, n_group, topk_group, group_top, renorm, scale, got, rows=slice(None)):
    """Kernel outputs of a sigmoid call on exact data: logits against the f64 GEMM, scores against the
    f64 sigmoid, ids against the f32 reference routing of the kernel's own scores, weights against the
    f64 formula on those scores."""
    ids, wts, sw, logits, scores = got
    x = _assert_logits_exact(logits, hidden, w, rows)
    _assert_close(scores[rows], ref.sigmoid(x)[rows], "scores")
    assert scores.dtype == np.float32
    v = mref.selection_values(scores, bias)
    assert v.dtype == np.float32
    rids = mref.select(v, k, n_group, topk_group, group_top)
    assert (ids[rows] == rids[rows]).all(), "topk_ids"
    _assert_close(wts[rows], mref.sigmoid_weights(scores, rids, renorm, scale)[rows], "weights")
    if sg is not None:
        _assert_close(sw[rows], ref.sigmoid(hidden.astype(np.float64) @ sg.astype(np.float64))[rows], "shared_w")
    else:
        assert sw is None


@pytest.mark.gpu
@pytest.mark.parametrize("renorm", [False, True])
def test_defaults_are_todays_call(gpu, renorm):
    T, H, E, k = 96, 2048, 60, 4
    hidden, w, sg = ref.exact_data(T, H, E, seed=0, shared=True)
    h, wd, sgd = _dev(hidden), _dev(w), _dev(sg)
    base = moe.gate(h, wd, k, renormalize=renorm, w_shared_gate=sgd, return_logits=True)
    same = moe.gate(h, wd, k, renormalize=renorm, w_shared_gate=sgd, return_logits=True, scoring="softmax", e_bias=None,
                    n_group=1, topk_group=1, group_top=None, routed_scaling_factor=1.0, return_scores=False)
    x16 = moe.gate(h, wd, k, renormalize=renorm, w_shared_gate=sgd, return_logits=True, routed_scaling_factor=16.0)
    torch.cuda.synchronize()
    assert len(base) == len(same) == len(x16) == 4
    for a, b in zip(base, same):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # a power of two: today's weights times 16 exactly, everything else bit for bit
    assert torch.equal(x16[1].view(torch.int32), (base[1] * 16.0).view(torch.int32))
    for i in (0, 2, 3):
        assert torch.equal(x16[i].view(torch.int32), base[i].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k,n_group,topk_group", [
    (48, 256, 160, 6, 8, 3),  # DeepSeek-V2's groups of 20, which straddle the 16-column blocks
    (33, 128, 8, 2, 2, 1),    # groups of 4: one lane's registers
])
@pytest.mark.parametrize("renorm", [False, True])
def test_softmax_group_limited_exact_data(gpu, T, H, E, k, n_group, topk_group, renorm):
    hidden, w, _ = ref.exact_data(T, H, E, seed=3)
    ids, wts, sw, logits = _run(hidden, w, k, renormalize=renorm, n_group=n_group, topk_group=topk_group,
                                routed_scaling_factor=16.0)
    x = _assert_logits_exact(logits, hidden, w)
    rids, rwts, _, _ = mref.gate(hidden, w, k, n_group=n_group, topk_group=topk_group, renormalize=renorm, routed_scale=16.0)
    assert (ids == rids).all(), "topk_ids"
    assert (np.sort(rids, axis=1) != np.sort(ref.select(x, k), axis=1)).any(), "the groups must change some row"
    _assert_close(wts, rwts, "weights")
    assert sw is None


SIGMOID_SHAPES = [
    # T, H, E, k, n_group, topk_group, shared gate
    (64, 256, 256, 8, 8, 4, False),      # DeepSeek-V3's routing: 16 column blocks
    (100, 64, 256, 8, 8, 4, True),       # 17 column blocks
    (300, 160, 160, 6, 8, 3, False),     # groups of 20, 12 column blocks
    (8192 + 17, 32, 128, 8, 4, 2, False),  # 32 rows per workgroup, 8 column blocks
    (8192 + 5, 64, 64, 6, 8, 3, True),   # 32 rows per workgroup, 5 column blocks
    (16384 + 33, 96, 64, 6, 4, 2, False),  # 64 rows per workgroup
    (40, 128, 64, 6, 1, 1, True),        # ungrouped (GLM-4.5-style), 5 column blocks
]


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k,n_group,topk_group,shared", SIGMOID_SHAPES)
@pytest.mark.parametrize("renorm", [False, True])
def test_sigmoid_exact_data(gpu, T, H, E, k, n_group, topk_group, shared, renorm):
    hidden, w, sg = ref.exact_data(T, H, E, seed=8, shared=shared)
    bias = mref.bias_data(E, np.random.default_rng(9))
    kw = dict(scoring="sigmoid", n_group=n_group, topk_group=topk_group, renormalize=renorm, routed_scaling_factor=2.5,
              return_scores=True)
    group_top = 2 if n_group > 1 else 1  # moe.gate's default
    _check_sigmoid(hidden, w, sg, bias, k, n_group, topk_group, group_top, renorm, 2.5, _run(hidden, w, k, sg, bias, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("group_top", [1, 2])
@pytest.mark.parametrize("with_bias", [True, False])
def test_sigmoid_group_top_and_no_bias(gpu, group_top, with_bias):
    T, H, E, k, n_group, topk_group = SIGMOID_SHAPES[0][:6]
    hidden, w, _ = ref.exact_data(T, H, E, seed=10)
    bias = mref.bias_data(E, np.random.default_rng(11)) if with_bias else None
    got = _run(hidden, w, k, None, bias, scoring="sigmoid", n_group=n_group, topk_group=topk_group, group_top=group_top,
               renormalize=True, return_scores=True)
    _check_sigmoid(hidden, w, None, bias, k, n_group, topk_group, group_top, True, 1.0, got)


@pytest.mark.gpu
@pytest.mark.parametrize("case", mref.ONEHOT_CASES, ids=str)
def test_by_construction_against_f64(gpu, case):
    """One-hot hidden rows: the logits are w_gate's entries, so ids and weights are compared with the
    f64 reference from the inputs alone. Weights: each score is within SOFTMAX_RTOL of the f64 one,
    a weight is one score over a sum of positive scores (+ three roundings), so 3 * SOFTMAX_RTOL."""
    T, E, k, n_group, topk_group = case
    (hidden, w, bias), (rids, rwts, rs, x), ok = mref.onehot_rows(*case)
    assert ok.sum() >= (1 - mref.ONEHOT_MAX_DROPPED) * T
    ids, wts, sw, logits, scores = _run(hidden, w, k, None, bias, scoring="sigmoid", n_group=n_group, topk_group=topk_group,
                                        renormalize=True, routed_scaling_factor=2.5, return_scores=True)
    assert (_bits(logits) == _bits(x.astype(np.float32) + 0.0)).all(), "logits bits"
    _assert_close(scores, rs, "scores")
    assert (ids[ok] == rids[ok]).all(), "topk_ids"
    _assert_close(wts[ok], rwts[ok], "weights", rtol=3 * ref.SOFTMAX_RTOL)


@pytest.mark.gpu
def test_ties_between_groups_and_experts(gpu):
    T, H, E, k, n_group, topk_group = 40, 256, 32, 10, 4, 2
    hidden, w, _ = ref.exact_data(T, H, E, seed=1)
    w[16:] = w[:16]  # groups 2, 3 repeat groups 0, 1: every group score and every v occurs twice
    for group_top in (1, 2):
        got = _run(hidden, w, k, scoring="sigmoid", n_group=n_group, topk_group=topk_group, group_top=group_top,
                   return_scores=True)
        _check_sigmoid(hidden, w, None, None, k, n_group, topk_group, group_top, False, 1.0, got)
    sids, swts, _, logits = _run(hidden, w, 3, n_group=n_group, topk_group=topk_group)  # softmax, on the logits
    _assert_logits_exact(logits, hidden, w)
    assert (sids == mref.gate(hidden, w, 3, n_group=n_group, topk_group=topk_group)[0]).all()
    # zero hidden: every score is 0.5, so the first topk experts of the first topk_group groups
    zero = np.zeros_like(hidden)
    first = np.arange(k, dtype=np.int32)[None, :]
    for group_top in (1, 2):
        ids, wts, _, _, scores = _run(zero, w, k, scoring="sigmoid", n_group=n_group, topk_group=topk_group,
                                      group_top=group_top, routed_scaling_factor=2.5, return_scores=True)
        assert (scores == np.float32(0.5)).all()
        assert (ids == first).all()
        assert (wts == np.float32(1.25)).all()
        ids, wts, _, _ = _run(zero, w, k, scoring="sigmoid", n_group=n_group, topk_group=topk_group, group_top=group_top,
                              renormalize=True, routed_scaling_factor=2.5)
        assert (ids == first).all()
        want = np.float32(2.5 / k)
        assert (np.abs(wts - want) <= np.spacing(want)).all()
    ids, wts, _, _ = _run(zero, w, 3, n_group=n_group, topk_group=topk_group, routed_scaling_factor=2.0)
    assert (ids == first[:, :3]).all() and (wts == np.float32(2.0 / 32)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 17, 65])
def test_ragged_token_counts_leave_the_padding_alone(gpu, T):
    H, E, k, n_group, topk_group, pad = 256, 64, 6, 4, 2, 64
    hidden, w, sg = ref.exact_data(T, H, E, seed=2, shared=True)
    bias = mref.bias_data(E, np.random.default_rng(3))
    nan_bits = int(np.int32(0x7FC12345))
    ids = torch.full((T + pad, k), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    wts, sw, logits, scores = (torch.full(shape, nan_bits, dtype=torch.int32, device=DEV)
                               for shape in ((T + pad, k), (T + pad,), (T + pad, E), (T + pad, E)))
    out = (ids[:T],) + tuple(t[:T].view(torch.float32) for t in (wts, sw, logits, scores))
    moe.gate(_dev(hidden), _dev(w), k, w_shared_gate=_dev(sg), return_logits=True, out=out, scoring="sigmoid",
             e_bias=_dev(bias), n_group=n_group, topk_group=topk_group, renormalize=True, routed_scaling_factor=2.5,
             return_scores=True)
    torch.cuda.synchronize()
    got = (_np(ids[:T]),) + tuple(_np(t[:T].view(torch.float32)) for t in (wts, sw, logits, scores))
    _check_sigmoid(hidden, w, sg, bias, k, n_group, topk_group, 2, True, 2.5, got)
    assert (ids[T:] == 0x7FFFFFFF).all()
    for t in (wts, sw, logits, scores):
        assert (t[T:] == nan_bits).all()


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", ["sigmoid", "softmax"])
def test_non_finite_rows(gpu, scoring):
    T, H, E, k, n_group, topk_group = 48, 256, 64, 4, 4, 2
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
            got = _run(hidden, w, k, None, bias, scoring="sigmoid", n_group=n_group, topk_group=topk_group,
                       renormalize=True, return_scores=True)
            _check_sigmoid(hidden, w, None, bias, k, n_group, topk_group, 2, True, 1.0, got, rows=others)
        else:
            got = _run(hidden, w, k, n_group=n_group, topk_group=topk_group, renormalize=True)
            x = _assert_logits_exact(got[3], hidden, w, others)
            rids, rwts, _, _ = mref.gate(hidden, w, k, n_group=n_group, topk_group=topk_group, renormalize=True)
            assert (got[0][others] == rids[others]).all()
            _assert_close(got[1][others], rwts[others], "weights")
    ids = got[0]
    for t in special:
        assert len(set(ids[t].tolist())) == k and ids[t].min() >= 0 and ids[t].max() < E
    r = moe.route(torch.from_numpy(ids).to(DEV), E)
    assert sum(r.counts) == T * k


@pytest.mark.gpu
def test_stream_and_preallocated_outputs(gpu):
    T, H, E, k = 70, 256, 64, 6
    hidden, w, sg = ref.exact_data(T, H, E, seed=7, shared=True)
    h, wd, sgd = _dev(hidden), _dev(w), _dev(sg)
    kw = dict(w_shared_gate=sgd, return_logits=True, scoring="sigmoid", n_group=8, topk_group=3, renormalize=True,
              e_bias=_dev(mref.bias_data(E, np.random.default_rng(8))), routed_scaling_factor=2.5, return_scores=True)
    first = moe.gate(h, wd, k, **kw)
    torch.cuda.synchronize()
    assert len(first) == 5
    want = [t.clone() for t in first]
    st = torch.cuda.Stream()
    out = tuple(torch.zeros_like(t) for t in first)
    torch.cuda.synchronize()
    for _ in range(2):
        got = moe.gate(h, wd, k, stream=st, out=out, **kw)
        st.synchronize()
        assert all(g is o for g, o in zip(got, out))
        for g, wnt in zip(got, want):
            assert torch.equal(g.view(torch.int32), wnt.view(torch.int32))
    with pytest.raises(ValueError):
        moe.gate(h, wd, k, out=out[:4], **kw)  # four buffers for a call with five outputs
    with pytest.raises(ValueError):
        moe.gate(h, wd, k, out=out[:4] + (out[4].double(),), **kw)


@pytest.mark.gpu
def test_moe_block_layer(gpu):
    T, topk, E, H, N, Ns = 70, 4, 16, 256, 128, 256
    g = torch.Generator().manual_seed(22)
    gate_up = [((torch.rand(2 * N, H, generator=g) * 2 - 1) * 0.2).half().to(DEV) for _ in range(E)]
    gate_up.append(((torch.rand(2 * Ns, H, generator=g) * 2 - 1) * 0.2).half().to(DEV))
    down = [((torch.rand(H, N, generator=g) * 2 - 1) * 0.2).half().to(DEV) for _ in range(E)]
    down.append(((torch.rand(H, Ns, generator=g) * 2 - 1) * 0.2).half().to(DEV))
    qcfg = [(W8A8, W8A8), (W4A4, W8A8), (FP16, FP16), (W8A8, W4A4)] * 4 + [(FP16, FP16)]
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).half().to(DEV)
    e_bias = ((torch.randint(-64, 65, (E,), generator=g)).float() / 256).to(DEV)
    hidden = ((torch.rand(T, H, generator=g) * 2 - 1) * 3).half().to(DEV)
    routing = dict(renormalize=True, scoring="sigmoid", e_bias=e_bias, n_group=4, topk_group=2)
    block = moe.MoEBlock(ffn, w_gate, topk, w_shared_gate=w_sg, routed_scaling_factor=2.5, **routing)
    out, mid = block.forward(hidden, return_intermediates=True)
    ids, wts, sw = moe.gate(hidden, w_gate, topk, w_shared_gate=w_sg, routed_scaling_factor=2.5, **routing)
    want = ffn.forward(hidden, ids, wts, sw)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.isfinite(out.float()).all()
    assert torch.equal(mid["topk_ids"], ids) and torch.equal(mid["topk_weights"], wts) and torch.equal(mid["shared_w"], sw)
    plain_ids = moe.gate(hidden, w_gate, topk, w_shared_gate=w_sg)[0]
    assert not torch.equal(plain_ids, ids)  # the rule routes differently from the default one
    # a factor of 2 doubles the routed part's weights and nothing else
    ids1, wts1, sw1 = moe.gate(hidden, w_gate, topk, w_shared_gate=w_sg, **routing)
    twice = moe.MoEBlock(ffn, w_gate, topk, w_shared_gate=w_sg, routed_scaling_factor=2.0, **routing).forward(hidden)
    want2 = ffn.forward(hidden, ids1, wts1 * 2.0, sw1)
    torch.cuda.synchronize()
    assert torch.equal(twice.view(torch.int16), want2.view(torch.int16))
    once = moe.MoEBlock(ffn, w_gate, topk, w_shared_gate=w_sg, **routing).forward(hidden)
    torch.cuda.synchronize()
    assert not torch.equal(once.view(torch.int16), twice.view(torch.int16))
