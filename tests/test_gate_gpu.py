"""The router kernel (mxmoe_moe_gate, moe.gate, moe.MoEBlock) on the GPU against tests/_gate_ref.py.

Exact data (integers in [-2, 2] x integers in [-2, 2] * 2^-6): f32 accumulation is exact in any
order, so the kernel's logits must equal the f64 reference bit for bit and its ids exactly — ties,
which this data has in every row, included. Random data: the logits within the project's fp16 bar,
ids and weights against the reference selection / softmax of the kernel's own logits. Weights and
shared_w: |w - ref| <= 4e-5 * ref + 2^-126 (derivation: _gate_ref.SOFTMAX_RTOL).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W8A8
from tests import _gate_ref as ref

DEV = "cuda"


@pytest.fixture()
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _dev(a):
    return None if a is None else torch.from_numpy(a).to(DEV)


def _run(hidden, w, k, renorm=False, sg=None):
    ids, wts, sw, logits = moe.gate(_dev(hidden), _dev(w), k, renormalize=renorm, w_shared_gate=_dev(sg),
                                    return_logits=True)
    torch.cuda.synchronize()
    return ids.cpu().numpy(), wts.cpu().numpy(), None if sw is None else sw.cpu().numpy(), logits.cpu().numpy()


def _assert_softmax(got, want, what):
    ok, worst = ref.softmax_close(got, want)
    print(f"{what}: worst relative error {worst:.3e}")
    assert ok, f"{what}: worst relative error {worst:.3e} > {ref.SOFTMAX_RTOL}"


def _check_exact(hidden, w, k, renorm, sg, got, rows=None):
    """Kernel outputs on exact data against the f64 reference (rows: the subset to compare)."""
    ids, wts, sw, logits = got
    rids, rwts, rsw, x = ref.gate(hidden, w, k, renormalize=renorm, w_shared_gate=sg)
    sel = slice(None) if rows is None else rows
    assert (x.astype(np.float32).astype(np.float64)[sel] == x[sel]).all()  # the data is exact in f32
    assert (logits[sel].view(np.uint32) == (x.astype(np.float32) + 0.0)[sel].view(np.uint32)).all(), "logits bits"
    assert (ids[sel] == rids[sel]).all(), "topk_ids"
    _assert_softmax(wts[sel], rwts[sel], "weights")
    if sg is not None:
        _assert_softmax(sw[sel], rsw[sel], "shared_w")
    else:
        assert sw is None


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k,renorm,shared", [
    (96, 2048, 60, 4, False, True),    # qwen2_moe: E no multiple of 16, the shared gate in a padded column
    (80, 2048, 64, 6, False, False),   # DeepSeek-V2-Lite
    (33, 128, 8, 2, True, False),      # Mixtral-like: E < 16, ragged T, the shortest K loop
    (64, 256, 256, 8, False, False),   # the E limit
])
def test_exact_data_parity(gpu, T, H, E, k, renorm, shared):
    hidden, w, sg = ref.exact_data(T, H, E, seed=0, shared=shared)
    _check_exact(hidden, w, k, renorm, sg, _run(hidden, w, k, renorm, sg))


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k,shared", [
    (8192 + 5, 64, 60, 4, True),     # 256 workgroups of 32 rows (two token blocks per workgroup), ragged
    (16384 + 33, 96, 64, 6, False),  # 64 rows per workgroup (four token blocks), K split unevenly over the waves
    (8192 + 17, 32, 120, 3, False),  # 8 column blocks at 32 rows per workgroup; one K step: 7 waves idle
    (40, 128, 64, 6, True),          # 5 column blocks: 64 experts and the shared gate in a block of its own
    (300, 160, 180, 16, True),       # 12 column blocks, the topk limit
    (100, 64, 256, 5, True),         # 17 column blocks: the 4-wave form
])
def test_every_launch_shape(gpu, T, H, E, k, shared):
    """The kernel forms the launch chooses between (rows per workgroup by T, column blocks by E,
    4 or 8 waves), each at the smallest T that selects it; narrow H keeps them quick."""
    hidden, w, sg = ref.exact_data(T, H, E, seed=8, shared=shared)
    _check_exact(hidden, w, k, False, sg, _run(hidden, w, k, False, sg))


@pytest.mark.gpu
def test_ties_at_the_boundary_in_every_row(gpu):
    T, H, E, k = 40, 256, 32, 3
    hidden, w, _ = ref.exact_data(T, H, E, seed=1)
    w[16:] = w[:16]  # every logit occurs twice: an odd topk always splits a pair
    _check_exact(hidden, w, k, False, None, _run(hidden, w, k))
    zero = np.zeros_like(hidden)
    ids, wts, _, _ = _run(zero, w, k)
    assert (ids == np.arange(k, dtype=np.int32)[None, :]).all()
    assert (wts == np.float32(1.0 / 32)).all()
    ids, wts, _, _ = _run(zero, w, k, renorm=True)
    assert (ids == np.arange(k, dtype=np.int32)[None, :]).all()
    third = np.float32(1.0 / 3)
    assert (np.abs(wts - third) <= np.spacing(third)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 15, 17, 63, 65, 129])
def test_ragged_token_counts_leave_the_padding_alone(gpu, T):
    H, E, k, pad = 256, 60, 4, 64
    hidden, w, sg = ref.exact_data(T, H, E, seed=2, shared=True)
    nan_bits = np.int32(0x7FC12345)
    ids = torch.full((T + pad, k), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    wts = torch.full((T + pad, k), int(nan_bits), dtype=torch.int32, device=DEV)
    sw = torch.full((T + pad,), int(nan_bits), dtype=torch.int32, device=DEV)
    logits = torch.full((T + pad, E), int(nan_bits), dtype=torch.int32, device=DEV)
    out = (ids[:T], wts[:T].view(torch.float32), sw[:T].view(torch.float32), logits[:T].view(torch.float32))
    moe.gate(_dev(hidden), _dev(w), k, w_shared_gate=_dev(sg), return_logits=True, out=out)
    torch.cuda.synchronize()
    got = (ids[:T].cpu().numpy(), wts[:T].view(torch.float32).cpu().numpy(), sw[:T].view(torch.float32).cpu().numpy(),
           logits[:T].view(torch.float32).cpu().numpy())
    _check_exact(hidden, w, k, False, sg, got)
    assert (ids[T:] == 0x7FFFFFFF).all()
    for t in (wts, sw, logits):
        assert (t[T:] == int(nan_bits)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,H,E,k", [(256, 2048, 60, 4), (256, 512, 64, 6)])
def test_random_data(gpu, T, H, E, k):
    hidden, w = ref.random_data(T, H, E, seed=5)
    ids, wts, _, logits = _run(hidden, w, k)
    x = ref.logits_f64(hidden, w)
    bar = 1e-3 * np.abs(x) + 1e-3 * np.sqrt(np.mean(x ** 2))  # the project's fp16 bar (tests/_util.py)
    assert (np.abs(logits - x) <= bar).all()
    rids, rwts, _, _ = ref.gate(hidden, w, k, logits=logits)  # selection / softmax of the kernel's own logits
    assert (ids == rids).all()
    _assert_softmax(wts, rwts, "weights")


@pytest.mark.gpu
def test_non_finite_rows(gpu):
    T, H, E, k = 48, 256, 60, 4
    hidden, w, _ = ref.exact_data(T, H, E, seed=6)
    hidden[5] = np.inf
    hidden[17, 100] = np.nan
    hidden[30] = 65504
    w[7] = 65504  # row 30: an f32 logit of 256 * 65504^2, beyond exp's range
    special = [5, 17, 30]
    # (w[7] changes logit 7 of every row to 65504 * an integer of at most 512: still exact in f32)
    got = _run(hidden, w, k)
    ids = got[0]
    for t in special:
        assert len(set(ids[t].tolist())) == k and ids[t].min() >= 0 and ids[t].max() < E
    others = np.setdiff1d(np.arange(T), special)
    with np.errstate(all="ignore"):
        _check_exact(hidden, w, k, False, None, got, rows=others)
    r = moe.route(torch.from_numpy(ids).to(DEV), E)
    assert sum(r.counts) == T * k


@pytest.mark.gpu
def test_stream_and_preallocated_outputs(gpu):
    T, H, E, k = 70, 256, 60, 4
    hidden, w, sg = ref.exact_data(T, H, E, seed=7, shared=True)
    h, wd, sgd = _dev(hidden), _dev(w), _dev(sg)
    first = moe.gate(h, wd, k, w_shared_gate=sgd, return_logits=True)
    torch.cuda.synchronize()
    want = [t.clone() for t in first]
    st = torch.cuda.Stream()
    out = tuple(torch.zeros_like(t) for t in first)
    torch.cuda.synchronize()
    for _ in range(2):
        got = moe.gate(h, wd, k, w_shared_gate=sgd, return_logits=True, stream=st, out=out)
        st.synchronize()
        assert all(g is o for g, o in zip(got, out))
        for g, wnt in zip(got, want):
            assert torch.equal(g.view(torch.int32), wnt.view(torch.int32))
    with pytest.raises(ValueError):
        moe.gate(h, wd, k, w_shared_gate=sgd, out=out)  # four buffers for a call with three outputs


@pytest.mark.gpu
def test_moe_block_layer(gpu):
    T, topk, E, H, N, Ns = 70, 2, 8, 256, 128, 256
    g = torch.Generator().manual_seed(21)
    gate_up = [((torch.rand(2 * N, H, generator=g) * 2 - 1) * 0.2).half().to(DEV) for _ in range(E)]
    gate_up.append(((torch.rand(2 * Ns, H, generator=g) * 2 - 1) * 0.2).half().to(DEV))
    down = [((torch.rand(H, N, generator=g) * 2 - 1) * 0.2).half().to(DEV) for _ in range(E)]
    down.append(((torch.rand(H, Ns, generator=g) * 2 - 1) * 0.2).half().to(DEV))
    qcfg = [(W8A8, W8A8), (W4A4, W8A8), (FP16, FP16), (W8A8, W4A4), (W4A4, W4A4), (FP16, W8A8), (W8A8, W8A8),
            (W4A4, FP16), (FP16, FP16)]
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).half().to(DEV)
    hidden = ((torch.rand(T, H, generator=g) * 2 - 1) * 3).half().to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, w_shared_gate=w_sg)
    out, mid = block.forward(hidden, return_intermediates=True)
    ids, wts, sw = moe.gate(hidden, w_gate, topk, w_shared_gate=w_sg)
    want = ffn.forward(hidden, ids, wts, sw)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
    assert torch.equal(block.forward(hidden).view(torch.int16), want.view(torch.int16))
    assert torch.isfinite(out.float()).all()
    assert torch.equal(mid["topk_ids"], ids) and torch.equal(mid["topk_weights"], wts) and torch.equal(mid["shared_w"], sw)
    assert "routing" in mid
    with pytest.raises(ValueError):
        moe.MoEBlock(ffn, w_gate[:, : H // 2], topk)
    with pytest.raises(ValueError):
        moe.MoEBlock(ffn, w_gate[: E - 1], topk)
    no_shared = moe.MoEFFN(gate_up[:E], down[:E], qcfg[:E], num_routed=E)
    with pytest.raises(ValueError):
        moe.MoEBlock(no_shared, w_gate, topk, w_shared_gate=w_sg)
