"""bf16 layers on the GPU: the router on the bf16 MFMA (mxmoe_moe_gate_dt), the gather that reads bf16 rows
(mxmoe_moe_gather_quant), the combine that writes bf16 (mxmoe_moe_combine_dt) and whole layers with bf16 ends — eager,
planned, graph forward and a captured graph. Helpers and data: tests/_bf16_ref.py.

Every comparison is bit for bit, with one named tolerance: the weights against the f64 softmax / sigmoid take
_gate_ref.SOFTMAX_RTOL, and the random-data logits the project's fp16 bar (1e-3 |x| + 1e-3 rms, tests/test_gate_gpu.py):
the error source there is the f32 accumulation, the same for both operand formats.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W4A8_MXFP8, W4A16_MXFP4, W8A8
from tests import _bf16_ref as bref
from tests import _gate_modes_ref as mref
from tests import _gate_ref as ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F16 = torch.bfloat16, torch.float16


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _t(a, dtype):
    """f32 numpy array of bf16 values -> device tensor of dtype (exact for the data of this file)"""
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dtype).to(DEV)


def _np(t):
    return None if t is None else t.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gate(hidden, w, k, dtype, sg=None, e_bias=None, logit_bias=None, **kw):
    """(ids, weights, shared_w, logits[, scores]) as numpy, the operands as ``dtype``"""
    f32 = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    out = moe.gate(_t(hidden, dtype), _t(w, dtype), k, w_shared_gate=_t(sg, dtype), e_bias=f32(e_bias),
                   logit_bias=f32(logit_bias), return_logits=True, **kw)
    torch.cuda.synchronize()
    return tuple(_np(t) for t in out)


def _assert_close(got, want, what, rtol=ref.SOFTMAX_RTOL):
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - want)
    big = want > 1e-30
    worst = float((err[big] / want[big]).max()) if big.any() else 0.0
    print(f"{what}: worst relative error {worst:.3e}")
    assert (err <= rtol * want + ref.SOFTMAX_ATOL).all(), f"{what}: worst relative error {worst:.3e} > {rtol}"


def _assert_same_outputs(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert (x is None) == (y is None)
        if x is not None:
            assert x.dtype == y.dtype and (_bits(x) == _bits(y)).all(), f"{what}: output {i} differs between bf16 and fp16"


def _assert_logits_exact(logits, hidden, w, logit_bias=None):
    x = ref.logits_f64(hidden, w)
    assert (x.astype(np.float32).astype(np.float64) == x).all()  # the data is exact in f32
    x32 = x.astype(np.float32)
    if logit_bias is not None:
        x32 = x32 + logit_bias[None, :]  # one f32 add, as the kernel's
    assert (_bits(logits) == _bits(x32 + np.float32(0.0))).all(), "logits bits"
    return x32.astype(np.float64)


# ------------------------------------------------------------------ 1: router parity on exact data

ROUTER_CASES = {
    # T, H, E, k, shared gate, keyword arguments of moe.gate, e_bias, logit_bias
    "plain_renorm": (33, 128, 8, 2, False, dict(renormalize=True), False, False),
    "plain_shared": (40, 128, 64, 6, True, dict(), False, False),
    "four_wave_form": (100, 64, 256, 5, True, dict(), False, False),
    "rows32_form": (8192 + 5, 64, 60, 4, True, dict(), False, False),
    "rows64_form": (16384 + 33, 96, 64, 6, False, dict(), False, False),
    "sigmoid_bias_groups": (64, 256, 256, 8, False, dict(scoring="sigmoid", n_group=8, topk_group=4, renormalize=True,
                                                         routed_scaling_factor=2.5), True, False),
    "softmax_logit_bias": (48, 128, 32, 4, False, dict(renormalize=True), False, True),
    "wide_sigmoid_bias": (64, 128, 384, 8, False, dict(scoring="sigmoid", renormalize=True, routed_scaling_factor=2.827),
                          True, False),
    "wide_shared": (40, 128, 512, 10, True, dict(renormalize=True), False, False),
}


@pytest.mark.parametrize("case", list(ROUTER_CASES))
def test_router_parity_on_exact_data(case):
    """The bf16 call's logits equal the f64 reference's bits, and its ids, weights and shared_w equal, bit for bit, the
    fp16 call's on the same values (the data is exact in both formats and in the f32 accumulation); the weights also
    lie within SOFTMAX_RTOL of the reference."""
    T, H, E, k, shared, kw, with_e_bias, with_lb = ROUTER_CASES[case]
    hidden, w, sg = bref.exact_data(T, H, E, seed=8, shared=shared)
    # (the biases: tests/_gate_modes_ref.bias_data, integers / 256 — exact sums with the logits' multiples of 2^-6)
    e_bias = mref.bias_data(E, np.random.default_rng(9)) if with_e_bias else None
    lb = mref.bias_data(E, np.random.default_rng(13)) if with_lb else None
    sig = kw.get("scoring") == "sigmoid"
    got = _gate(hidden, w, k, BF, sg, e_bias, lb, return_scores=sig, **kw)
    old = _gate(hidden, w, k, F16, sg, e_bias, lb, return_scores=sig, **kw)
    _assert_same_outputs(got, old, case)
    ids, wts, sw, logits = got[:4]
    x = _assert_logits_exact(logits, hidden, w, lb)
    renorm, scale = bool(kw.get("renormalize")), kw.get("routed_scaling_factor", 1.0)
    if sig:  # the f32 reference routing on the kernel's own scores (tests/test_gate_modes_gpu.py: exactly reproducible)
        scores = got[4]
        _assert_close(scores, ref.sigmoid(x), "scores")
        ng, tg = kw.get("n_group", 1), kw.get("topk_group", 1)
        rids = mref.select(mref.selection_values(scores, e_bias), k, ng, tg, 2 if ng > 1 else 1)
        assert (ids == rids).all(), "topk_ids"
        _assert_close(wts, mref.sigmoid_weights(scores, rids, renorm, scale), "weights")
    else:
        rids, rwts, _, _ = mref.gate(None, None, k, renormalize=renorm, routed_scale=scale, logits=x)
        assert (ids == rids).all(), "topk_ids"
        _assert_close(wts, rwts, "weights")
    if shared:
        _assert_close(sw, ref.sigmoid(hidden.astype(np.float64) @ sg.astype(np.float64)), "shared_w")
    else:
        assert sw is None


@pytest.mark.parametrize("case", bref.ONEHOT_CASES, ids=str)
def test_router_by_construction_against_f64(case):
    """The biased rules end to end against an independent f64 routing: one-hot hidden rows, so the logits are w_gate's
    entries (tests/_gate_modes_ref.py's and _gate_wide_ref.py's cases, the table rounded to bf16). ids and weights
    against the f64 reference from the inputs alone, on the rows whose f64 margins exceed the scores' error bound
    (at most 20 % left out: tests/test_bf16_layer.py); the weights' bound is the existing by-construction tests',
    3 * SOFTMAX_RTOL. And bit for bit the fp16 call's outputs on the same values."""
    T, E, k, n_group, topk_group, seed, H = case
    (hidden, w, bias), (rids, rwts, rs, x), ok = bref.onehot_rows(*case)
    assert (~ok).sum() <= mref.ONEHOT_MAX_DROPPED * T
    kw = dict(scoring="sigmoid", n_group=n_group, topk_group=topk_group, renormalize=True, routed_scaling_factor=2.5,
              return_scores=True)
    got = _gate(hidden, w, k, BF, None, bias, None, **kw)
    _assert_same_outputs(got, _gate(hidden, w, k, F16, None, bias, None, **kw), str(case))
    ids, wts, sw, logits, scores = got
    assert (_bits(logits) == _bits(x.astype(np.float32) + np.float32(0.0))).all(), "logits bits"
    assert (np.abs(scores - rs) <= mref.SCORE_ABS_ERR).all(), "scores"
    _assert_close(scores, rs, "scores")
    assert (ids[ok] == rids[ok]).all(), "topk_ids"
    _assert_close(wts[ok], rwts[ok], "weights", rtol=3 * ref.SOFTMAX_RTOL)


# ------------------------------------------------------------------ 2: the router keeps bf16's range

@pytest.mark.parametrize("T,H,E,k", [(40, 256, 32, 3), (40, 128, 384, 8)])
def test_router_range(T, H, E, k):
    """hidden = integers * 2^17 (Inf as fp16), w_gate = integers * 2^-30 (0 as fp16): the logits are exact in f32 and
    must equal the f64 reference's bits, the ids exactly. Operands rounded to fp16 on the way in give Inf * 0."""
    hidden, w = bref.range_data(T, H, E, seed=3)
    ids, wts, sw, logits = _gate(hidden, w, k, BF, renormalize=True)
    x = _assert_logits_exact(logits, hidden, w)
    assert np.isfinite(logits).all() and (logits != 0).any()
    rids, rwts, _, _ = ref.gate(hidden, w, k, renormalize=True, logits=x)
    assert (ids == rids).all(), "topk_ids"
    _assert_close(wts, rwts, "weights")


# ------------------------------------------------------------------ 3: random bf16 data

def test_router_random_data():
    T, H, E, k = 256, 512, 64, 6
    hidden, w = bref.random_data(T, H, E, seed=5)
    ids, wts, _, logits = _gate(hidden, w, k, BF)
    x = ref.logits_f64(hidden, w)  # the f64 product of the bf16 values
    bar = 1e-3 * np.abs(x) + 1e-3 * np.sqrt(np.mean(x ** 2))  # the project's bar (tests/test_gate_gpu.py)
    print(f"logits: worst |err| / bar {float((np.abs(logits - x) / bar).max()):.3e}")
    assert (np.abs(logits - x) <= bar).all()
    rids, rwts, _, _ = ref.gate(hidden, w, k, logits=logits)  # selection / softmax of the kernel's own logits
    assert (ids == rids).all()
    _assert_close(wts, rwts, "weights")


# ------------------------------------------------------------------ 4: ragged T

@pytest.mark.parametrize("T", [1, 17, 65])
def test_ragged_token_counts_leave_the_padding_alone(T):
    H, E, k, pad = 256, 60, 4, 64
    hidden, w, sg = bref.exact_data(T, H, E, seed=2, shared=True)
    nan_bits = 0x7FC12345
    ids = torch.full((T + pad, k), 0x7FFFFFFF, dtype=torch.int32, device=DEV)
    wts = torch.full((T + pad, k), nan_bits, dtype=torch.int32, device=DEV)
    sw = torch.full((T + pad,), nan_bits, dtype=torch.int32, device=DEV)
    logits = torch.full((T + pad, E), nan_bits, dtype=torch.int32, device=DEV)
    out = (ids[:T], wts[:T].view(torch.float32), sw[:T].view(torch.float32), logits[:T].view(torch.float32))
    moe.gate(_t(hidden, BF), _t(w, BF), k, w_shared_gate=_t(sg, BF), return_logits=True, out=out)
    torch.cuda.synchronize()
    x = _assert_logits_exact(_np(out[3]), hidden, w)
    rids, rwts, rsw, _ = ref.gate(hidden, w, k, w_shared_gate=sg, logits=x)
    assert (_np(ids[:T]) == rids).all()
    _assert_close(_np(out[1]), rwts, "weights")
    _assert_close(_np(out[2]), rsw, "shared_w")
    assert (ids[T:] == 0x7FFFFFFF).all()
    for t in (wts, sw, logits):
        assert (t[T:] == nan_bits).all()


# ------------------------------------------------------------------ 5: the gather

GATHER_TAGS = [moe.ACT_FP16, moe.ACT_INT8, moe.ACT_INT4, moe.ACT_INT4_G128, moe.ACT_MXFP4, moe.ACT_MXFP8]


def _same_batches(a, b, what):
    """Every segment's stored rows and scales byte for byte (what lies between segments is padding)."""
    assert a.qtags == b.qtags
    for e, s in enumerate(a.segs):
        assert s.rows > 0
        x, y = a.A(e), b.A(e)
        assert x.shape == y.shape and torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), \
            f"{what}: seg {e} (tag {a.qtags[e]}) rows differ"
        if a.qtags[e] != moe.ACT_FP16:
            sx, sy = a.scale(e), b.scale(e)
            assert torch.equal(sx.contiguous().view(torch.uint8), sy.contiguous().view(torch.uint8)), f"{what}: seg {e} scales"


@pytest.mark.parametrize("K", [128, 640, 2944])
def test_gather_reads_bf16_rows(K):
    """One expert per tag and a shared expert: every segment's bytes equal those the fp16 pass writes for
    hidden.to(fp16) — zeros, -0, the fp16-subnormal range with its ties, and values beyond fp16 (Inf on both sides)."""
    T, topk, E = 37, 2, len(GATHER_TAGS)
    ids = torch.stack([torch.arange(T) % E, (torch.arange(T) + 1 + torch.arange(T) // E) % E], dim=1)
    ids[:, 1] = torch.where(ids[:, 1] == ids[:, 0], (ids[:, 1] + 1) % E, ids[:, 1])
    r = moe.route(ids.to(torch.int32).to(DEV), E)
    assert min(r.counts) > 0
    hb = _t(bref.gather_edge_rows(T, K, seed=K), BF)
    h16 = hb.to(F16)
    assert torch.isinf(h16[3]).any() and (h16[2, :10].view(torch.int16) != 0).any()
    for shared_tag in (moe.ACT_MXFP8, moe.ACT_INT8):
        tags = GATHER_TAGS + [shared_tag]
        got = moe.quant_act(hb, r, tags, True)
        want = moe.quant_act(h16, r, tags, True)
        torch.cuda.synchronize()
        _same_batches(got, want, f"K={K} shared tag {shared_tag}")
    # without an MX tag (the builds without the MX code), and fp16 through the new entry against the entries it had
    plain = [moe.ACT_FP16, moe.ACT_INT8, moe.ACT_INT4, moe.ACT_INT4_G128, moe.ACT_INT8, moe.ACT_FP16]
    _same_batches(moe.quant_act(hb, r, plain, False), moe.quant_act(h16, r, plain, False), f"K={K} no MX tag")
    for tags, shared in ((GATHER_TAGS + [moe.ACT_INT4], True), (plain, False)):
        want = moe.quant_act(h16, r, tags, shared)
        segs, dsegs, out, scales = moe._segments_of(r, tags, K, K, shared, h16.device)
        nat.check(nat.symbol("mxmoe_moe_gather_quant")(
            nat.DT_FP16, h16.data_ptr(), T, K, topk, int(shared), r.sorted_expert.data_ptr(), r.perm_token.data_ptr(),
            dsegs.data_ptr(), len(segs), moe._tag_mask(tags), out.data_ptr(), scales.data_ptr(), None))
        torch.cuda.synchronize()
        _same_batches(moe.ActBatch(out, scales, segs, list(tags)), want, f"K={K} fp16 through mxmoe_moe_gather_quant")


# ------------------------------------------------------------------ 6: the combine

def _route_ids(T, topk, n_exp, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.topk(torch.rand(T, n_exp, generator=g), topk, dim=1).indices.to(torch.int32)


@pytest.mark.parametrize("biased", [False, True])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("H", [128, 200, 2944])
def test_combine_writes_bf16(H, shared, biased):
    """The f32 fma chain (bias add first) rounded once to bf16, against oracle.moe_ref.fma_f32's restatement; with
    fp16 out the new entry equals the old ones. Data: the recipe of the existing combine tests."""
    T, topk, E = 33, 3, 8
    r = moe.route(_route_ids(T, topk, E, 9).to(DEV), E)
    g = torch.Generator().manual_seed(10 + H)
    y = (torch.rand(T * topk, H, generator=g) * 2 - 1).half()
    w = torch.softmax(torch.rand(T, topk, generator=g), dim=1)
    bias = (torch.rand(E, H, generator=g) * 2 - 1).half() if biased else None
    sh = (torch.rand(T, H, generator=g) * 2 - 1).half() if shared else None
    sw = torch.rand(T, generator=g) if shared else None
    sb = (torch.rand(H, generator=g) * 2 - 1).half() if shared and biased else None
    dev = lambda t: None if t is None else t.to(DEV)
    npy = lambda t: None if t is None else t.numpy()
    inv, sorted_e = _np(r.inv_slot), _np(r.sorted_expert)
    want = bref.combine_bf16(y.numpy(), inv, sorted_e, w.numpy(), topk, npy(bias), E, npy(sh), npy(sw), npy(sb))
    if biased:
        got = moe.combine_bias(dev(y), r, dev(w), dev(bias), dev(sh), dev(sw), dev(sb), out_dtype=BF)
        old = moe.combine_bias(dev(y), r, dev(w), dev(bias), dev(sh), dev(sw), dev(sb))
    else:
        got = moe.combine(dev(y), r, dev(w), dev(sh), dev(sw), out_dtype=BF)
        old = moe.combine(dev(y), r, dev(w), dev(sh), dev(sw))
    assert got.dtype == BF and old.dtype == F16
    assert (_np(got.view(torch.int16)).view(np.uint16) == want).all()
    # fp16 through mxmoe_moe_combine_dt: the old entries' bits
    out16 = torch.empty_like(old)
    keep = [dev(t) for t in (y, w, bias, sh, sw, sb)]  # (alive across the call)
    ptr = lambda t: None if t is None else t.data_ptr()
    nat.check(nat.symbol("mxmoe_moe_combine_dt")(
        nat.DT_FP16, ptr(keep[0]), r.inv_slot.data_ptr(), r.sorted_expert.data_ptr() if biased else None, ptr(keep[1]),
        ptr(keep[2]), ptr(keep[3]), ptr(keep[4]), ptr(keep[5]), T, topk, E, H, out16.data_ptr(), None))
    torch.cuda.synchronize()
    assert torch.equal(out16.view(torch.int16), old.view(torch.int16))
    # without a shared_w (weight one) and bf16 out
    if shared and not biased:
        got1 = moe.combine(dev(y), r, dev(w), dev(sh), None, out_dtype=BF)
        want1 = bref.combine_bf16(y.numpy(), inv, sorted_e, w.numpy(), topk, None, E, npy(sh), None, None)
        assert (_np(got1.view(torch.int16)).view(np.uint16) == want1).all()


# ------------------------------------------------------------------ 7: layers, end to end

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


def _mixed_blocks():
    """(bf16 block, fp16 block on the same MoEFFN and the same router values, T): H 256, N 128, Ns 256, 8 experts and a
    shared one, top-2, qcfgs mixing fp16, w8a8, w4a4 and w4a8_g32_sym_MXFP8."""
    T, topk, E, H, N, Ns = 48, 2, 8, 256, 128, 256
    g = torch.Generator().manual_seed(21)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)
    gate_up = [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)]
    down = [mk(H, N) for _ in range(E)] + [mk(H, Ns)]
    qcfg = [(W8A8, W8A8), (W4A4, W8A8), (FP16, FP16), (W4A8_MXFP8, W4A8_MXFP8), (W4A4, W4A4), (FP16, W8A8),
            (W4A8_MXFP8, W8A8), (W4A4, FP16), (FP16, FP16)]
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    _, w, sg = bref.exact_data(T, H, E, seed=31, shared=True)
    blocks = [moe.MoEBlock(ffn, _t(w, dt), topk, w_shared_gate=_t(sg, dt)) for dt in (BF, F16)]
    return (*blocks, T)


def _gptoss_blocks():
    """(bf16 block, fp16 block, T): a biased SwigluClamp layer, 4 experts, H = N = 128, MXFP4 weights through
    prepare_weight_mx (w4a16_g32_sym_MXFP4), the router with a logit bias."""
    T, topk, E, H, N = 48, 2, 4, 128, 128
    g = torch.Generator().manual_seed(41)

    def weight(rows, K):  # random e2m1 codes, scales 2^-6 .. 2^-4
        codes = torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8)
        scales = torch.randint(121, 124, (rows, K // 32), generator=g, dtype=torch.uint8)
        return moe.prepare_weight_mx(codes.to(DEV), scales.to(DEV), W4A16_MXFP4)

    rnd = lambda *s: torch.rand(*s, generator=g) * 2 - 1
    ffn = moe.MoEFFN([weight(2 * N, H) for _ in range(E)], [weight(H, N) for _ in range(E)], [(W4A16_MXFP4, W4A16_MXFP4)] * E,
                     num_routed=E, gate_up_bias=list((rnd(E, 2 * N) * 0.5).to(DEV)), down_bias=list((rnd(E, H) * 0.5).to(DEV)),
                     activation=moe.SwigluClamp())
    assert ffn.b2.dtype == F16 and ffn.b1.dtype == F16 and ffn.b1.is_cuda and ffn.b2.is_cuda  # the biases stay fp16
    _, w, _ = bref.exact_data(T, H, E, seed=43)
    lb = mref.bias_data(E, np.random.default_rng(44))
    blocks = [moe.MoEBlock(ffn, _t(w, dt), topk, renormalize=True, logit_bias=torch.from_numpy(lb).to(DEV)) for dt in (BF, F16)]
    return (*blocks, T)


def _want_out(ffn, y, ys, inv, sorted_e, wts, sw, topk):
    """test 6's bf16 combine reference applied to the layer's own down outputs"""
    E, b2, b2s = ffn.down_bias if ffn.down_bias is not None else (ffn.E, None, None)
    return bref.combine_bf16(_np(y), _np(inv), _np(sorted_e), _np(wts), topk, _np(b2), E, _np(ys), _np(sw), _np(b2s))


def _out_bits(t):
    assert t.dtype == BF
    return _np(t.view(torch.int16)).view(np.uint16)


@pytest.mark.parametrize("make", [_mixed_blocks, _gptoss_blocks], ids=["mixed_qcfgs", "gptoss_biased"])
def test_layer_end_to_end(make):
    """A bf16 MoEBlock against the fp16 block on the same values, as forward, PlannedForward, GraphForward.launch and
    one captured graph replayed on two routings: ids, weights, y and ys identical, out = the bf16 combine reference
    applied to that y. (Each form against the fp16 run of the SAME form: their GroupGEMM plans are the same ones.)"""
    bb, b16, T = make()
    ffn, topk, H = bb.ffn, bb.topk, bb.ffn.H
    hiddens = [bref.exact_data(T, H, ffn.E, seed=s)[0] for s in (51, 52)]
    assert not np.array_equal(hiddens[0], hiddens[1])
    gf, gf16 = moe.GraphForward(bb, T), moe.GraphForward(b16, T)
    assert gf.dtype == BF and gf.out.dtype == BF and gf16.out.dtype == F16 and gf.y.dtype == F16 and gf.h1.dtype == F16
    with pytest.raises(ValueError):
        gf.launch(_t(hiddens[0], F16))
    with pytest.raises(ValueError):
        bb.forward(_t(hiddens[0], F16))
    static = _t(hiddens[0], BF).clone()
    graph = _captured(gf, static)
    routings = []
    for hid in hiddens:
        hb, h16 = _t(hid, BF), _t(hid, F16)
        # eager
        out, mid = bb.forward(hb, return_intermediates=True)
        out16, mid16 = b16.forward(h16, return_intermediates=True)
        torch.cuda.synchronize()
        assert out.dtype == BF and out16.dtype == F16
        for k in ("topk_ids", "topk_weights", "shared_w", "y", "ys"):
            assert (mid[k] is None) == (mid16[k] is None)
            if mid[k] is not None:
                assert torch.equal(mid[k].view(torch.int32) if mid[k].dtype != F16 else mid[k].view(torch.int16),
                                   mid16[k].view(torch.int32) if mid16[k].dtype != F16 else mid16[k].view(torch.int16)), k
        r = mid["routing"]
        ids, wts, sw = mid["topk_ids"], mid["topk_weights"], mid["shared_w"]
        routings.append(_np(ids))
        assert (_out_bits(out) == _want_out(ffn, mid["y"], mid["ys"], r.inv_slot, r.sorted_expert, wts, sw, topk)).all(), "forward"
        # planned
        pf, pf16 = moe.PlannedForward(ffn, hb, ids, wts), moe.PlannedForward(ffn, h16, ids, wts)
        sw_p = None  # (PlannedForward takes no shared_w: the shared expert's weight is one)
        got_p, got_p16 = pf(), pf16()
        torch.cuda.synchronize()
        assert got_p.dtype == BF and torch.equal(pf.y.view(torch.int16), pf16.y.view(torch.int16))
        assert (pf.ys is None) == (pf16.ys is None) and (pf.ys is None or torch.equal(pf.ys.view(torch.int16), pf16.ys.view(torch.int16)))
        assert (_out_bits(got_p) == _want_out(ffn, pf.y, pf.ys, pf.r.inv_slot, pf.r.sorted_expert, wts, sw_p, topk)).all(), "planned"
        # graph forward, eager launches
        for which in ("launch", "replay"):
            if which == "launch":
                gf.launch(hb)
            else:
                static.copy_(hb)
                graph.replay()
            gf16.launch(h16)
            torch.cuda.synchronize()
            g_ids, g_wts, g_sw = gf.gate_out
            assert torch.equal(g_ids, ids) and torch.equal(g_wts.view(torch.int32), wts.view(torch.int32)), which
            assert torch.equal(gf.gate_out[0], gf16.gate_out[0]) and torch.equal(gf.gate_out[1].view(torch.int32),
                                                                                gf16.gate_out[1].view(torch.int32)), which
            assert torch.equal(gf.y.view(torch.int16), gf16.y.view(torch.int16)), which
            if gf.ys is not None:
                assert torch.equal(gf.ys.view(torch.int16), gf16.ys.view(torch.int16)), which
            sorted_e, _, inv, _ = gf.route_bufs
            assert (_out_bits(gf.out) == _want_out(ffn, gf.y, gf.ys, inv, sorted_e, g_wts, g_sw, topk)).all(), which
            assert gf.status() == 0 and gf16.status() == 0, which
    assert not np.array_equal(routings[0], routings[1]), "the two replays must see different routings"
