"""GPU tests of the decode forward's MFMA tile on edge values and shapes (mxmoe_amd/csrc/moe_decode_mfma.h; DESIGN.md §4
"Decode forward on MFMA"), bit for bit: the operands of tests/_decode_lp_edges.py, whose CPU file
(tests/test_decode_lp_edges.py) proves for every problem run here that the kernel's f32 sums are exact in any order and
that a kernel wrong in the way a docstring names would give other bits.

The reference is float64 arithmetic on the operands the contract defines, rounded to fp16 once; fp16 bits are compared,
NaN by isnan. The entries run on raw expert records (L-a, L-c, L-d, L-e) or through moe.DecodeForwardLp beside the eager
layer built from the same prepared weights (L-b). Every output buffer is pre-filled with the guard pattern and carries
one row behind the last pair, which must keep it."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4_MXFP4, W4A8_MXFP8, W4A16_ASYM, W8A8, W8A8_E4M3
from tests import _decode_lp_edges as ed
from tests._decode_util import DEV, GUARD, assert_act_close, biases, bits, check_stages, down_raw, guard
from tests._fp8_bf16_edges import mismatch
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
QP = {"e4m3": W8A8_E4M3, "mxfp8": W4A8_MXFP8, "mxfp4": W4A4_MXFP4, "w8a8": W8A8, "fp16": FP16,
      "w4a16": W4A16_ASYM}
KIND = {"e4m3": nat.DECODE_W8A8_E4M3, "mxfp8": nat.DECODE_W4A8_MXFP8, "mxfp4": nat.DECODE_W4A4_MXFP4,
        "w8a8": nat.DECODE_W8A8, "fp16": nat.DECODE_FP16, "w4a16": nat.DECODE_W4A16_ASYM}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _prep(w: ed.Weight, kind: str) -> moe.ExpertWeights:
    if kind in ed.OTHER_KINDS:
        return moe.prepare_weight(_dev(w.fp16()), QP[kind])
    if w.mx:
        return moe.prepare_weight_mx(_dev(w.packed()), _dev(w.scales), QP[kind], warn=False)
    return moe.prepare_weight_e4m3(_dev(w.codes), _dev(w.scales), warn=False)


def _records(kinds, ws1, ws2):
    """(device records, kind mask, the tensors they point to) of raw experts; a missing side repeats the other"""
    tables, keep = (nat.MoeDecodeExpertC * len(kinds))(), []
    for rec, k, w1, w2 in zip(tables, kinds, ws1, ws2):
        p1, p2 = _prep(w1, k), _prep(w2, k)
        keep += [p1, p2]
        sb = lambda p: 0 if p.scale_b is None else p.scale_b.data_ptr()
        for p in (p1, p2):
            assert p.B.data_ptr() % 16 == 0 and sb(p) % 4 == 0
        rec.b1, rec.sb1, rec.kind1 = p1.B.data_ptr(), sb(p1), KIND[k]
        rec.b2, rec.sb2, rec.kind2 = p2.B.data_ptr(), sb(p2), KIND[k]
    mask = 0
    for k in kinds:
        mask |= 1 << KIND[k]
    return torch.frombuffer(bytearray(bytes(tables)), dtype=torch.uint8).to(DEV), mask, keep


def _guarded(rows, cols):
    t = torch.empty(rows + 1, cols, dtype=torch.float16, device=DEV)
    bits(t).fill_(GUARD)
    return t


def _assert_bits(out: torch.Tensor, want: np.ndarray, what: str):
    got = out.cpu().numpy()
    assert (got[-1].view(np.uint16) == GUARD).all(), f"{what}: the guard row was written"
    bad = mismatch(got[:-1], want)
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}: " \
                          f"{got[:-1][bad][:4]} != {want[bad][:4]}"


def _run_down(p: ed.DownProblem):
    """mxmoe_moe_decode_down_lp on the problem's raw records; y and ys against p.expected, bit for bit."""
    p.assert_exact()
    T, topk = p.ids.shape
    N, Ns = p.act.shape[1], p.act_shared.shape[1]
    experts, mask, keep = _records(p.kinds, p.weights, p.weights)
    ids = _dev(p.ids)
    assert int(ids.min()) >= 0 and int(ids.max()) < p.E
    y, ys = _guarded(T * topk, p.H), _guarded(T, p.H)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    down_raw("lp", T, topk, p.E, 1, ids, experts, mask, p.H, N, Ns, _dev(p.act), _dev(p.act_shared), y, ys, status)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    want, want_s = p.expected
    _assert_bits(y, want, p.name + " (y)")
    _assert_bits(ys, want_s, p.name + " (ys)")
    return y[:-1].cpu().numpy(), ys[:-1].cpu().numpy()


@pytest.mark.parametrize("K", [640, 1152])
@pytest.mark.parametrize("kind", ed.KINDS)
def test_la_quantiser_readout(kind, K):
    """L-a (gap 5). One-hot weight rows read out every position of the A rows lp_quant_row wrote: zero, -0, subnormal,
    65504, below the E4M3 scale floor, every e4m3 / e2m1 rounding tie and values above saturation, MX blocks on a
    ladder of exponents with zero blocks between, +Inf and NaN rows (an e8m0 byte 255 on the A side: the row is NaN,
    0 * NaN). Catches a quantiser that rounds ties away from zero, leaves the 2^-14 floor out, keeps an Inf block's
    codes, pairs an A block with another block's or step's scale byte, or swaps the 64-byte halves of an fp8 step."""
    _run_down(ed.la_problem(kind, K))


@pytest.mark.parametrize("T", [7, 16])
def test_lc_e4m3_scale_ladder(T):
    """L-c (gap 5). scale_a = 2^k against a ladder of scale_b: the epilogue fp16_rn(acc * f32(fp16_rn(sa * sb))) with
    products that are ordinary, a tie on fp16's grid, subnormal, zero by underflow and overflowing. Catches a scale
    product not rounded on its own, a flushed subnormal product and an output tie rounded away from zero."""
    y, ys = _run_down(ed.lc_problem(T))
    both = np.concatenate([y.ravel(), ys.ravel()])
    assert (both == np.inf).any() and (both == -np.inf).any()
    assert ((both != 0) & (np.abs(both.astype(np.float64)) < 2.0 ** -14)).any()


@pytest.mark.parametrize("T", [1, 7, 16])
@pytest.mark.parametrize("kind", ["mxfp8", "mxfp4"])
def test_ld_mx_scale_range(kind, T):
    """L-d (gap 1). One e8m0 byte per weight row on a ladder 99 .. 155, one per A row: sa + sb - 254 reaches both ends of
    fp16. Catches a scale exponent clipped or wrapped by the tile and an output conversion that flushes subnormals or
    saturates instead of overflowing."""
    y, ys = _run_down(ed.ld_problem(kind, T))
    both = np.concatenate([y.ravel(), ys.ravel()])
    assert np.isinf(both).any() and ((both != 0) & (np.abs(both.astype(np.float64)) < 2.0 ** -14)).any()


@pytest.mark.parametrize("kind", ed.KINDS)
def test_le_cut_batches(kind):
    """L-e (ii) (gaps 2 and 4). K = 4096 (S = 32: eight trips of the K loop for fp8 weights, four for fp4; eight scale
    groups): lp_lds cuts the E4M3 / MXFP8 batch to 14 rows, so the 64 rows of expert 2 run as 14 + 14 + 14 + 14 + 8
    and the shared expert's as 14 + 2. The weight column that meets the rows' scale-selecting element (448 / 256 code
    units) holds a small nonzero code, so that element is part of every sum. Catches a batch that re-reads the previous
    batch's rows or scales, a row index that forgets r0, and a scale group of s0 == 0 reused on a later trip."""
    p = ed.le_cut_problem(kind)
    assert p.info["rb"] == (16 if kind == "mxfp4" else 14)
    _run_down(p)


@pytest.mark.parametrize("ct", [64, 128])
def test_le_wide_tiles_down(ct):
    """L-e (i), down (gap 3). geometry() (mxmoe_amd/csrc/moe_decode.h): cols = min(E, T topk) C + C_shared; ct starts at
    128 and is halved while cols / ct < 1024. E = 64, T = 16, topk = 4 with C = H = 1024 gives ct = 64 and C = 2048
    ct = 128 (asserted through ed.decode_ct; C is the smallest that does): all four waves of lp_tile work and the n
    loop takes a second trip at ct = 128. Experts cycle through E4M3, MXFP8, MXFP4, w8a8 and fp16, so lp_tile and
    expert_tile both run with more than two column groups per workgroup. Catches a column group skipped,
    written twice or paired with another group's weight rows."""
    p = ed.le_wide_down_problem(ct)
    assert ed.decode_ct(p.E, 16, 4, p.H, p.H) == ct
    _run_down(p)


@pytest.mark.parametrize("kind", ed.KINDS)
def test_lf_dense_down(kind):
    """L-f (gaps 1 and 2). The down entry alone on dense exact sums with cancellation at K = 1152 (S = 9), weight bytes
    of four values per block and A scales of four values. Catches, on the down entry, a weight or A scale byte of the
    neighbouring block, of step u ^ 1 of its dword, the 16-byte group of s0 == 0 reused at s0 > 0, and swapped halves
    of an fp8 step."""
    _run_down(ed.dense_down_problem(kind))


def _run_layer(case: ed.LayerCase, variant: str = "plain", stages=("act", "y", "out")):
    """L-b's checks on one layer case; variant: plain | interleaved (fp16 tensors that MoEFFN interleaves and
    quantises again, to the same codes and bytes) | bias_clamp | bf16. stages: what is compared with the eager layer
    bit for bit; without "y" the down stage is not compared with its f64 reference either."""
    T, topk = case.ids.shape
    E = case.E
    g = torch.Generator().manual_seed(77)
    qcfg = [(QP[k1], QP[k2]) for k1, k2 in case.pairs]
    if variant == "interleaved":
        f16 = lambda w: torch.from_numpy(w.values()).half().to(DEV)
        w1, w2, kw = [f16(w) for w in case.w1], [f16(w) for w in case.w2], dict(fuse_silu=True)
    else:
        w1 = [_prep(w, k[0]) for w, k in zip(case.w1, case.pairs)]
        w2 = [_prep(w, k[1]) for w, k in zip(case.w2, case.pairs)]
        kw = {}
    b1 = None
    if variant == "bias_clamp":
        b1, b2 = biases(g, E, case.H, case.N, case.Ns)
        kw = dict(gate_up_bias=b1, down_bias=b2, activation=moe.SwigluClamp())
    ffn = moe.MoEFFN(w1, w2, qcfg, num_routed=E, **kw)
    assert ffn.fuse_silu == (variant == "interleaved")
    dtype = torch.bfloat16 if variant == "bf16" else torch.float16
    cap = min(T + 1, 16)  # a spare row behind the call's pairs where the capacity allows one
    df = moe.DecodeForwardLp(ffn, cap, topk, dtype=dtype)
    bufs = guard(df)
    h = _dev(case.hidden).to(dtype)
    assert torch.equal(h.to(torch.float16).cpu(), torch.from_numpy(case.hidden))  # (bf16 holds the exact rows)
    ids = _dev(case.ids)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
    sw = torch.rand(T, generator=g).to(DEV)
    # a layer with a w8a8 or w4a16 down (L-b "mixed"): act here, y and out expert by expert in _check_other_downs
    others = any(p[1] not in ed.KINDS for p in case.pairs)
    mid = check_stages(df, ffn, h, ids, wts, sw, stages=("act",) if others else stages)
    assert df.status() == 0
    n = T * topk
    if cap > T:
        for t in bufs:
            assert (bits(t[n if t.shape[0] == cap * topk else T:]) == GUARD).all()
    act, act_s = df.act[:n].cpu().numpy(), df.act_shared[:T].cpu().numpy()
    y, ys = df.y[:n].cpu().numpy(), df.ys[:T].cpu().numpy()
    # the down stage on the device's own act: exact by the bound, then bit for bit the f64 reference
    down = "y" in stages
    assert np.isfinite(act).all()
    assert not down or (case.bound2(act, act_s) < case.limit(1) and case.span2(act, act_s) < ed.SPAN)
    act_fn = "clamp" if variant == "bias_clamp" else "silu"
    glu = dict(alpha=ffn.activation.alpha, limit=ffn.activation.limit) if variant == "bias_clamp" else {}
    if others and down:
        _check_other_downs(case, df, ffn, mid, h, ids, wts, sw)
    for p, e in enumerate(case.ids.reshape(-1)):
        bad = mismatch(y[p:p + 1], case.y_ref(e, act[p:p + 1])) if down and case.pairs[e][1] in ed.KINDS else np.zeros(1, bool)
        assert not bad.any(), f"{case.name}: y row {p} (expert {e}): {bad.sum()} differ"
        try:
            assert_act_close(act[p:p + 1], case.gu_ref(e, case.hidden[p // topk:p // topk + 1]),
                             None if b1 is None else ffn.b1[e].cpu().numpy(), act_fn, glu)
        except AssertionError as err:
            raise AssertionError(f"{case.name}: act row {p} (expert {e}, {case.pairs[e][0]}): {err}") from None
    bad = mismatch(ys, case.y_ref(E, act_s)) if down and case.pairs[E][1] in ed.KINDS else np.zeros(1, bool)
    assert not bad.any(), f"{case.name}: ys: {bad.sum()} differ"
    assert_act_close(act_s, case.gu_ref(E, case.hidden), None if b1 is None else ffn.b1s.cpu().numpy(), act_fn, glu)


def _check_other_downs(case: ed.LayerCase, df, ffn, mid, h, ids, wts, sw):
    """y and out of a layer that holds w8a8 and w4a16 downs, against the eager layer. Bit for bit: y of every expert
    whose down is E4M3, MXFP8, MXFP4 (exact sums) or w8a8 (integer sums; ys here), and out of every token none of
    whose experts has a w4a16 down. A w4a16 down sums fp16 act values of 11 significant bits in f32, in another order
    than the GroupGEMM, so no data make it exact: its y rows, and out of its tokens, are held to assert_f16_close of
    the eager layer and (y) of the f64 reference."""
    T, topk = case.ids.shape
    flat = case.ids.reshape(-1)
    want = ffn.forward(h, ids, wts, sw)
    torch.cuda.synchronize()
    inv = mid["routing"].inv_slot.long()
    ey, y = mid["y"][inv].cpu().numpy(), df.y[:T * topk].cpu().numpy()
    act = df.act[:T * topk].cpu().numpy()
    loose = np.array([case.pairs[e][1] == "w4a16" for e in flat])
    assert not mismatch(y[~loose], ey[~loose]).any(), "down (routed y)"
    for p in np.nonzero(loose)[0]:
        assert_f16_close(y[p:p + 1], ey[p:p + 1], case.N)
        assert_f16_close(y[p:p + 1], case.y_ref(flat[p], act[p:p + 1]), case.N)
    ys = df.ys[:T].cpu().numpy()
    assert case.pairs[case.E][1] == "w8a8" and not mismatch(ys, mid["ys"].cpu().numpy()).any(), "down (shared ys)"
    assert_f16_close(ys, case.y_ref(case.E, df.act_shared[:T].cpu().numpy()), case.Ns)
    got, want = df.out[:T].float().cpu().numpy(), want.float().cpu().numpy()
    tok = loose.reshape(T, topk).any(axis=1)
    assert np.array_equal(got[~tok], want[~tok]), "combine"
    if tok.any():
        assert_f16_close(got[tok], want[tok], case.H)


@pytest.mark.parametrize("ct", [64, 128])
def test_le_wide_tiles_gate_up(ct):
    """L-e (i), gate_up (gap 3). A layer of 64 experts cycling through E4M3, MXFP8, MXFP4, w8a8 and fp16 with H = 128 and
    N = 1024 / 2048 (ct = 64 / 128 by geometry()'s rule, asserted through ed.decode_ct): act and act_shared equal the
    eager layer's bit for bit (the gate_up sums are exact, the CPU file asserts their bounds) and stay within
    assert_act_close of the f64 reference. Both accumulators of a lane, all four waves, the second trip of the n loop,
    in lp_tile and expert_tile. Catches a gate / up column group skipped, written twice or fed another group's rows."""
    case = ed.wide_layer_case(ct)
    assert ed.decode_ct(case.E, 16, 4, case.N, case.Ns) == ct
    _run_layer(case, stages=("act",))


@pytest.mark.parametrize("name,shape,T", ed.LB_CASES)
def test_lb_exact_sums(name, shape, T):
    """L-b (gaps 1 and 2). Dense exact sums through both entries at K = 128 / 512 / 640 / 1024 / 1152 on either side
    (S = 1, 4, 5, 8 and 9: S == kSteps for both weight widths, the second trip of the K loop for fp4 weights and a
    third 16-byte scale group), weight and A scale bytes varied per block. act, y and out equal the eager layer's bit
    for bit, y and ys the f64 reference of the device's own act, act stays within assert_act_close. "cross": the experts'
    gate_up and down kinds differ (E4M3 -> MXFP8, MXFP8 -> MXFP4, MXFP4 -> E4M3: act written for one kind and quantised
    by another, kind1 != kind2 in a record). "mixed": the whole MIXED list of tests/test_decode_lp_gpu.py, with a
    (w8a8, w4a16_asym) expert and a (w4a16_asym, w8a8) shared one: everything bit for bit but what the w4a16 down
    touches (_check_other_downs). Catches a weight
    or A scale byte of the neighbouring block, of step u ^ 1 of its dword, the scale group of s0 == 0 reused at
    s0 > 0, a step offset that forgets s0 and swapped halves of an fp8 step."""
    _run_layer(ed.layer_case(name, shape, T))


@pytest.mark.parametrize("variant", ["interleaved", "bias_clamp", "bf16"])
def test_lb_layouts_and_ends(variant):
    """L-b at H = 640, N = 1024 with MXFP8 activations: the interleaved gate_up layout (weight rows 2 n + r16 and + 16),
    the four biases with the clamped SwiGLU, and bf16 hidden / out. Catches a gate / up row pairing of the other layout
    and a bias column offset."""
    _run_layer(ed.layer_case("mxfp8", "c", 5, clamp=variant == "bias_clamp", anchor=variant == "interleaved"), variant)
