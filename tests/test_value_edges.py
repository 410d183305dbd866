"""What the value-edge inputs of tests/test_value_edges_gpu.py contain, proved on the CPU.

The GPU file compares kernels with the oracle on operands chosen for their VALUES (tests/_util.py
generators). Two things are shown here, with the oracle alone, so that the GPU tests cannot lose
their coverage silently:

  * class coverage: every family contains each value class it is built for (an extreme code, an
    accumulator above 2^24, a subnormal / tie / underflowing scale product, an output that is +-inf,
    subnormal or +0 from acc == 0, a quantiser tie, a clamped code, ...), and no oracle output is NaN;
  * sensitivity: a deliberately wrong numpy restatement of the reference differs from the true oracle
    on the family. Each numpy restatement is first checked to equal the C / numpy oracle bit for bit.

Wrong reference                                         caught by
  unpack clamps -128 / -8 to -127 / -7                   full range (w8a8, w4a4, w4a4 g128)
  scale product flushed to zero when subnormal           scale ladder (w8a8, w4a4), g128 "steps"
  acc in exact arithmetic instead of f32(acc)            large accumulators (the tie pair)
  g128 fold in reversed group order                      g128 "cancel"
  g128 fold as a separate multiply and add               NOTHING, provably: |acc_g| <= 8192 has at most
                                                         13 significant bits (8192 itself one) and the
                                                         fp16 scale product 11, so f32(acc_g) * s is
                                                         exact in f32 and fmaf(a, s, o) == a * s + o for
                                                         every input (test_g128_unfused_fold_is_the_same_function)
  dequant as u*s + fp16(zp - off*s) (two roundings)      dequant readout, 4- and 8-bit sym types (asym:
                                                         off = 0, 2-bit sym: off * s = s is exact — the
                                                         same function there)
  quantiser rounds half away from zero                   activation rows, kind "tie"
  quantiser leaves scale 0 as 0                          activation rows, kinds "zero" and "tiny"
  split-row amax from quarter 0 only                     split rows (peak in quarters 1-3)
"""
from __future__ import annotations

import numpy as np
import pytest

from mxmoe_amd.groupgemm import W4A4, W4A4_G128, W8A8
from oracle import moe_ref, oracle, weightonly
from tests import _util as U
from tests._util import HostProblem

INT_QS = [W8A8, W4A4, W4A4_G128]
INT_IDS = ["w8a8", "w4a4", "w4a4g128"]


def _bits(x):
    return np.ascontiguousarray(x, np.float16).view(np.uint16)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _expected(raw):
    return HostProblem.from_raw(raw, None).expected()


def _subnormal(x):
    b = _bits(x) & 0x7FFF
    return (b > 0) & (b < 0x0400)


# ------------------------------------------------------------------ numpy restatements (true and wrong)
def np_gg_quant(raw, clamp=False, flush=False, exact_acc=False):
    qa, qb = U.raw_codes(raw)
    if clamp:
        lo = -(1 << (raw.q.a_bits - 1)) + 1
        qa, qb = np.maximum(qa, lo), np.maximum(qb, lo)
    acc = oracle.acc_exact(qa, qb)
    s16 = U.raw_scale_product(raw)[1]
    if flush:
        s16 = np.where(_subnormal(s16), np.float16(0), s16)
    with np.errstate(over="ignore"):  # outputs that overflow to inf are a class of their own
        if exact_acc:  # the exact product (25 + 11 bits fit f64), one rounding to fp16
            return (acc.astype(np.float64) * s16.astype(np.float64) + 0.0).astype(np.float16)
        return (np.float32(0) + acc.astype(np.float32) * s16.astype(np.float32)).astype(np.float16)


def _fma_f32(a, b, c):
    """fmaf on f32 arrays whose product is exact in f64: the f64 sum is rounded to odd (TwoSum gives
    the error's sign), then to f32 — one rounding of the exact a * b + c."""
    p = a.astype(np.float64) * b.astype(np.float64)
    o = c.astype(np.float64)
    t = p + o
    bp = t - o
    err = (p - bp) + (o - (t - bp))
    ti = t.view(np.int64).copy()
    fix = (err != 0) & ((ti & 1) == 0)
    up = (err > 0) == (t > 0)
    ti = np.where(fix, np.where(up, ti + 1, ti - 1), ti)
    return ti.view(np.float64).astype(np.float32)


def np_gg_grouped(raw, fused=True, reverse=False, clamp=False, flush=False):
    qa, qb = U.raw_codes(raw)
    if clamp:
        qa, qb = np.maximum(qa, -7), np.maximum(qb, -7)
    G = raw.K // 128
    s16 = U.raw_scale_product(raw)[1]
    if flush:
        s16 = np.where(_subnormal(s16), np.float16(0), s16)
    out = np.zeros((raw.M, raw.N), np.float32)
    for g in (range(G - 1, -1, -1) if reverse else range(G)):
        acc = oracle.acc_exact(qa[:, g * 128:(g + 1) * 128], qb[:, g * 128:(g + 1) * 128]).astype(np.float32)
        s = s16[g].astype(np.float32)
        out = _fma_f32(acc, s, out) if fused else (acc * s).astype(np.float32) + out
    with np.errstate(over="ignore"):
        return out.astype(np.float16)


def np_int(raw, **kw):
    return np_gg_grouped(raw, **kw) if raw.q.gsize == 128 else np_gg_quant(raw, **kw)


def np_quant_rows(x, qmax, half_away=False, keep_zero_scale=False, amax_cols=None):
    """oracle_quant_rtn_sym in numpy: (codes int32 [R, W], scales fp16 [R])."""
    xf = x.astype(np.float32)
    amax = np.abs(xf[:, :amax_cols] if amax_cols else xf).max(axis=1)
    s = (amax / np.float32(qmax)).astype(np.float16)
    if not keep_zero_scale:
        s = np.where(s == 0, np.float16(1), s)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = (xf / s.astype(np.float32)[:, None]).astype(np.float16).astype(np.float32)
    d = np.clip(d, -qmax, qmax)
    q = np.where(np.isnan(d), 0, np.sign(d) * np.floor(np.abs(d) + 0.5) if half_away else np.rint(d))
    return q.astype(np.int32), s


def np_dequant(raw, two_roundings=False):
    q = raw.q
    G = 1 if q.gsize == -1 else raw.K // q.gsize
    g = raw.K // G
    off = weightonly.sym_offset(q.w_bits, q.sym)
    if q.sym:
        s = raw.sb.reshape(G, raw.N).T.astype(np.float64)
        z = np.zeros_like(s)
    else:
        t = raw.sb.reshape(G, raw.N, 2).transpose(1, 0, 2).astype(np.float64)
        s, z = t[..., 0], t[..., 1]
    s, z = np.repeat(s, g, axis=1), np.repeat(z, g, axis=1)
    u = raw.qb.astype(np.float64) + off
    if two_roundings:
        return (u * s + (z - off * s).astype(np.float16).astype(np.float64)).astype(np.float16)
    return ((u - off) * s + z).astype(np.float16)


# ------------------------------------------------------------------ (a) full code range
@pytest.mark.parametrize("q", INT_QS, ids=INT_IDS)
def test_full_range_classes_and_clamped_unpack(q):
    lo = -(1 << (q.a_bits - 1))
    caught = 0
    for raw in U.full_range_problems(q):
        qa, qb = U.raw_codes(raw)
        assert qa.min() == lo and qb.min() == lo and qa.max() == -lo - 1 and qb.max() == -lo - 1
        assert len(np.unique(raw.B)) == 256 and (raw.A.size < 512 or len(np.unique(raw.A)) == 256)
        assert ((qa[0] == lo) & (qb[0] == lo)).any(), "no (-extreme)^2 product"
        ref = _expected(raw)
        assert np.isfinite(ref).all()
        assert _same(np_int(raw), ref)
        caught += not _same(np_int(raw, clamp=True), ref)
    assert caught == len(U.full_range_problems(q))


# ------------------------------------------------------------------ (b) large accumulators
@pytest.mark.parametrize("splitk", [False, True], ids=["plain", "splitk"])
def test_large_acc_classes_and_exact_acc(splitk):
    seen_zero = False
    for raw in U.large_acc_problems(splitk):
        acc = U.raw_acc(raw)
        ref = _expected(raw)
        assert np.abs(acc).max() == 16384 * raw.K > 2 ** 24
        assert (acc.astype(np.float32).astype(np.int64) != acc).any(), "every acc exact in f32"
        assert np.isfinite(ref).all()
        zero = acc == 0
        seen_zero |= bool(zero.any())
        assert (_bits(ref)[zero] == 0).all()  # +0, not -0
        m, n = raw.info["tie"]
        assert acc[m, n] == raw.info["target"] and float(ref[m, n]) == 4 * raw.info["X"]
        assert _same(np_gg_quant(raw), ref)
        wrong = np_gg_quant(raw, exact_acc=True)
        assert float(wrong[m, n]) == 4 * (raw.info["X"] + 1) and not _same(wrong, ref)
    assert seen_zero, "no accumulator cancels to 0"


# ------------------------------------------------------------------ (c) scale ladder
def _tie(ex, r16):
    """exact f64 values lying exactly halfway between two fp16 neighbours (r16 = their rounding)."""
    r = r16.astype(np.float64)
    other = np.nextafter(r16, np.where(ex > r, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
    return (ex != r) & np.isfinite(other) & (np.abs(ex - r) == np.abs(other.astype(np.float64) - ex))


@pytest.mark.parametrize("q", [W8A8, W4A4], ids=["w8a8", "w4a4"])
def test_scale_ladder_classes_and_flushed_product(q):
    for raw in U.ladder_problems(q):
        ex, s16 = U.raw_scale_product(raw)
        acc = U.raw_acc(raw)
        ref = _expected(raw)
        assert np.isfinite(s16).all() and not np.isnan(ref).any()
        normal = (_bits(s16) & 0x7FFF) >= 0x0400
        assert (normal & (ex == s16.astype(np.float64))).any() and (normal & (ex != s16.astype(np.float64))).any()
        assert (_tie(ex, s16) & normal).any(), "no rounding tie among normal products"
        assert (_tie(ex, s16) & _subnormal(s16)).any(), "no tie among subnormal products"
        assert _subnormal(s16).any() and ((s16 == 0) & (ex > 0)).any()
        assert (ref == np.inf).any() and (ref == -np.inf).any()
        assert _subnormal(ref).any()
        assert ((acc == 0) & (s16 != 0)).any() and (_bits(ref)[acc == 0] == 0).all()
        assert (np.abs(acc) == 0).all(axis=1).any(), "no all-zero A row"
        assert _same(np_gg_quant(raw), ref)
        assert not _same(np_gg_quant(raw, flush=True), ref)


@pytest.mark.parametrize("kind", U.G128_KINDS)
def test_g128_ladder_classes_and_group_order(kind):
    for raw in [r for r in U.ladder_problems(W4A4_G128) if r.info["kind"] == kind]:
        ex, s16 = U.raw_scale_product(raw)
        acc = U.raw_acc(raw)
        ref = _expected(raw)
        assert np.isfinite(s16).all() and not np.isnan(ref).any()
        assert _same(np_gg_grouped(raw), ref)
        e = np.log2(s16.astype(np.float64).max(axis=(1, 2)))
        if kind == "steps":
            assert _subnormal(s16).any() and ((s16 == 0) & (ex > 0)).any() and _subnormal(ref).any()
            assert e.max() - e.min() > 7.9 and (np.diff(e) > 0).any() and (np.diff(e) < 0).any()
            assert not _same(np_gg_grouped(raw, flush=True), ref)
        elif kind == "dominant":
            assert np.sort(e)[-1] - np.sort(e)[-2] >= 20
            assert (ref == np.inf).any() and (ref == -np.inf).any() and np.isfinite(ref).any()
        else:
            assert (acc[1] == -acc[0]).all() and (acc[0] != 0).any()
            assert np.array_equal(_bits(s16[0]), _bits(s16[1])) and e[0] - e[2] >= 20
            assert np.isfinite(ref).all() and (ref != 0).any()
            assert not _same(np_gg_grouped(raw, reverse=True), ref)


def test_g128_unfused_fold_is_the_same_function():
    """out = fmaf(f32(acc_g), s, out) against a separate multiply and add: |acc_g| <= 8 * 8 * 128 = 8192
    has at most 13 significant bits and an fp16 value 11, so the f32 product is exact and both forms
    round the same exact sum once. No input tells them apart; the crafted ones do not either."""
    assert 8191 * 2047 < 2 ** 24  # the widest significands (8192 = 2^13 has one bit)
    for raw in U.ladder_problems(W4A4_G128) + U.full_range_problems(W4A4_G128):
        assert np.abs(U.raw_acc(raw)).max() <= 8192
        assert _same(np_gg_grouped(raw, fused=False), _expected(raw))


# ------------------------------------------------------------------ (d) dequant readout
@pytest.mark.parametrize("q", U.WO_READOUT_QS, ids=[q.qcfg for q in U.WO_READOUT_QS])
def test_dequant_readout_classes_and_two_roundings(q):
    caught = 0
    for raw in U.dequant_readout_problems(q):
        deq = weightonly.dequant(raw.qb, raw.sb, raw.N, raw.K, q.w_bits, q.gsize, q.sym)
        ref = _expected(raw)
        assert np.isfinite(deq).all()
        assert _same(ref, deq[:, raw.info["pi"]].T), "the readout is not the dequantised weights"
        assert _same(np_dequant(raw), deq)
        u = raw.qb + weightonly.sym_offset(q.w_bits, q.sym)
        assert u.min() == 0 and u.max() == (1 << q.w_bits) - 1 and len(np.unique(u)) == 1 << q.w_bits
        sz = raw.sb.reshape(-1) if q.sym else raw.sb.reshape(-1, 2)[:, 0]
        S, Z = U.wo_scale_zp_sets(q.w_bits)
        assert set(_bits(sz)) == set(_bits(S)) and _subnormal(sz).any() and (sz == U.p2(-14)).any()
        if not q.sym:
            pairs = {(a, b) for a, b in _bits(raw.sb.reshape(-1, 2))}
            assert len(pairs) == 25  # every scale with every zero point
            zp = raw.sb.reshape(-1, 2)[:, 1]
            assert _subnormal(zp).any() and (zp > 500).any() and (zp < 0).any() and (_bits(zp) == 0).any()
        assert _subnormal(deq).any() and np.abs(deq.astype(np.float64)).max() >= 64 * np.abs(raw.qb).max()  # the scale 64
        caught += not _same(np_dequant(raw, two_roundings=True), deq)
    # asym: off = 0; 2-bit sym: off * s = s is exact — there the two forms are one function
    assert caught == (len(U.dequant_readout_problems(q)) if q.sym and q.w_bits > 2 else 0)


@pytest.mark.parametrize("subnormal", [False, True])
def test_f16_readout_classes(subnormal):
    raw = U.gen_f16_readout(256, 264, seed=780, subnormal=subnormal)
    ref = _expected(raw)
    assert _same(ref, raw.B[:, raw.info["pi"]].T)  # the oracle keeps subnormals
    b = _bits(raw.B)
    exps = set(((b >> 10) & 31).ravel())
    assert set(range(1, 31)) <= exps and 31 not in exps and 0x7BFF in b and 0xFBFF in b
    assert (0 in exps) == subnormal
    assert _subnormal(ref)[raw.info["sub"]].all() and not _subnormal(ref)[~raw.info["sub"]].any()


# ------------------------------------------------------------------ (e) activation kernels
def _row_quant(x, tag):
    """(codes [R, W], scales [R] or [R, W/128]) of the oracle for an integer tag."""
    bits = 8 if tag == 1 else 4
    stored, s = moe_ref.quant_rows(x, tag)
    q = oracle.unpack_wxax(stored, bits, x.shape[1]).astype(np.int32)
    return q, (s.reshape(x.shape[1] // 128, x.shape[0]).T if tag == 3 else s)


@pytest.mark.parametrize("tag", [1, 2, 3])
def test_act_special_rows_classes(tag):
    W, qmax = 512, U.act_qmax(tag)
    rows = U.act_special_rows(W, tag)
    kind = {k: i for i, k in enumerate(U.ACT_KINDS)}
    q, s = _row_quant(rows, tag)
    s = s.reshape(len(rows), -1)  # [R, groups] (one group for the per-row tags)
    sx = np.repeat(s, W // s.shape[1], axis=1).astype(np.float64)
    ratio = rows.astype(np.float64) / sx
    one = _bits(np.float16(1))
    assert (_bits(s[kind["zero"]]) == one).all() and (q[kind["zero"]] == 0).all()
    assert (_bits(s[kind["tiny"]]) == one).all() and np.abs(rows[kind["tiny"]]).max() == U.p2(-24)
    assert (q[kind["tiny"]] == 0).all()
    assert (s[kind["subscale"]] == np.float16(3 * 2.0 ** -24)).all() and np.abs(q[kind["subscale"]]).max() == qmax
    assert np.abs(rows[kind["amax_max"]]).max() == 65504 and (rows[kind["amax_max"]] == -65504).any()
    t = ratio[kind["tie"]]
    ties = (np.floor(t) + 0.5 == t)
    k = np.floor(t[ties]).astype(int)
    assert (s[kind["tie"]] == 0.125).all() and set(k) == set(range(-qmax, qmax)), "ties for every k, even and odd"
    assert np.array_equal(q[kind["tie"]][ties], np.rint(t[ties]).astype(int))  # half to even
    z = rows[kind["tie"]]
    assert ((z == 0) & np.signbit(z)).any() and ((z == 0) & ~np.signbit(z)).any()
    assert (ratio[kind["clamp"]].astype(np.float16) > qmax).any() and np.abs(q[kind["clamp"]]).max() == qmax
    z = rows[kind["neg_zero"]]
    assert ((z == 0) & np.signbit(z)).any()
    nz = (rows[kind["one_nonzero"]] != 0)
    assert nz.sum() == 1 and nz[-1] and q[kind["one_nonzero"], -1] == qmax
    if tag == 3:
        assert (_bits(s[kind["zero_group"]][1]) == one) and (s[kind["zero_group"]][[0, 2, 3]] != 1).all()
        assert (_bits(s[kind["one_nonzero"]][:3]) == one).all()
    # the numpy restatement is the oracle; the wrong quantisers differ where they should
    for g in range(s.shape[1]):
        cols = slice(g * (W // s.shape[1]), (g + 1) * (W // s.shape[1]))
        qn, sn = np_quant_rows(rows[:, cols], qmax)
        assert np.array_equal(qn, q[:, cols]) and np.array_equal(_bits(sn), _bits(s[:, g]))
        qa, _ = np_quant_rows(rows[:, cols], qmax, half_away=True)
        assert not np.array_equal(qa[kind["tie"]], q[kind["tie"], cols])
        _, s0 = np_quant_rows(rows[:, cols], qmax, keep_zero_scale=True)
        assert s0[kind["zero"]] == 0 and s0[kind["tiny"]] == 0  # the oracle's are 1


def test_act_schedules_give_every_expert_every_kind():
    R = len(U.ACT_KINDS)
    W = 512
    seen = {e: set() for e in range(4)}
    for c in range(R):
        routed, shared = U.act_slot_call(W, W, 1, c)
        for e, seg in enumerate(U.act_segments(routed, None, U.ACT_IDS)):
            ref = U.act_special_rows(W, U.ACT_TAGS[e])
            seen[e] |= {i for row in seg for i in range(R) if _same(row, ref[i])}
        assert all(_same(shared[t], U.act_special_rows(W, 1)[(t + c) % R]) for t in range(5))
    assert all(v == set(range(R)) for v in seen.values()), seen
    seen = {e: set() for e in range(4)}
    for c in range(R):
        for parity in (0, 1):
            hidden, ids = U.act_hidden_call(W, c, parity)
            perm, counts = moe_ref.route(ids, 4)[1], moe_ref.route(ids, 4)[3]
            assert (counts > 0).all()
            for e, seg in enumerate(U.act_segments(hidden[perm], None, ids)):
                ref = U.act_special_rows(W, 1 if e < 2 else 2)  # built for this expert's qmax
                seen[e] |= {i for row in seg for i in range(R) if _same(row, ref[i])}
    assert all(v == set(range(R)) for v in seen.values()), seen


def test_act_launch_arithmetic_reaches_every_instantiation_and_branch():
    ntk, T = U.ACT_IDS.size, U.ACT_IDS.shape[0]
    # one launch of width W (quant_act: K = W; the slot modes: N = Ns = W): every MAXC
    plans = [U.act_launch_plan(ntk, T, W, W) for W in U.ACT_WIDTHS]
    assert all(len(p) == 1 and p[0][0] == "one_launch" for p in plans)
    assert {p[0][1] for p in plans} == set(U.ACT_MAXC)
    assert max(U.ACT_WIDTHS) == 16384  # the ABI's widest row
    b = U.ACT_BRANCH_WIDTHS
    assert [x[0] for x in U.act_launch_plan(ntk, T, *b["split_row"])] == ["split_row"]
    assert [x[0] for x in U.act_launch_plan(ntk, T, 256, 640)] == ["split_row"]  # last quarter empty
    assert (640 // 4 + 127) // 128 * 128 * 3 >= 640
    for name, wide in (("two_launch_wide_quarter", True), ("two_launch_narrow_shared", False)):
        N, Ns = b[name]
        assert [x[0] for x in U.act_launch_plan(ntk, T, N, Ns)] == ["two_launch"] * 2
        assert (Ns > N and (Ns // 4 + 127) // 128 * 128 > N) if wide else Ns < N


@pytest.mark.parametrize("Ws", [5632, 640])
def test_split_rows_classes_and_quarter0_amax(Ws):
    qw = (Ws // 4 + 127) // 128 * 128
    peaks = U.split_row_peaks(Ws)
    rows = U.gen_split_rows(Ws, seed=5)
    assert (np.abs(rows.astype(np.float32)).argmax(axis=1) == peaks).all()
    quarters = [p // qw for p in peaks]
    assert quarters[:-1] == list(range(len(peaks) - 1)) and peaks[-1] >= Ws - 128
    assert len(peaks) == (5 if Ws == 5632 else 4)  # Ws = 640: the fourth quarter is empty
    act = moe_ref.silu_mul(U.gen_split_rows(Ws, seed=5, silu=True))
    assert (np.abs(act.astype(np.float32)).argmax(axis=1) == peaks).all() and np.abs(act).max() > 49
    for qmax in (127, 7):
        q, s = np_quant_rows(rows, qmax)
        qo, so = oracle.quant_rtn_sym(rows, 8 if qmax == 127 else 4)
        assert np.array_equal(q, qo) and np.array_equal(_bits(s), _bits(so))
        q0, s0 = np_quant_rows(rows, qmax, amax_cols=qw)
        assert _bits(s0[0]) == _bits(s[0]) and (_bits(s0[1:]) != _bits(s[1:])).all()


def test_silu_inputs_classes():
    gu = U.gen_silu_inputs(15, 512, seed=3)
    g = gu[:, :512].astype(np.float32)
    assert {float(np.float16(v)) for v in U.SILU_G} <= set(np.unique(g[:, ::4]).tolist())
    act = moe_ref.silu_mul(gu)
    assert np.isfinite(act).all() and np.abs(act.astype(np.float32)).max() <= 80
    assert ((act == 0) & np.signbit(act)).any() and _subnormal(act).any()
    amax = np.abs(act.astype(np.float32)).reshape(15, 4, 128).max(axis=2)
    assert amax.min() > 1.0  # no group near the scale's 0 -> 1 switch
    il = U.interleave_gate_up_cols(gu)
    assert _same(il[:, 0:16], gu[:, 0:16]) and _same(il[:, 16:32], gu[:, 512:528]) and _same(il[:, 32:48], gu[:, 16:32])


@pytest.mark.parametrize("topk", U.COMBINE_TOPK)
@pytest.mark.parametrize("H", U.COMBINE_H)
def test_combine_inputs_keep_the_reference_exact(H, topk):
    d = U.gen_combine(3, topk, H, seed=H + topk)
    inv = moe_ref.route(d["ids"], 8)[2]
    assert (d["w"] == 0).any() and (d["w"] < 0).any() and (d["shared_w"] == 0).any() and (d["shared_w"] < 0).any()
    assert all(len(set(r)) == topk for r in d["ids"].tolist())
    for sh, sw in ((None, None), (d["shared"], None), (d["shared"], d["shared_w"])):
        out = moe_ref.combine(d["y"], inv, d["w"], topk, sh, sw)  # asserts its own exactness
        assert np.isfinite(out).all()
