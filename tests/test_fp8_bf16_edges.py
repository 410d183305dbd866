"""What the E4M3 / bf16 edge-value inputs of tests/test_fp8_bf16_edges_gpu.py contain, proved on the CPU.

The GPU file compares the QT_F8 and QT_BF16 GroupGEMM bodies with the f64 oracle bit for bit on the
families of tests/_fp8_bf16_edges.py. Shown here, with the oracle alone:

  * exactness: every family's operands are multiples of its granules and sum |a b| / g < 2^24 for every
    (row, column) pair (recomputed from the operands), or a pair has a single nonzero product — so an
    f32 sum in any order equals the oracle's f64 sum and no tolerance is needed;
  * class coverage: all 254 finite E4M3 codes on both sides (E-a), every code at every byte position
    (E-b), each scale-product class (E-c), every bf16 exponent and each fp16_rn class (B-b), ...;
  * sensitivity: a deliberately wrong numpy restatement differs from the oracle on the family.

Wrong arithmetic                                     caught by
  scale product flushed to zero when subnormal        E-c ladder, E-b readouts at 2^-15 / 2^-16
  output conversion saturating instead of +-inf       E-c ladder, B-b unit / scaled, B-a integers
  output conversion truncating instead of nearest     B-b unit / tie / scaled, E-b readout at 2^-16
  a K-tail chunk that is not zero-filled              (GPU) E-a / B-a at 3 stages + 48 bytes: any stray
                                                      product moves an exact sum
"""
from __future__ import annotations

import numpy as np
import pytest

from mxmoe_amd import _native as nat
from mxmoe_amd.groupgemm import BF16, W8A8_E4M3
from oracle import oracle
from tests import _fp8_bf16_edges as E
from tests._util import HostProblem, raw_scale_product

def _expected(raw):
    return HostProblem.from_raw(raw, None).expected()


def _same(a, b):
    return not E.mismatch(np.asarray(a), np.asarray(b)).any()


def _sub16(x):
    b = E.f16_bits(x) & 0x7FFF
    return (b > 0) & (b < 0x0400)


def _tie16(ex, r16):
    """exact f64 values lying exactly halfway between two fp16 neighbours (r16 = their rounding)."""
    r = r16.astype(np.float64)
    with np.errstate(invalid="ignore"):
        other = np.nextafter(r16, np.where(ex > r, np.float16(np.inf), np.float16(-np.inf)).astype(np.float16))
        return (ex != r) & np.isfinite(r) & np.isfinite(other) & (np.abs(ex - r) == np.abs(other.astype(np.float64) - ex))


def _assert_exact(raw):
    bound = E.exact_bound(raw)
    assert bound == raw.info["bound"] and bound < 2 ** 24, (raw.M, raw.N, raw.K, bound)


# ------------------------------------------------------------------ the code table and conversions
def test_e4m3_table_is_the_oracles():
    lut = oracle.e4m3_to_f32(np.arange(256)).astype(np.float64)
    assert np.array_equal(np.isnan(lut), np.isnan(E.E4M3)) and np.isnan(E.E4M3).sum() == 2
    fin = ~np.isnan(lut)
    assert np.array_equal(lut[fin], E.E4M3[fin]) and np.array_equal(np.signbit(lut)[fin], np.signbit(E.E4M3)[fin])
    assert np.abs(E.E4M3[fin]).max() == 448 and (E.E4M3[fin] * 512 == np.rint(E.E4M3[fin] * 512)).all()
    assert np.array_equal(E.E4M3[fin].astype(np.float16).astype(np.float64), E.E4M3[fin])  # every value an fp16 value
    assert E.E4M3[0x38] == 1.0


def test_to_f16_modes():
    x = np.array([65519.0, 65520.0, -70000.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1 + 2.0 ** -10 + 2.0 ** -12),
                  2.0 ** -25, -1.75 * 2.0 ** -24, np.inf, 3.0])
    rn, sat, tr = E.to_f16(x), E.to_f16(x, "sat"), E.to_f16(x, "trunc")
    assert rn.tolist() == [65504.0, np.inf, -np.inf, 1.0, 1.0 + 2.0 ** -9, -(1 + 2.0 ** -10), 0.0, -2.0 ** -23, np.inf, 3.0]
    assert sat.tolist() == [65504.0, 65504.0, -65504.0] + rn.tolist()[3:]
    assert tr.tolist() == [65504.0, 65504.0, -65504.0, 1.0, 1.0 + 2.0 ** -10, -(1 + 2.0 ** -10), 0.0, -2.0 ** -24, np.inf, 3.0]


# ------------------------------------------------------------------ E-a: every code in exact windows
def test_ea_every_finite_code_on_both_sides_and_exact():
    raws = E.e4m3_window_problems()
    assert len(raws) == len(E.EA_WINDOWS) * 2 and {(r.M, r.N, r.K) for r in raws} == set(E.EA_SHAPES)
    finite = set(range(256)) - set(E.E4M3_NAN)
    seen_a, seen_b = set(), set()
    for raw in raws:
        _assert_exact(raw)
        ca, cb = set(np.unique(raw.A).tolist()), set(np.unique(raw.B).tolist())
        assert ca == set(E.window_codes(*raw.info["wa"]).tolist()) and cb == set(E.window_codes(*raw.info["wb"]).tolist())
        seen_a |= ca
        seen_b |= cb
        # the scales are powers of two (1 unless the sums would leave fp16), so the rescaling is exact
        ex, s16 = raw_scale_product(raw)
        assert (ex == s16.astype(np.float64)).all() and len(np.unique(s16)) == 1 and np.log2(float(s16[0, 0])) % 1 == 0
        ref = _expected(raw)
        assert np.isfinite(ref).all() and (ref != 0).any()
        assert _same(E.np_gg_e4m3(raw), ref)
    assert len(finite) == 254 and 0x00 in finite and 0x80 in finite
    assert seen_a == finite and seen_b == finite, "a finite E4M3 code is missing on a side"
    scaled = [r for r in raws if r.sa[0] != 1 or r.sb[0] != 1]
    assert scaled and all(r.info["wa"] == E.W_TOP and r.info["wb"] == E.W_TOP for r in scaled)  # unit scales elsewhere
    # the windows' own bound: spans sA + sB <= 7 at K <= 432
    for wa, wb in E.EA_WINDOWS:
        assert (wa[1] - max(wa[0], 1)) + (wb[1] - max(wb[0], 1)) <= 7 and 432 * 225 * 2 ** 7 < 2 ** 24


def test_ed_split_k_data_is_exact_at_k_8192():
    for raw in E.e4m3_splitk_problems():
        assert raw.K == 8192 and raw.N == 256 and raw.M in (256, 96)
        _assert_exact(raw)
        assert (raw.sa == 1).all() and (raw.sb == 1).all()
        ref = _expected(raw)
        assert np.isfinite(ref).all() and _same(E.np_gg_e4m3(raw), ref)


# ------------------------------------------------------------------ E-b: readout of every byte position
@pytest.mark.parametrize("i", range(5))
def test_eb_readout_classes(i):
    raw = E.e4m3_readout_problems()[i]
    side, src, nan_rows = raw.info["side"], raw.info["src"], raw.info["nan_rows"]
    cyc, hot = (raw.B, raw.A) if side == "B" else (raw.A, raw.B)
    assert ((hot != 0).sum(axis=1) == 1).all() and set(np.unique(hot).tolist()) == {0, 0x38}
    # every code at every byte position of a 16-B chunk and in every chunk of both 128-B stages
    for c in range(256):
        rows, ks = np.nonzero(cyc == c)
        if c in E.E4M3_NAN:
            assert nan_rows[rows].all() and len(set((ks % 16).tolist())) == 16
        elif (c & 0x7F) != 0x7E:  # (+-448 also stands in for the NaN codes)
            assert len(set(ks.tolist())) == 256  # (so all 16 bytes of all 8 chunks of both stages)
    ref = _expected(raw)
    # a NaN code poisons exactly the outputs whose dot product contains it: its row of the cycling operand
    want_nan = np.zeros((raw.M, raw.N), bool)
    if side == "B":
        want_nan[:, nan_rows] = True
    else:
        want_nan[nan_rows, :] = True
    assert np.array_equal(np.isnan(ref), want_nan) and want_nan.any() and not want_nan.all()
    # elsewhere the output is the value read, times the power-of-two scale, rounded once; -0 reads as +0
    val = E.E4M3[src] * raw.info["scale"]
    want = np.where(val == 0, 0.0, val).astype(np.float16)
    ok = ~want_nan
    assert np.array_equal(E.f16_bits(ref)[ok], E.f16_bits(want)[ok])
    assert _same(E.np_gg_e4m3(raw), ref)
    assert set(np.unique(src[ok]).tolist()) >= set(range(256)) - set(E.E4M3_NAN)  # every finite code is read back
    if raw.info["scale"] == 1:
        assert np.array_equal(want[ok].astype(np.float64), np.where(val == 0, 0.0, val)[ok])  # exactly the value
    else:
        ex, s16 = raw_scale_product(raw)
        assert _sub16(s16).all() and (ex == s16.astype(np.float64)).all()  # the product itself is a subnormal fp16
        assert _sub16(ref[ok]).any()
        assert not _same(E.np_gg_e4m3(raw, flush=True), ref)
        ties = _tie16(val, want) & ok
        if raw.info["scale"] == 2.0 ** -16:
            assert (ties & _sub16(want)).any() and (ties & (want == 0)).any(), "no tie on the subnormal grid"
            assert not _same(E.np_gg_e4m3(raw, mode="trunc"), ref)
        else:
            assert not ties.any()  # m 2^-24: on the grid


# ------------------------------------------------------------------ E-c: scale ladder
def test_ec_ladder_classes_and_wrong_arithmetic():
    raws = E.e4m3_ladder_problems()
    assert [(r.M, r.N, r.K) for r in raws] == [(37, 136, 256), (130, 264, 512)]
    for raw in raws:
        _assert_exact(raw)
        ex, s16 = raw_scale_product(raw)
        a, b = E.operand_values(raw)
        acc = a @ b.T
        ref = _expected(raw)
        assert np.isfinite(s16).all() and not np.isnan(ref).any()
        normal = (E.f16_bits(s16) & 0x7FFF) >= 0x0400
        assert (normal & (ex == s16.astype(np.float64))).any() and (normal & (ex != s16.astype(np.float64))).any()
        assert (_tie16(ex, s16) & normal).any(), "no rounding tie among normal products"
        assert (_tie16(ex, s16) & _sub16(s16)).any(), "no tie among subnormal products"
        assert _sub16(s16).any() and ((s16 == 0) & (ex > 0)).any()
        assert (ref == np.inf).any() and (ref == -np.inf).any() and _sub16(ref).any()
        assert ((acc == 0) & (s16 != 0)).any() and (E.f16_bits(ref)[acc == 0] == 0).all()  # +0, not -0
        zero_rows = (raw.A == 0x00).all(axis=1)
        negz_rows = (raw.A == 0x80).all(axis=1)
        one_rows = ((raw.A & 0x7F) != 0).sum(axis=1) == 1
        for rows in (zero_rows, negz_rows, one_rows):  # each with every LADDER_A scale
            assert len(set((np.nonzero(rows)[0] % 6).tolist())) >= (6 if raw.M >= 60 else 3)
        assert zero_rows.any() and negz_rows.any() and one_rows.any()
        assert (E.f16_bits(ref)[negz_rows] == 0).all() and (ref[one_rows] != 0).any()
        assert _same(E.np_gg_e4m3(raw), ref)
        assert not _same(E.np_gg_e4m3(raw, flush=True), ref), "a flushed subnormal scale product goes unnoticed"
        assert not _same(E.np_gg_e4m3(raw, mode="sat"), ref), "a saturating output conversion goes unnoticed"


# ------------------------------------------------------------------ B-a: exact bf16 sums
def test_ba_exact_sums():
    raws = E.bf16_exact_problems()
    assert {r.M for r in raws} == {300, 130, 17} and {r.K for r in raws} == {256, 216} and {r.N for r in raws} == {264}
    for kind in ("eighths", "ints"):
        assert {r.M for r in raws if r.info["kind"] == kind} == {300, 130, 17}
    for raw in raws + E.bf16_splitk_problems():
        _assert_exact(raw)
        a, b = E.operand_values(raw)
        top = 8 if raw.info["kind"] == "eighths" else 128
        assert np.abs(a).max() == top and np.abs(b).max() == top and (a[0, :2] * b[0, :2]).tolist() == [top * top, -top * top]
        assert raw.A[0, 2] == 0x8000  # a -0 operand
        ref = _expected(raw)
        assert not np.isnan(ref).any() and _same(E.np_gg_bf16(raw), ref)
        if raw.info["kind"] == "ints":  # sums beyond 65504: the overflowing conversion is exercised
            assert np.isinf(ref).any() and np.isfinite(ref).any() and not _same(E.np_gg_bf16(raw, "sat"), ref)
        else:
            assert np.isfinite(ref).all()
            assert not _same(E.np_gg_bf16(raw, "trunc"), ref)  # sums with more than 11 significant bits
    assert [(r.M, r.N, r.K) for r in E.bf16_splitk_problems()] == [(256, 256, 4096), (96, 256, 4096)]


# ------------------------------------------------------------------ B-b: readout of B and of A
def _readout_expected(raw):
    """fp16_rn(h * p) from the patterns alone (one product per output, exact in f64)."""
    return E.bf16_f64(raw.info["hot"]) * E.bf16_f64(raw.info["src"])


@pytest.mark.parametrize("side", [0, 1], ids=["B", "A"])
@pytest.mark.parametrize("kind", E.BF16_KINDS)
def test_bb_readout_classes(kind, side):
    raw = E.bf16_readout_problems(kind)[side]
    assert raw.info["side"] == "BA"[side] and (raw.M, raw.N, raw.K) == (256, 264, 256)
    pat, hot = (raw.B, raw.A) if side == 0 else (raw.A, raw.B)
    assert ((hot != 0).sum(axis=1) == 1).all()
    field = (pat >> 7) & 0xFF
    assert 255 not in field  # finite patterns only
    ex = _readout_expected(raw)
    f32 = ex.astype(np.float32)
    assert (f32.astype(np.float64) == ex).all()  # the one product is an f32 value ...
    assert ((np.abs(f32) >= 2.0 ** -126) | (f32 == 0)).all()  # ... and a normal one
    want = E.to_f16(ex)
    ref = _expected(raw)
    assert np.array_equal(E.f16_bits(ref), E.f16_bits(want)) and _same(E.np_gg_bf16(raw), ref)
    ties = _tie16(ex, want)
    sub = raw.info["sub"]
    if kind == "unit":
        assert set(range(1, 255)) == set(np.unique(field).tolist())
        assert set(E.UNIT_PLANTED) <= set(pat[1].tolist()) and ((pat >> 15) == 1).any() and ((pat >> 15) == 0).any()
        assert (ex == 65280).any() and (want[ex == 65536] == np.inf).all() and (want[ex == -65536] == -np.inf).all()
        assert (ex == 65536).any() and (ex == -65536).any()
        assert not (ties & ~_sub16(want) & (want != 0)).any()  # 8 significant bits: no tie on fp16's normal grid
    if kind in ("unit", "scaled"):
        assert (ties & _sub16(want)).any() and (ties & (want == 0)).any(), "no tie on the subnormal grid"
        assert (want == np.inf).any() and (want == -np.inf).any(), "no overflow"
        assert ((want == 0) & (ex > 0)).any() and ((want == 0) & (ex < 0) & np.signbit(want)).any(), "no underflow to +-0"
        assert not _same(E.np_gg_bf16(raw, "sat"), ref)
    if kind == "tie":
        assert np.isfinite(want).all() and not _sub16(want).any()
        assert ties.any() and (E.f16_bits(want)[ties] & 1 == 0).all(), "no tie on the normal grid"
        up = ties & (np.abs(want.astype(np.float64)) > np.abs(ex))
        assert up.any() and (ties & ~up).any()  # ties that round up and ties that round down
    if kind == "scaled":
        assert set(np.unique(field).tolist()) == set(E.SCALED_FIELDS)
        far = (field < 127 - 30) | (field > 127 + 20)
        assert far.mean() > 0.7 and np.isfinite(want).any() and (~_sub16(want) & (want != 0) & np.isfinite(want)).any()
        assert (ex == 65280).any() or (ex == -65280).any()
    if kind != "subnormal":
        assert 0 not in field and not sub.any()
        assert not _same(E.np_gg_bf16(raw, "trunc"), ref), "a truncating conversion goes unnoticed"
    else:
        src = raw.info["src"]
        assert (((src >> 7) & 0xFF)[sub] == 0).all() and ((src & 0x7F)[sub] != 0).all() and (((src >> 7) & 0xFF)[~sub] != 0).all()
        assert sub.mean() == 0.5 and {1, 127} <= set((src & 0x7F)[sub].tolist())
        assert ((src >> 15)[sub] == 1).any() and ((src >> 15)[sub] == 0).any()
        assert (np.abs(want[sub]) >= 2.0 ** -6).all() and (want.astype(np.float64) == ex).all()  # kept by the oracle, exactly


# ------------------------------------------------------------------ B-c: non-finite operands
def test_bc_nonfinite_classes():
    raws = E.bf16_nonfinite_problems()
    assert [r.info["kind"] for r in raws] == ["inf", "inf_flipped", "overflow"]
    for raw in raws:
        a, b = E.operand_values(raw)
        ref = _expected(raw)
        rows, cols = raw.info["rows"], raw.info["cols"]
        hit = np.zeros((raw.M, raw.N), bool)
        hit[rows, :] = True
        hit[:, cols] = True
        # outside the affected rows and columns: finite operands, exact sums
        fa, fb = np.delete(a, rows, axis=0), np.delete(b, cols, axis=0)
        assert np.isfinite(fa).all() and np.isfinite(fb).all() and np.abs(fa).max() <= 8 and np.abs(fb).max() <= 8
        assert (fa * 8 == np.rint(fa * 8)).all() and (fb * 8 == np.rint(fb * 8)).all() and raw.K * 64 * 64 < 2 ** 24
        assert np.isfinite(ref[~hit]).all()
        assert np.array_equal(E.f16_bits(ref[~hit]), E.f16_bits((fa @ fb.T).astype(np.float32).astype(np.float16)).ravel())
        with np.errstate(invalid="ignore", over="ignore"):
            prod = a[:, None, :] * b[None, :, :]  # [M, N, K] in f64
        if raw.info["kind"] == "overflow":
            assert np.isfinite(a).all() and np.isfinite(b).all() and (np.abs(prod) > 3.5e38).sum() == 1
            r, c = rows[0], cols[0]
            assert ref[r, c] == np.inf and not np.isnan(ref).any()
            assert np.isinf(ref[r]).sum() > 100 and np.isinf(ref[:, c]).sum() > 100
            continue
        assert np.isinf(a).sum() == 1 and np.isinf(b).sum() == 1 and np.isnan(a).sum() == 1 and np.isnan(b).sum() == 1
        assert np.sign(a[np.isinf(a)][0]) == -np.sign(b[np.isinf(b)][0])
        # no 0 x inf, and no pair sums infinities of opposite sign
        assert not (np.isnan(prod) & ~np.isnan(a)[:, None, :] & ~np.isnan(b)[None, :, :]).any()
        assert not ((prod == np.inf).any(axis=2) & (prod == -np.inf).any(axis=2)).any()
        r1, r2 = rows
        c1, c2 = cols
        want_nan = np.zeros_like(hit)
        want_nan[r2, :] = True
        want_nan[:, c2] = True
        assert np.array_equal(np.isnan(ref), want_nan)
        assert np.isinf(ref[r1][~want_nan[r1]]).all() and np.isinf(ref[:, c1][~want_nan[:, c1]]).all()
        assert (ref[r1] == np.inf).any() and (ref[r1] == -np.inf).any() and (ref[:, c1] == np.inf).any() and (ref[:, c1] == -np.inf).any()
    ks = [int(np.nonzero(np.isinf(E.bf16_f64(r.A)))[1][0]) for r in raws[:2]]
    assert ks[0] < 192 <= ks[1]  # one inside a full stage, one inside the K tail (3 stages = 192 elements)


# ------------------------------------------------------------------ host validation
@pytest.mark.parametrize("q", [W8A8_E4M3, BF16], ids=["e4m3", "bf16"])
def test_silu_epilogue_is_rejected_and_names_the_problem(q):
    def cp(silu):
        return nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=64, N=512, K=256, a_bits=q.a_bits, w_bits=q.w_bits,
                              gsize=q.gsize, sym=int(q.sym), fmt=q.fmt_code | (nat.EPI_SILU_MUL if silu else 0), lda=0,
                              ldb=0, ldc=0)

    for v in nat.production_variants(q.qcfg) + [nat.VARIANT_AUTO]:
        ok = (nat.GGProblemC * 2)(cp(False), cp(False))
        assert nat.workspace_size(ok, 2, v) > 0
        bad = (nat.GGProblemC * 2)(cp(False), cp(True))
        with pytest.raises(nat.GGError, match=r"problem 1: the SiLU epilogue needs"):
            nat.workspace_size(bad, 2, v)
