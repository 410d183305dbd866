"""CPU proofs of what tests/test_f8g128_edges_gpu.py relies on (no GPU): the families of tests/_f8g128_edges.py keep
the per-group exactness bounds, cover the codes, byte positions and scale classes they claim, and expose wrong
arithmetic - every mutant of ``_f8g128_edges.mutant`` differs from the reference on the operands it is aimed at.

Which mutant is aimed at which family. C is fp16 (11 bits) and the fold rounds at 24, so on sums without cancellation
(F-a) another fold order, an unfused multiply-add or another rounding of the scale product moves an output only where
the f32 value sits within 2^-13 of an fp16 tie: F-a catches the mutants that take the wrong operand - one sum over
all of K, sb of the neighbouring block, sa of the neighbouring row - in nearly every output, and the rounding mutants
in almost none (measured: at most 1e-3 of the outputs). F-d is built for those: its partial sums stand 2^10 .. 2^20
above the result, and descending order, (acc sa) sb, the unfused form and the wrong split point of two K slices each
move 15 % or more of its outputs. The condition checked is the issue's: a mutant differs in at least one output of
every problem of a family it is aimed at (and on which it can differ at all, ``applies``), and in at least 1 % of
the family's outputs. The figure is a condition on the inputs, not a tolerance on any kernel."""
from __future__ import annotations

from fractions import Fraction

import numpy as np
import pytest
import torch

from mxmoe_amd.quantize import quant_e4m3_g128
from tests import _f8g128_edges as X
from tests import _f8g128_ref as ref

PATHS = ("v2x", "wo3")
FAMILIES = {"a": X.window_problems, "c": X.ladder_problems, "d": X.cancel_problems, "x": X.span_problems}
AIMED = {"a": ("one_sum", "sb_neighbour", "sa_neighbour"), "d": X.MUTANTS + ("floor_split",)}
_cache: dict = {}


def problems(fam: str, path: str):
    key = (fam, path)
    if key not in _cache:
        _cache[key] = X.readout_problems() if fam == "b" else FAMILIES[fam](path)
    return _cache[key]


def decode_probs(case, gate_up=False):
    """A decode case of the shared lists (_f8g128_edges.DOWN_CASES / GATE_UP_CASES / SPAN_CASE: exactly what the GPU
    file runs) as one Prob per expert, built once."""
    key = ("decode", case, gate_up)
    if key not in _cache:
        _cache[key] = X.decode_probs(case, gate_up)
    return _cache[key]


DECODE_ALL = [(c, False) for c in X.DOWN_CASES + [X.SPAN_CASE]] + [(c, True) for c in X.GATE_UP_CASES]


def test_fma32_is_one_rounding():
    """_f8g128_ref.fma32 against exact rational arithmetic: random operands, near-cancellation, and sums that a double
    rounding through f64 gets wrong (a product whose low bits sit just beyond f64's reach of the sum)."""
    rng = np.random.default_rng(0)
    a = X.full_f32(rng, 4000, -20, 20) * rng.choice([-1, 1], 4000).astype(np.float32)
    b = X.full_f32(rng, 4000, -20, 20)
    c = -(a.astype(np.float64) * b.astype(np.float64) * (1 + np.exp2(rng.uniform(-30, -2, 4000)))).astype(np.float32)
    c[::3] = X.full_f32(rng, len(c[::3]), -40, 40)
    # a tie at 24 bits in f64 that the exact sum is just above: c = 1, a b = 2^-24 + 2^-60-ish
    a[:4] = np.float32(2.0 ** -24) * np.float32(1 + 2.0 ** -23), np.float32(2.0 ** -24), np.float32(3 * 2.0 ** -25), np.float32(1 + 2.0 ** -23)
    b[:4] = np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -23), np.float32(1 + 2.0 ** -22), np.float32(1 + 2.0 ** -23)
    c[:4] = 1, 1, -1, np.float32(2.0 ** 30)
    got = ref.fma32(a, b, c)
    for x, y, z, r in zip(a.tolist(), b.tolist(), c.tolist(), got.tolist()):
        exact = Fraction(x) * Fraction(y) + Fraction(z)
        lo, hi = np.nextafter(np.float32(r), np.float32(-np.inf)), np.nextafter(np.float32(r), np.float32(np.inf))
        err = abs(Fraction(r) - exact)
        for other in (float(lo), float(hi)):
            assert err <= abs(Fraction(other) - exact), (x, y, z, r)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):  # a tie: the even one
            assert np.float32(r).view(np.uint32) & 1 == 0
    with np.errstate(all="ignore"):
        sp = ref.fma32(np.float32([0, 0, 1, np.inf, 3]), np.float32([np.inf, np.nan, np.nan, 1, 2.0 ** 127]), np.float32([1, 1, 1, 1, 2.0 ** 127]))
    assert np.isnan(sp[:3]).all() and sp[3] == np.inf and sp[4] == np.inf


def test_sliced_reference():
    """One slice is the contract; the slice bounds are the kernel's (ceil, the last what remains, none for one group)."""
    assert ref.slice_bounds(1, 2) == [(0, 1), (1, 1)] and ref.slice_bounds(5, 2) == [(0, 3), (3, 5)]
    assert ref.slice_bounds(9, 2) == [(0, 5), (5, 9)] and ref.slice_bounds(4, 2) == [(0, 2), (2, 4)]
    assert ref.slice_bounds(5, 2, lambda g, ks: g // ks) == [(0, 2), (2, 5)] and ref.slice_bounds(3, 1) == [(0, 3)]
    p = problems("d", "wo3")[0]
    assert np.array_equal(ref.gemm_fold_f32_sliced(*p.ops, 1).view(np.uint16), X.expected(p).view(np.uint16))
    assert X.mismatch(ref.gemm_fold_f32_sliced(*p.ops, 2), X.expected(p)).any()  # two slices: another answer


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fam", ["a", "b", "c", "d", "x"])
def test_bounds_and_exact_group_sums(fam, path):
    """The three bounds recomputed from the operands in f64 and compared with info; every acc_g equals its f32
    rounding (it would in any summation order: the bound). F-x keeps the sum bound (2^22) and breaks the span rule."""
    if fam == "b" and path == "wo3":
        return  # one problem list for both paths: checked under "v2x"
    for p in problems(fam, path):
        bound, span = X.bounds(p)
        assert (bound, span) == (p.info["bound"], p.info["span"])
        if fam == "x":
            assert bound < 2.0 ** 22 and 2.0 ** 20 < span < 2.0 ** 21
        elif p.info.get("one_product"):  # F-b: one nonzero product per (row, column, group), exact at any size
            hot = p.ops[0] if p.info["side"] == "B" else p.ops[2]
            assert bound < 2.0 ** 24 and ((hot != 0).sum(axis=1) == 1).all()
        else:
            assert bound < 2.0 ** 24 and span < X.SPAN, (fam, p.shape, bound, span)
        acc = X.group_accs(p)
        fin = np.isfinite(acc)
        assert (acc[fin].astype(np.float32).astype(np.float64) == acc[fin]).all()
        assert p.K % 128 == 0 and p.ops[1].shape == (p.M, p.K // 128) and p.ops[3].shape == ((p.N + 127) // 128, p.K // 128)
        X.scale_classes(p)  # (asserts: no f32-subnormal scale product)
        if fam in ("a", "d", "x"):
            assert np.isfinite(X.expected(p)).all()


@pytest.mark.parametrize("path", PATHS)
def test_window_family_covers_every_finite_code_and_rounds(path):
    finite = {c for c in range(256) if c & 0x7F != 0x7F}
    probs = problems("a", path)
    assert {int(c) for p in probs for c in np.unique(p.ops[0])} == finite
    assert {int(c) for p in probs for c in np.unique(p.ops[2])} == finite
    assert [p.shape for p in probs[:4]] == X.SHAPES[path]
    for p in probs:  # 24-bit scales: f32_rn(sa sb) rounds nearly everywhere, and each group / block step differs
        sa, sb = p.ops[1], p.ops[3]
        assert ((sa.view(np.uint32) & 1) == 1).all() and ((sb.view(np.uint32) & 1) == 1).all()
        prod = sa.astype(np.float64)[:, None, :] * sb.astype(np.float64)[None, :, :]
        assert (prod.astype(np.float32).astype(np.float64) != prod).mean() > 0.9
        assert len(np.unique(sa)) == sa.size and len(np.unique(sb)) == sb.size


def test_readout_places_every_code_at_every_byte_and_tells_swaps():
    for p in problems("b", "v2x"):
        side = p.info["side"]
        cyc = p.ops[2] if side == "B" else p.ops[0]
        hot = p.ops[0] if side == "B" else p.ops[2]
        assert p.shape == ((256, 264, 256) if side == "B" else (264, 256, 256))
        assert ((hot == X.ONE).sum(axis=1) == 1).all() and ((hot == 0) | (hot == X.ONE)).all()
        assert sorted(np.argmax(hot, axis=1).tolist()) == list(range(256))
        full = ((np.arange(256)[None, :] + np.arange(264)[:, None]) % 256).astype(np.uint8)  # before the NaN replacement
        for k in range(256):  # every code at byte k (of its group: k % 128 in group k / 128)
            assert len(set(full[:256, k].tolist())) == 256
        nan = (cyc & 0x7F) == 0x7F
        assert (nan.any(axis=1) == p.info["nan_rows"]).all() and ((cyc == full) | ((full & 0x7F) == 0x7F)).all()
        want = X.expected(p)
        poisoned = np.isnan(want).all(axis=0 if side == "B" else 1)
        assert (poisoned == p.info["nan_rows"][: len(poisoned)]).all() and np.isnan(want).sum() == poisoned.sum() * 256
        # swapping two byte positions (within a group, or across the groups: K = 256 is two groups) or the two groups
        # of the cycling side alone changes the expected output
        rng = np.random.default_rng(5)
        swaps = [(0, 1), (0, 127), (126, 127), (128, 255), (3, 131), (127, 128)] + \
                [tuple(rng.choice(256, 2, replace=False).tolist()) for _ in range(10)]
        for k1, k2 in swaps:
            c2 = cyc.copy()
            c2[:, [k1, k2]] = c2[:, [k2, k1]]
            ops = (p.ops[0], p.ops[1], c2, p.ops[3]) if side == "B" else (c2, p.ops[1], p.ops[2], p.ops[3])
            assert X.mismatch(ref.gemm_fold_f32(*ops), want).any(), (side, k1, k2)
        c2 = np.concatenate([cyc[:, 128:], cyc[:, :128]], axis=1)
        ops = (p.ops[0], p.ops[1], c2, p.ops[3]) if side == "B" else (c2, p.ops[1], p.ops[2], p.ops[3])
        assert X.mismatch(ref.gemm_fold_f32(*ops), want).mean() > 0.9
        for i in (1, 3):  # the scales tell the group and the block: swapping the groups' (blocks') scales shows
            s2 = p.ops[i][:, ::-1].copy()
            assert X.mismatch(ref.gemm_fold_f32(*p.ops[:i], s2, *p.ops[i + 1:]), want).mean() > 0.5
        s2 = p.ops[3][::-1].copy()
        assert X.mismatch(ref.gemm_fold_f32(*p.ops[:3], s2), want).mean() > 0.3


@pytest.mark.parametrize("path", PATHS)
def test_ladder_holds_every_scale_class(path):
    probs = problems("c", path)
    assert {p.info["kind"] for p in probs} == set(X.LADDER_KINDS)
    seen = set().union(*(X.scale_classes(p) for p in probs))
    assert {"sa_zero", "sa_negzero", "sb_zero", "sb_negzero", "sa_negative", "sb_negative", "nan_sa", "nan_sb", "inf_sb",
            "inf_sa"} <= seen
    partial = set()
    for p in probs:
        want, kind, M, N = X.expected(p), p.info["kind"], p.M, p.N
        sub = (np.abs(want.astype(np.float64)) < 2.0 ** -14) & (want != 0)
        if kind == "sub_exact":
            assert sub.sum() > 100
        elif kind == "sub_tie":  # exact f64 values halfway between two fp16 subnormals
            v = ref.gemm(*p.ops) * 2.0 ** 24
            assert ((np.abs(v) < 1024) & (v - np.floor(v) == 0.5)).sum() >= 20
        elif kind == "overflow":
            assert (want == np.inf).any() and (want == -np.inf).any() and np.isfinite(want).mean() > 0.5
        elif kind in ("nan_sa", "inf_sa"):
            rows = p.info["rows"]
            assert np.isnan(want[rows]).all() and not np.isnan(np.delete(want, rows, axis=0)).any()
            assert any(r // 16 == (M - 1) // 16 for r in rows) and (kind == "inf_sa" or (0 in rows and M - 1 in rows))
            for r in rows:  # exactly what the quantiser emits: zero codes under the non-finite scale
                g = int(np.flatnonzero(~np.isfinite(p.ops[1][r]))[0])
                assert (p.ops[0][r, g * 128:(g + 1) * 128] == 0).all()
        elif kind == "nan_inf_sb":
            assert N % 128 and (~np.isfinite(p.ops[3][-1])).any()  # the partial block is one of the two
            partial |= {c for c in p.info["classes"] if c.startswith("partial_block")}
            nb = int(np.flatnonzero(np.isnan(p.ops[3]).any(axis=1))[0])
            ib = int(np.flatnonzero(np.isinf(p.ops[3]).any(axis=1))[0])
            assert np.isnan(want[:, nb * 128:(nb + 1) * 128]).all() and not np.isfinite(want[:, ib * 128:(ib + 1) * 128]).any()
            mid = np.ones(N, bool)
            mid[nb * 128:(nb + 1) * 128] = mid[ib * 128:(ib + 1) * 128] = False
            assert np.isfinite(want[:, mid]).all()
        elif kind == "zero":
            assert (want[5] == 0).all() and (want != 0).mean() > 0.5
        else:
            assert (want < 0).any() and np.isfinite(want).all()
    assert partial == {"partial_block_nan", "partial_block_inf"}


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fam", ["a", "d"])
def test_mutants_differ(fam, path):
    """Every mutant aimed at the family differs from the reference in at least one output of every problem on which
    it can differ at all, and in at least 1 % of the family's outputs (module docstring)."""
    probs = problems(fam, path)
    for name in AIMED[fam]:
        diff = total = 0
        for p in probs:
            if not X.applies(name, p):
                continue
            want = ref.gemm_fold_f32_sliced(*p.ops, 2) if name == "floor_split" else X.expected(p)
            bad = int(X.mismatch(X.mutant(p, name), want).sum())
            assert bad > 0, (name, p.shape)
            diff, total = diff + bad, total + want.size
        assert total and diff >= 0.01 * total, (name, diff, total)


@pytest.mark.parametrize("case,gate_up", DECODE_ALL, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else ("gate_up" if v else "down"))
def test_decode_operands(case, gate_up):
    """Every decode case the GPU file runs, on exactly its operands: the bounds (F-x: the sum bound only), exact group
    sums, no f32-subnormal scale product, and the in-kernel quantisation known - _f8g128_ref.quant of the fp16 rows
    gives the generator's codes and scales."""
    kind = case[-1]
    for p in decode_probs(case, gate_up):
        assert X.bounds(p) == (p.info["bound"], p.info["span"])
        assert p.info["bound"] < (2.0 ** 22 if kind == "span" else 2.0 ** 24)
        assert (2.0 ** 20 < p.info["span"] < 2.0 ** 21) if kind == "span" else p.info["span"] < X.SPAN
        acc = X.group_accs(p)
        assert (acc.astype(np.float32).astype(np.float64) == acc).all()
        X.scale_classes(p)
        codes, sa = ref.quant(p.info["x"])
        assert (codes == p.ops[0]).all() and (sa == p.ops[1]).all()
        if kind == "cancel":  # sa is no power of two: (acc sa) sb is another computation
            assert (np.frexp(p.ops[1])[0] != 0.5).all()
        if kind in ("", "cancel", "span"):
            assert np.isfinite(ref.gemm_fold_f32_sliced(*p.ops, case[5])).all()


@pytest.mark.parametrize("case", [c for c in X.DOWN_CASES if c[-1] == "cancel"], ids=lambda c: "-".join(map(str, c)))
def test_mutants_differ_on_decode_cancel_cases(case):
    """The decode down cases with cancellation, on exactly the operands the GPU file runs: against the reference the
    GPU test uses (gemm_fold_f32_sliced at the case's ks), descending order, the unfused form and (acc sa) sb - each
    inside the kernel's slices - and with two slices also a single slice (ks = 1) and the floor split each move at
    least 1 % of the case's outputs. (The window cases of DOWN_CASES carry no such proof: without cancellation fp16
    hides these differences, as on F-a; they are there for the codes, the trips and the scale edges.)"""
    ks = case[5]
    names = ["descending", "unfused", "split_scale"] + (["floor_split", "one_slice"] if ks == 2 else [])
    moved, total = dict.fromkeys(names, 0), 0
    for p in decode_probs(case):
        want = ref.gemm_fold_f32_sliced(*p.ops, ks)
        total += want.size
        for name in names:
            got = ref.gemm_fold_f32(*p.ops) if name == "one_slice" else X.mutant(p, name, ks)
            moved[name] += int(X.mismatch(got, want).sum())
    assert all(m >= 0.01 * total for m in moved.values()), (moved, total)


@pytest.mark.parametrize("n,K", [(32, 384), (10, 384)])
def test_quantiser_rows(n, K):
    """F-q: quantize.quant_e4m3_g128 equals the search-based restatement on the rows; the specials stand at every group
    position (n = 32) and always in the last group; Inf / NaN groups give a NaN scale and zero codes."""
    x = X.quant_rows(n, K, 2500 + n)
    codes, sc = quant_e4m3_g128(torch.from_numpy(x))
    rcodes, rsc = ref.quant(x)
    assert (codes.numpy() == rcodes).all() and np.array_equal(sc.numpy(), rsc, equal_nan=True)
    sp = X.special_groups()
    Gk = K // 128
    for r in range(min(n, 6 * Gk)):
        g = Gk - 1 - r // 6
        assert np.array_equal(x[r, g * 128:(g + 1) * 128].view(np.uint16), sp[r % 6].view(np.uint16))
    assert {Gk - 1 - r // 6 for r in range(min(n, 6 * Gk))} >= ({0, 1, 2} if n == 32 else {Gk - 1})
    bad = ~np.isfinite(x.astype(np.float32)).reshape(n, Gk, 128).all(axis=2)
    assert bad.any() and (np.isnan(rsc) == bad).all() and (rcodes.reshape(n, Gk, 128)[bad] == 0).all()
    amax = np.abs(x.astype(np.float64)).reshape(n, Gk, 128).max(axis=2)
    frac = np.log2(amax[np.isfinite(amax) & (amax > 0)] / 448)
    assert (frac != np.rint(frac)).sum() >= n  # groups whose amax is not 448 * 2^e
    W, sb, pi = X.readout_weight(512, K, 7)
    assert sorted(pi.tolist()) == list(range(K)) and (W[K:] == 0).all() and (sb == 1).all()
