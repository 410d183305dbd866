"""GPU tests of the w8a8_g128_sym_E4M3 bodies on the edge-value families of tests/_f8g128_edges.py (proved on the CPU
by tests/test_f8g128_edges.py): gg_tile_f8g128 in the exact v2x build and in the widest fallback, gg_tile_f8g128s
forced onto wo3, a device-planned call, and decode_f8g_kernel through its down and gate_up entries.

Every comparison is bit for bit against tests/_f8g128_ref.py's restatement of the contract (gemm_fold_f32; the decode
kernel's two K slices: gemm_fold_f32_sliced), a zero's sign included, NaN by isnan. Each body meets the contract on
its own - the wo3-equals-v2x comparison stays in tests/test_f8g128_small_gpu.py. Tolerances appear in three places
and nowhere on a block-scaled output outside them: assert_f16_close on F-x (operands outside the exactness rule,
where no reference says what the bits should be), assert_act_close on gate_up (the gated activation has no bit-level
reference in this project: g and u come from the fold reference, rounded to fp16), and assert_f16_close on the fp16
companion problem of the fallback launch, which is not of this type (as tests/test_f8g128_gpu.py holds it)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W8A8, W8A8_G128_E4M3, DynamicGroupGemm, GroupGemm, Problem
from mxmoe_amd.quantize import pack_e4m3
from tests import _f8g128_edges as X
from tests import _f8g128_ref as ref
from tests import _fp8_bf16_edges as E
from tests._decode_util import assert_act_close
from tests._util import HostProblem, assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0x7B7B  # fp16 bit pattern of the sentinel around C
QG = W8A8_G128_E4M3
PATHS = ("auto", "wo3", "fallback")
FAMILIES = {"a": X.window_problems, "b": lambda path: X.readout_problems(), "c": X.ladder_problems, "d": X.cancel_problems}
_want: dict = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _wo3() -> int:
    return [ln.split()[1] for ln in nat.list_variants()].index("wo3_64x256_w8_3wg")


def _family(fam: str, shapes: str):
    """A family's problems and their expected outputs, computed once per module."""
    key = (fam, "v2x" if fam == "b" else shapes)
    if key not in _want:
        probs = FAMILIES[fam](shapes)
        _want[key] = (probs, [X.expected(p) for p in probs])
    return _want[key]


def _dev(t):
    return torch.from_numpy(np.ascontiguousarray(t)).to(DEV)


def _padded_c(rows: int, N: int):
    """C [rows + 3, ldc] filled with the sentinel, ldc = N rounded up to 8 plus 8 (rows stay 16-byte aligned)."""
    ldc = (N + 7) // 8 * 8 + 8
    full = torch.full((rows + 3, ldc), GUARD, dtype=torch.int16, device=DEV).view(torch.float16)
    return full, ldc


def _problem(p: X.Prob):
    a, sa, b, sb = p.ops
    full, ldc = _padded_c(p.M, p.N)
    return Problem(A=pack_e4m3(_dev(a)), B=pack_e4m3(_dev(b)), C=full[:p.M, :p.N], M=p.M, N=p.N, K=p.K, q=QG,
                   scale_a=_dev(sa.T), scale_b=_dev(sb.T), ldc=ldc), full  # scales group-major


def _assert_same(out, want, what):
    bad = X.mismatch(out, want)
    where = np.argwhere(bad)[:4].tolist()
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {where}: got "
                           f"{out[bad][:4]} (bits {[hex(b) for b in E.f16_bits(out[bad][:4])]}), expected {want[bad][:4]} "
                           f"(bits {[hex(b) for b in E.f16_bits(want[bad][:4])]})")


def _outputs(p: X.Prob, full: torch.Tensor, what) -> np.ndarray:
    """The problem's C out of its padded buffer; the sentinel columns and rows must be untouched."""
    c = full.cpu().numpy()
    bits = c.view(np.uint16)
    assert (bits[:, p.N:] == GUARD).all() and (bits[p.M:] == GUARD).all(), f"{what}: the sentinel around C was written"
    return np.ascontiguousarray(c[:p.M, :p.N])


def _launch(probs, path):
    """One GroupGemm call of all the problems on a path: AUTO at the exact v2x build, forced wo3, or the widest fallback
    (the type beside one small fp16 and one small w8a8 problem, each checked against its own reference)."""
    built = [_problem(p) for p in probs]
    ps = [b[0] for b in built]
    if path == "fallback":
        hps = [HostProblem(77, 128, 192, FP16, seed=1, device=DEV), HostProblem(513, 256, 128, W8A8, seed=2, device=DEV)]
        gg = GroupGemm(ps[:1] + [hps[0].problem] + ps[1:] + [hps[1].problem])
    else:
        gg = GroupGemm(ps, variant=_wo3() if path == "wo3" else None)
    if path == "wo3":
        assert gg.variant == _wo3()
    else:
        assert gg.variant == nat.default_variant()
    gg.launch()
    torch.cuda.synchronize()
    if path == "fallback":
        assert_f16_close(hps[0].result(), hps[0].expected(), 192)
        assert (hps[1].result().view(np.uint16) == hps[1].expected().view(np.uint16)).all()
    return [_outputs(p, full, (path, p.shape)) for p, (_, full) in zip(probs, built)]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_groupgemm_family(fam, path):
    """F-a (windows: every finite code, scales whose product and fold round), F-b (readout: every code at every byte
    position, per-group and per-block scales, NaN codes), F-c (the scale ladder: zero, negative, fp16-subnormal
    results and ties, overflow, NaN / Inf sa and sb) and F-d (cancellation across 9 groups) on each of the three code
    paths, one launch per family and path, bit for bit against the contract."""
    probs, wants = _family(fam, "wo3" if path == "wo3" else "v2x")
    for p, out, want in zip(probs, _launch(probs, path), wants):
        _assert_same(out, want, f"F-{fam} {path} {p.shape} {p.info.get('kind', '')}")


@pytest.mark.parametrize("path", ["v2x", "wo3"])
def test_device_planned_call(path):
    """F-a through the dynamic plan GraphForward uses: every problem planned at a capacity above its rows, the rows
    device-counted (the row table), so the group-major sa is strided by the launch's M, not the capacity."""
    probs, wants = _family("a", path)
    v = _wo3() if path == "wo3" else nat.default_variant()
    planned, fulls, table, extents = [], [], [], []
    for p in probs:
        a, sa, b, sb = p.ops
        cap, Gk = p.M + 40, p.K // 128
        A = torch.zeros(cap, p.K, dtype=torch.uint8, device=DEV)
        A[:p.M] = pack_e4m3(_dev(a))
        SA = torch.ones(Gk * cap, dtype=torch.float32, device=DEV)
        SA[:Gk * p.M] = _dev(sa.T).reshape(-1)  # [K/128][M]: the stride is the launch's row count
        full, ldc = _padded_c(cap, p.N)
        planned.append(Problem(A=A, B=pack_e4m3(_dev(b)), C=full[:cap, :p.N], M=cap, N=p.N, K=p.K, q=QG, scale_a=SA,
                               scale_b=_dev(sb.T), ldc=ldc))
        fulls.append(full)
        table.append((p.M, 0, 0, 0))
        extents.append((A.numel(), SA.numel() * 4, full.numel() * 2))
    dyn = DynamicGroupGemm(planned, joint=range(len(probs)), rows_total=sum(p.M for p in probs), variant=v, extents=extents)
    assert dyn.variant == v
    dyn.launch(DynamicGroupGemm.row_table(table, DEV))
    torch.cuda.synchronize()
    assert dyn.status() == 0
    for p, full, want in zip(probs, fulls, wants):
        _assert_same(_outputs(p, full, ("dynamic", p.shape)), want, f"F-a dynamic {path} {p.shape}")


# ------------------------------------------------------------------ the decode kernel
def _decode_layer(E_, T, topk, N, H, w1=None, w2=None):
    """A DecodeForwardF8g on a layer of the given gate_up [2N, H] / down [H, N] (codes, sb) pairs; a missing side is one
    zero weight shared by every expert."""
    def prep(ws, rows, k):
        if ws is None:
            z = moe.prepare_weight_e4m3_g128(torch.zeros(rows, k, dtype=torch.uint8, device=DEV),
                                             torch.ones((rows + 127) // 128, k // 128, device=DEV))
            return [z] * E_
        return [moe.prepare_weight_e4m3_g128(_dev(b), _dev(sb)) for b, sb in ws]
    ffn = moe.MoEFFN(prep(w1, 2 * N, H), prep(w2, H, N), [(QG, QG)] * E_, num_routed=E_)
    df = moe.DecodeForwardF8g(ffn, T, topk)
    for t in (df.act, df.y):
        t.view(torch.int16).fill_(GUARD)
    return df


def _ids(T, topk, E_):
    return (torch.arange(T * topk, dtype=torch.int32) % E_).view(T, topk).to(DEV)


def _run_down(df, E_, T, topk, N, H, x, ids):
    df.act.copy_(torch.from_numpy(x))
    p = lambda t: None if t is None else moe._ptr(t)  # noqa: E731
    nat.check(nat.symbol(df.ENTRIES[1])(T, topk, E_, 0, p(ids), p(df.experts), df.mask2, H, N, 0, p(df.act), None, p(df.y), None,
                                        p(df.dev_status), None))
    torch.cuda.synchronize()
    assert df.status() == 0
    return df.y.cpu().numpy()


def _per_expert(flat, fn):
    """fn(rows of expert e, e) -> [len(rows), C] stitched back into pair order."""
    out = None
    for e in sorted(set(flat)):
        ps = [p for p, x in enumerate(flat) if x == e]
        r = fn(ps, e)
        out = np.zeros((len(flat), r.shape[1]), r.dtype) if out is None else out
        out[ps] = r
    return out


@pytest.mark.parametrize("T", [16, 5])
def test_decode_quantiser_readout(T):
    """F-q through the down entry: fp16 rows with the special groups (zero with -0, a single 65504, code ties, fp16
    subnormals, Inf, NaN) at every group position and random groups whose amax is not 448 * 2^e; the weight a permuted
    identity of code 0x38 with sb = 1 (H = 512 >= N = 384), so y[p, h] = fp16_rn(f32(code[p, pi[h]]) * sa[p][group]) with
    the codes and scales of _f8g128_ref.quant, the independent restatement. A wrong code moves the value by at least
    2^-4 of itself and shows; an error in the LAST BITS of an f32 scale mostly does not survive the rounding to fp16,
    so this test does not claim the scale is held to bits. Rows with an Inf / NaN group come back all NaN, their
    neighbours finite. T = 16 gives 32 rows, T = 5 gives 10 (two or three per expert: lanes r16 >= nr read the head)."""
    E_, topk, N, H = 4, 2, 384, 512
    n = T * topk
    x = X.quant_rows(n, N, 2500 + n)
    W, sb, _ = X.readout_weight(H, N, 7)
    codes, sa = ref.quant(x)
    want = ref.gemm_fold_f32_sliced(codes, sa, W, sb, 2)  # ct = 32: two K slices (one nonzero product per output)
    assert not X.mismatch(want, ref.gemm_fold_f32(codes, sa, W, sb)).any()
    bad = ~np.isfinite(x.astype(np.float32)).all(axis=1)
    assert bad.any() and np.isnan(want[bad]).all() and np.isfinite(want[~bad]).all()
    df = _decode_layer(E_, T, topk, N, H, w2=[(W, sb)] * E_)
    y = _run_down(df, E_, T, topk, N, H, x, _ids(T, topk, E_))
    _assert_same(y, want, f"decode readout T={T}")


def _ident(case):
    return "-".join(map(str, case))


@pytest.mark.parametrize("case", X.DOWN_CASES, ids=_ident)
def test_decode_down_fold(case):
    """The down entry alone, bit for bit, on the cases of _f8g128_edges.DOWN_CASES (E, topk, T, K = N, C = H, ks, kind),
    whose operands tests/test_f8g128_edges.py proves case by case, at the smallest shapes that reach each tile width:
    K of 640 and 1152 on 32-column tiles (E = 4, H = 256: two K slices, the uneven splits 3 + 2 and 5 + 4, more than one
    trip) against gemm_fold_f32_sliced(ks = 2); E = 64 at H = 1024 (64-column tiles) and H = 2048 (128-column tiles,
    two column passes): one slice, against gemm_fold_f32. The act rows quantise in the kernel to known codes and
    scales.
      ""        window codes, power-of-two act scales, 24-bit block scales: every code path and trip count; without
                cancellation fp16 hides most f32 rounding differences, so these cases say little about the fold's order
      "scales"  the same with a NaN block scale (its 128 columns NaN for that expert's rows and no others) and a zero one
      "cancel"  F-d for the decode kernel (decode_cancel_operands): group pairs cancel to 2^-10 .. 2^-20 of a
                contribution and the act scales are no powers of two; on exactly these operands the CPU file shows that
                descending order, the unfused form, (acc sa) sb and, with two slices, one slice or the floor split
                each move at least 1 % of the outputs. These cases carry the fold and the two-slice order."""
    E_, topk, T, N, H, ks, kind = case
    x, a_codes, sa, ws, flat = X.decode_case(case)
    ids = _ids(T, topk, E_)
    assert ids.view(-1).tolist() == flat
    want = _per_expert(flat, lambda ps, e: ref.gemm_fold_f32_sliced(a_codes[ps], sa[ps], *ws[e], ks))
    if kind == "scales":
        nan_rows = [p for p, e in enumerate(flat) if e == 0]
        assert np.isnan(want[nan_rows][:, :128]).all() and np.isnan(want).sum() == len(nan_rows) * 128
    else:
        assert np.isfinite(want).all()
    df = _decode_layer(E_, T, topk, N, H, w2=ws)
    _assert_same(_run_down(df, E_, T, topk, N, H, x, ids), want, f"decode down {case}")


@pytest.mark.parametrize("case", X.GATE_UP_CASES, ids=_ident)
def test_decode_gate_up_fold(case):
    """The gate_up entry, called as the down entry is (df.ENTRIES[0]), on the down cases' shapes with K = H and the gate
    and up rows in one [2 N, H] weight (_f8g128_edges.GATE_UP_CASES: ct = 32 with K = 640 and 1152, ct = 64, ct = 128,
    and a zero block scale): g and u from the fold reference (sliced where ct = 32), rounded to fp16 as the kernel
    rounds them, then the gated activation within assert_act_close - it has no bit-level reference in this project.
    The operands are the down cases' generator at a smaller scale range (|g|, |u| < 64, asserted on the reference), so
    that silu(g) u stays inside fp16: assert_act_close takes finite rows only. For the same reason no NaN block scale
    is run here (it would make act NaN, and the checker's bound needs the row's rms); the NaN scale goes through the
    same fold code in the down case "scales"."""
    E_, topk, T, H, N, ks, kind = case
    x, a_codes, sa, ws, flat = X.decode_case(case, gate_up=True)
    ids = _ids(T, topk, E_)
    assert ids.view(-1).tolist() == flat
    tok = lambda ps: [p // topk for p in ps]  # noqa: E731
    gu = _per_expert(flat, lambda ps, e: ref.gemm_fold_f32_sliced(a_codes[tok(ps)], sa[tok(ps)], *ws[e], ks))
    assert np.abs(gu.astype(np.float64)).max() < 64 and np.abs(gu.astype(np.float64)).mean() > 0.05
    df = _decode_layer(E_, T, topk, N, H, w1=ws)
    h = torch.from_numpy(x).to(DEV)
    p = lambda t: None if t is None else moe._ptr(t)  # noqa: E731
    nat.check(nat.symbol(df.ENTRIES[0])(df._glu, moe._DT[torch.float16], p(h), T, topk, E_, 0, p(ids), p(df.experts), df.mask1,
                                        H, N, 0, df.layout, p(df.act), None, p(df.dev_status), None))
    torch.cuda.synchronize()
    assert df.status() == 0
    act = df.act.cpu().numpy()
    for r in range(len(gu)):
        assert_act_close(act[r:r + 1], gu[r:r + 1], None, "silu", {})


# ------------------------------------------------------------------ F-x: the 448 question
def test_span_question(capsys):
    """F-x (DESIGN.md §4 "Decode forward on MFMA", the open observation): a 448 code in every A group meets a weight
    code of 0.25 .. 3.75 beside products down to 2^-4 - exact in f32 in any order, but one product stands 2^20.7
    granules above the sum's granule. Held to the type's own tolerance (assert_f16_close against the f64 GEMM) on the
    three GroupGEMM paths and the decode down entry; nothing is asserted about bits. The test prints, per kernel, how
    many outputs differ in bits from gemm_fold_f32 and how many of those the GroupGEMM kernels share (the same
    operands run on all three); the counts stand in DESIGN.md beside the observation."""
    probs = X.span_problems("v2x")
    folds = [X.expected(p) for p in probs]
    exact = [ref.gemm(*p.ops) for p in probs]
    bad = {}
    for path in PATHS:
        outs = _launch(probs, path)
        for p, out, want in zip(probs, outs, exact):
            assert_f16_close(out, want, p.K)
        bad[path] = [X.mismatch(o, f) for o, f in zip(outs, folds)]
    total = sum(f.size for f in folds)
    counts = {path: sum(int(b.sum()) for b in bs) for path, bs in bad.items()}
    shared = sum(int((a & b & c).sum()) for a, b, c in zip(*bad.values()))
    union = sum(int((a | b | c).sum()) for a, b, c in zip(*bad.values()))
    # the decode down entry: the same construction as quantised act rows (the 448 is the group's amax)
    E_, topk, T, N, H, ks, _ = X.SPAN_CASE
    x, a_codes, sa, ws, flat = X.decode_case(X.SPAN_CASE)
    ids = _ids(T, topk, E_)
    want = _per_expert(flat, lambda ps, e: ref.gemm_fold_f32_sliced(a_codes[ps], sa[ps], *ws[e], ks))
    f64 = _per_expert(flat, lambda ps, e: ref.gemm(a_codes[ps], sa[ps], *ws[e]))
    y = _run_down(_decode_layer(E_, T, topk, N, H, w2=ws), E_, T, topk, N, H, x, ids)
    assert_f16_close(y, f64, N)
    with capsys.disabled():
        print(f"\nF-x: outputs differing in bits from the fold reference: GroupGEMM {counts} of {total} "
              f"(in all three: {shared}, in any: {union}); decode down {int(X.mismatch(y, want).sum())} of {want.size}")
