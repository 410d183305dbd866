"""The w8a8_g-1_sym_E4M3 (QT_F8) and bf16 (QT_BF16) GroupGEMM bodies against the f64 oracle on edge
operand VALUES, bit for bit (tests/test_fp8_bf16_gpu.py covers the shape edges on uniform data within
the fp16 tolerance).

Inputs come from tests/_fp8_bf16_edges.py; tests/test_fp8_bf16_edges.py proves on the CPU that every
family's f32 sums are exact in any order (so no tolerance is needed), which value classes it contains
and which wrong arithmetic it exposes. NaN outputs compare by isnan, everything else by its bits. Every
test runs on every production variant with a body for the type, and on AUTO.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd.groupgemm import BF16, W4A4, W8A8, W8A8_E4M3, GroupGemm
from tests import _fp8_bf16_edges as E
from tests import _util as U
from tests._util import HostProblem

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x7B7B  # fp16 bit pattern of the guard elements


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _variants(*qcfgs) -> list:
    """Every production variant with a tile body for each of qcfgs, plus AUTO (None)."""
    return [v for v in nat.production_variants() if all(nat.variant_supports(v, q) for q in qcfgs)] + [None]


def _vid(v):
    return "auto" if v is None else nat.list_variants()[v].split()[1]


F8V, BFV = _variants(W8A8_E4M3.qcfg), _variants(BF16.qcfg)
BOTH = _variants(W8A8_E4M3.qcfg, BF16.qcfg)
EVERY = _variants(W8A8_E4M3.qcfg, BF16.qcfg, W8A8.qcfg, W4A4.qcfg, "fp16")

_REFS: dict = {}


def _problems(key, make):
    """(raws, oracle outputs) of one problem list, computed once and shared by the variants."""
    if key not in _REFS:
        raws = make()
        refs = [HostProblem.from_raw(r, None).expected() for r in raws]
        for ref in refs:
            ref.setflags(write=False)
        _REFS[key] = (raws, refs)
    return _REFS[key]


def _assert_same(out, ref, what):
    bad = E.mismatch(out, ref)
    where = np.argwhere(bad)[:4].tolist()
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} outputs differ, first at {where}: got "
                           f"{out[bad][:4]} (bits {[hex(b) for b in E.f16_bits(out[bad][:4])]}), expected {ref[bad][:4]} "
                           f"(bits {[hex(b) for b in E.f16_bits(ref[bad][:4])]})")


def _what(h, extra=""):
    return f"{h.q.qcfg} M={h.M} N={h.N} K={h.K}{extra}"


def _run_exact(raws, refs, variant, launches=1, want_splitk=False):
    hps = [HostProblem.from_raw(r, DEV) for r in raws]
    gg = GroupGemm([h.problem for h in hps], variant=variant)
    if want_splitk:
        assert gg.info.splitk_slabs > 0, "expected a split-K plan"
    for it in range(launches):
        for h in hps:
            h.problem.C.fill_(float("nan"))
        gg.launch()
        torch.cuda.synchronize()
        for h, ref in zip(hps, refs):
            _assert_same(h.result(), ref, _what(h, f" launch {it}"))
    return hps


# ------------------------------------------------------------------ E4M3
@pytest.mark.parametrize("variant", F8V, ids=_vid)
def test_e4m3_every_code_in_exact_windows(variant):
    """E-a: all 254 finite codes on both sides, in windows whose sums are exact: subnormal x subnormal,
    top x top (power-of-two scales), subnormal x top and the swap, the middle exponents; a 256-row tile
    with tails and a K tail inside a 128-B stage."""
    _run_exact(*_problems("ea", E.e4m3_window_problems), variant)


@pytest.mark.parametrize("variant", F8V, ids=_vid)
def test_e4m3_readout_of_every_byte_position(variant):
    """E-b: a permuted identity of code 0x38 reads every code back from every byte position of B, and
    of A; NaN codes poison exactly their dot products; at sa sb = 2^-15 / 2^-16 the values land on fp16's
    subnormal grid (exactly / with ties) through a subnormal scale product."""
    _run_exact(*_problems("eb", E.e4m3_readout_problems), variant)


@pytest.mark.parametrize("variant", F8V, ids=_vid)
def test_e4m3_scale_ladder(variant):
    """E-c: scale products that are ordinary, rounding ties, subnormal, zero by underflow, or large
    enough that the output overflows to +-inf; rows of 0, of -0 and of one nonzero code."""
    _run_exact(*_problems("ec", E.e4m3_ladder_problems), variant)


@pytest.mark.parametrize("variant", F8V, ids=_vid)
def test_e4m3_split_k_exact(variant):
    """E-d: the split-K shapes of test_low_fill_split_k on exact data (f32 slabs summed in slice order:
    exact in any order), launched twice."""
    _run_exact(*_problems("ed", E.e4m3_splitk_problems), variant, launches=2, want_splitk=True)


# ------------------------------------------------------------------ bf16
@pytest.mark.parametrize("variant", BFV, ids=_vid)
def test_bf16_exact_sums(variant):
    """B-a: multiples of 1/8 up to 8 and integers up to 128 (sums beyond 65504 overflow to +-inf) over
    the 256-, 128- and 64-row classes, K = 256 and 216 (3 stages + 48 bytes)."""
    _run_exact(*_problems("ba", E.bf16_exact_problems), variant)


@pytest.mark.parametrize("variant", BFV, ids=_vid)
def test_bf16_split_k_exact(variant):
    """B-a through split-K (K = 4096), launched twice."""
    _run_exact(*_problems("ba_splitk", E.bf16_splitk_problems), variant, launches=2, want_splitk=True)


@pytest.mark.parametrize("variant", BFV, ids=_vid)
@pytest.mark.parametrize("kind", E.BF16_KINDS[:3])
def test_bf16_readout(kind, variant):
    """B-b: fp16_rn of bf16 patterns of every exponent read back through a one-hot 1.0 (ties on the
    subnormal grid, the 65280 / 65536 boundary, overflow, underflow), through 1 + 2^-7 (ties on the
    normal grid) and through 2^s (values far outside fp16's range brought back into it), for B and A."""
    _run_exact(*_problems(("bb", kind), lambda: E.bf16_readout_problems(kind)), variant)


@pytest.mark.parametrize("variant", BFV, ids=_vid)
def test_bf16_readout_subnormal_inputs(variant):
    """B-b, f32-subnormal bf16 inputs (exponent field 0) times 2^127, beside normal ones, in B and in A.
    The oracle keeps them, and so does the hardware: measured on an MI355X (DESIGN.md §4 "fp8 E4M3 and
    bf16"), v_mfma_f32_16x16x32_bf16 kept 33792 of 33792 subnormal B inputs and 33792 of 33792 subnormal A
    inputs, both signs, on the v2x variant and on AUTO, and flushed none. The rule asserted is that one:
    every subnormal input is read back exactly (a flush to signed zero fails), and so is every normal one."""
    raws, refs = _problems(("bb", "subnormal"), lambda: E.bf16_readout_problems("subnormal"))
    hps = [HostProblem.from_raw(r, DEV) for r in raws]
    GroupGemm([h.problem for h in hps], variant=variant).launch()
    torch.cuda.synchronize()
    for h, raw, ref in zip(hps, raws, refs):
        out, sub = h.result(), raw.info["sub"]
        kept = E.f16_bits(out) == E.f16_bits(ref)
        flushed = sub & (out == 0) & (np.signbit(out) == np.signbit(ref))
        neg = np.signbit(ref)
        print(f"bf16 readout, subnormal {raw.info['side']} inputs: {int(kept[sub].sum())} kept, "
              f"{int((flushed & ~kept).sum())} flushed to signed zero, of {int(sub.sum())} "
              f"({int(kept[sub & neg].sum())} / {int((flushed & ~kept & neg).sum())} of the {int((sub & neg).sum())} negative ones)")
        assert kept[~sub].all(), f"side {raw.info['side']}: a normal value beside subnormal ones was not read back"
        assert kept[sub].all(), f"side {raw.info['side']}: {int((~kept[sub]).sum())} subnormal inputs not kept"


@pytest.mark.parametrize("variant", BFV, ids=_vid)
def test_bf16_nonfinite_operands(variant):
    """B-c: one infinity and one NaN in an A row and in a B row (both signs, inside a full stage and
    inside the K tail), and one product that overflows f32: the affected rows and columns equal the
    oracle by class (inf with its sign, or NaN), every other output bit for bit."""
    raws, refs = _problems("bc", E.bf16_nonfinite_problems)
    for raw, ref in zip(raws, refs):
        assert not np.isnan(np.delete(np.delete(ref, raw.info["rows"], axis=0), raw.info["cols"], axis=1)).any()
    _run_exact(raws, refs, variant)


# ------------------------------------------------------------------ paths these two types had never run
def _strided_raws():
    ea = [E.gen_e4m3_window(130, 136, 432, wa, wb, seed=910 + i) for i, (wa, wb) in enumerate(E.EA_WINDOWS[2:4])]
    ba = [E.gen_bf16_exact(130, 136, 216, "eighths", seed=920 + i) for i in range(2)]
    return ea + ba


@pytest.mark.parametrize("t", [0, 1], ids=["e4m3", "bf16"])
@pytest.mark.parametrize("variant", BOTH, ids=_vid)
def test_strided_c_and_guards(variant, t):
    """Two problems written side by side into one C buffer through c_col0, with ldc = 2 N + 24 and a
    guard row behind row M: the outputs are exact and every guard element keeps its bits."""
    raws, refs = _problems("strided", _strided_raws)
    raws, refs = raws[2 * t:2 * t + 2], refs[2 * t:2 * t + 2]
    M, N = raws[0].M, raws[0].N
    C = torch.full((M + 1, 2 * N + 24), SENTINEL, dtype=torch.int16, device=DEV).view(torch.float16)
    hps = []
    for i, raw in enumerate(raws):
        h = HostProblem.from_raw(raw, None)
        h._bind(DEV, 0, C, i * N)
        assert h.problem.ldc == 2 * N + 24
        hps.append(h)
    GroupGemm([h.problem for h in hps], variant=variant).launch()
    torch.cuda.synchronize()
    full = C.cpu().numpy()
    for i, (h, ref) in enumerate(zip(hps, refs)):
        _assert_same(full[:M, i * N:(i + 1) * N], ref, _what(h, f" at column {i * N}"))
    assert (E.f16_bits(full[:M, 2 * N:]) == SENTINEL).all(), "a guard column was written"
    assert (E.f16_bits(full[M]) == SENTINEL).all(), "the guard row was written"


def _graph_raws():
    return [E.gen_e4m3_window(150, 264, 432, *E.EA_WINDOWS[4], seed=930), E.gen_bf16_exact(90, 136, 216, "eighths", seed=931),
            E.gen_e4m3_window(150, 264, 432, *E.EA_WINDOWS[5], seed=932), E.gen_bf16_exact(90, 136, 216, "ints", seed=933)]


@pytest.mark.parametrize("variant", BOTH, ids=_vid)
def test_graph_replay_and_rebind(variant):
    """An E4M3 + bf16 call captured once and replayed after C is refilled with NaN, then rebound to a
    second operand set of the same shapes: bit for bit both times."""
    raws, refs = _problems("graph", _graph_raws)
    first = [HostProblem.from_raw(r, DEV) for r in raws[:2]]
    second = [HostProblem.from_raw(r, DEV) for r in raws[2:]]
    gg = GroupGemm([h.problem for h in first], variant=variant)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        gg.launch(s)
    for h in first:
        h.problem.C.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for h, ref in zip(first, refs[:2]):
        _assert_same(h.result(), ref, _what(h, " graph replay"))
    gg.rebind([h.problem for h in second])
    gg.launch()
    torch.cuda.synchronize()
    for h, ref in zip(second, refs[2:]):
        _assert_same(h.result(), ref, _what(h, " after rebind"))


def _mixed_raws():
    return [E.gen_e4m3_window(300, 264, 256, *E.EA_WINDOWS[0], seed=940), E.gen_bf16_exact(200, 264, 216, "eighths", seed=941),
            U.gen_f16_readout(256, 264, seed=942), E.gen_e4m3_ladder(37, 136, 256, seed=943),
            E.gen_bf16_exact(5, 136, 64, "ints", seed=944)]


@pytest.mark.parametrize("variant", EVERY, ids=_vid)
def test_mixed_launch_every_type_exact(variant):
    """Exact E4M3, bf16 and fp16 problems beside w8a8 and w4a4 problems and an M = 0 E4M3 problem in one
    launch (the every-body build): every output bit for bit."""
    raws, refs = _problems("mixed", _mixed_raws)
    hps = [HostProblem.from_raw(r, DEV) for r in raws]
    ints = [HostProblem(513, 256, 128, W8A8, seed=951, device=DEV), HostProblem(129, 384, 512, W4A4, seed=952, device=DEV)]
    empty = HostProblem.from_raw(U.Raw(0, 256, 256, W8A8_E4M3, np.zeros((0, 256), np.uint8), raws[0].B[:256, :256].copy(),
                                       np.zeros(0, np.float16), np.ones(256, np.float16)), DEV)
    order = [hps[0], ints[0], hps[1], empty, hps[2], ints[1], hps[3], hps[4]]
    gg = GroupGemm([h.problem for h in order], variant=variant)
    for q in (W8A8_E4M3, BF16, W8A8, W4A4, U.FP16):
        assert nat.variant_supports(gg.variant, q.qcfg)
    want = (1 << 0) | (1 << 1) | (1 << 2) | (1 << 7) | (1 << 8)  # fp16, w8a8, w4a4, E4M3, bf16: one build with all five bodies
    assert gg.info.qtype_mask & want == want, hex(gg.info.qtype_mask)
    gg.launch()
    torch.cuda.synchronize()
    for h, ref in zip(hps, refs):
        _assert_same(h.result(), ref, _what(h))
    for h in ints:
        _assert_same(h.result(), h.expected(), _what(h))
    assert torch.isnan(empty.Cbuf).all()  # the M = 0 problem wrote nothing
