"""Kernels against the oracle on edge operand VALUES (the shapes are small; tests/test_gg_gpu.py and
tests/test_moe.py cover the shape edges on uniform data).

Inputs come from the generators in tests/_util.py; tests/test_value_edges.py proves on the CPU which
value classes each family contains and which wrong arithmetic it exposes. Integer GroupGEMM paths,
the weight-only / fp16 readouts, the quantisers and combine are compared bit for bit; the SiLU modes
within 1 fp16 ulp / 1 code step / 1 scale ulp (hardware exp2 / rcp against libm, oracle/moe_ref.py).
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W4A4_G128, W8A8, GroupGemm, group_gemm
from oracle import moe_ref, oracle
from tests import _util as U
from tests._util import HostProblem

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _variants(qcfg: str) -> list:
    """Every production variant with a tile body for qcfg, plus AUTO (None)."""
    return [v for v in nat.production_variants() if nat.variant_supports(v, qcfg)] + [None]


def _vid(v):
    return "auto" if v is None else nat.list_variants()[v].split()[1]


INT_CASES = [(q, v) for q in (W8A8, W4A4, W4A4_G128) for v in _variants(q.qcfg)]
INT_IDS = [f"{q.qcfg}-{_vid(v)}" for q, v in INT_CASES]
V2 = [int(ln.split()[0]) for ln in nat.list_variants() if ln.split()[1].startswith("v2")]
WO = [v for v in nat.production_variants("w4a16_g-1_asym") if not nat.variant_supports(v, "w4a4_g128_sym")]
B3 = [ln.split()[1] for ln in nat.list_variants()].index("v2x_256x256_w8_b3_buf_spread_edma")

_REFS: dict = {}


def _problems(key, make):
    """(raws, oracle outputs) of one problem list, computed once and shared by the variants."""
    if key not in _REFS:
        raws = make()
        _REFS[key] = (raws, [HostProblem.from_raw(r, None).expected() for r in raws])
    return _REFS[key]


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
            out = h.result()
            bad = out.view(np.uint16) != ref.view(np.uint16)
            where = np.argwhere(bad)[:4].tolist()
            assert not bad.any(), (f"{h.q.qcfg} M={h.M} N={h.N} K={h.K} launch {it}: {int(bad.sum())} outputs differ, "
                                   f"first at {where}: got {out[bad][:4]}, expected {ref[bad][:4]}")


# ------------------------------------------------------------------ (a) full code range
@pytest.mark.parametrize("q,variant", INT_CASES, ids=INT_IDS)
def test_full_code_range(q, variant):
    """Bytes uniform over 0..255: codes -128 and -8 (widen_i4 turns -8 into the int8 lane -128)."""
    _run_exact(*_problems(("full", q.qcfg), lambda: U.full_range_problems(q)), variant)


# ------------------------------------------------------------------ (b) large accumulators
@pytest.mark.parametrize("variant", _variants(W8A8.qcfg), ids=_vid)
def test_large_accumulators(variant):
    """|acc| up to 16384 K > 2^24, rows that cancel to acc == 0 (+0 out), and the pair whose f32(acc)
    decides an fp16 tie."""
    _run_exact(*_problems("large", lambda: U.large_acc_problems(False)), variant)


@pytest.mark.parametrize("variant", [None, B3], ids=["auto", "v2x"])
def test_large_accumulators_split_k(variant):
    """The same through split-K (int32 partial slabs reduced in slice order), launched twice."""
    _run_exact(*_problems("large_splitk", lambda: U.large_acc_problems(True)), variant, launches=2, want_splitk=True)


# ------------------------------------------------------------------ (c) scale ladder
@pytest.mark.parametrize("q,variant", INT_CASES, ids=INT_IDS)
def test_scale_ladder(q, variant):
    """Scale products that are ordinary, rounding ties, subnormal, zero by underflow, or large enough
    that the output overflows to +-inf; all-zero A rows; g128: group scales stepping by powers of two,
    one dominant group, two huge groups that cancel."""
    _run_exact(*_problems(("ladder", q.qcfg), lambda: U.ladder_problems(q)), variant)


# ------------------------------------------------------------------ (d) dequant readout
@pytest.mark.parametrize("variant", V2 + WO, ids=_vid)
@pytest.mark.parametrize("q", U.WO_READOUT_QS, ids=[q.qcfg for q in U.WO_READOUT_QS])
def test_dequant_readout(q, variant):
    """A permuted identity for A: C[m, n] = fp16(fma(u - off, s, zp))[n, pi(m)] bit for bit, over every
    code and crafted scales / zero points (subnormal, 2^-14, large, a big zp with a tiny s)."""
    _run_exact(*_problems(("deq", q.qcfg), lambda: U.dequant_readout_problems(q)), variant)


@pytest.mark.parametrize("variant", _variants("fp16"), ids=_vid)
def test_f16_readout_normal_values(variant):
    """fp16 B of every exponent, both signs and +-65504 read back through a permuted identity."""
    raws, refs = _problems("f16", lambda: [U.gen_f16_readout(256, 264, seed=780)])
    assert np.array_equal(refs[0].view(np.uint16), oracle.gg_f16(raws[0].A, raws[0].B, 256, 264, 256).view(np.uint16))
    _run_exact(raws, refs, variant)


@pytest.mark.parametrize("variant", _variants("fp16"), ids=_vid)
def test_f16_readout_subnormal_values(variant):
    """Subnormal fp16 B values beside normal ones: expected as the oracle keeps them (the fp16 MFMA
    keeps input subnormals)."""
    raws, refs = _problems("f16sub", lambda: [U.gen_f16_readout(256, 264, seed=781, subnormal=True)])
    hp = HostProblem.from_raw(raws[0], DEV)
    group_gemm([hp.problem], variant=variant)
    torch.cuda.synchronize()
    out, ref, sub = hp.result(), refs[0], raws[0].info["sub"]
    kept = out.view(np.uint16) == ref.view(np.uint16)
    flushed = sub & (out == 0) & (np.signbit(out) == np.signbit(ref))
    print(f"fp16 readout, subnormal B values: {int(kept[sub].sum())} kept, {int((flushed & ~kept).sum())} flushed "
          f"to signed zero, of {int(sub.sum())}")
    assert kept[~sub].all(), "a normal value beside subnormal ones was not read back"
    assert kept[sub].all(), f"{int((~kept[sub]).sum())} subnormal values not kept"


# ------------------------------------------------------------------ (e) activation kernels
T_ACT, TOPK_ACT, E_ACT = U.ACT_IDS.shape[0], U.ACT_IDS.shape[1], 4
MODES = ("quant_act", "quant_slots", "silu", "silu_il")


def _check_act(b, seg_rows, tags, exact, what):
    for e, (rows, tag) in enumerate(zip(seg_rows, tags)):
        if rows.shape[0] == 0:
            continue
        stored, scale = moe_ref.quant_rows(rows, tag)
        got = b.A(e).cpu().numpy()
        if tag == moe.ACT_FP16:
            d = U.f16_ulp_distance(got, stored)
            assert d.max() <= (0 if exact else 1), f"{what} seg {e}: fp16 rows differ by {d.max()} ulp"
            if exact:
                assert np.array_equal(got.view(np.uint16), stored.view(np.uint16)), f"{what} seg {e}: sign of zero"
            continue
        sg = b.scale(e).cpu().numpy()
        if exact:
            assert np.array_equal(sg.view(np.uint16), scale.view(np.uint16)), \
                f"{what} seg {e} tag {tag}: scales {sg[sg.view(np.uint16) != scale.view(np.uint16)][:4]} != " \
                f"{scale[sg.view(np.uint16) != scale.view(np.uint16)][:4]}"
            assert np.array_equal(got, stored), f"{what} seg {e} tag {tag}: {int((got != stored).sum())} code bytes differ"
            continue
        bits = 8 if tag == moe.ACT_INT8 else 4
        qg = oracle.unpack_wxax(got, bits, rows.shape[1]).astype(np.int32)
        qr = oracle.unpack_wxax(stored, bits, rows.shape[1]).astype(np.int32)
        assert U.f16_ulp_distance(sg, scale).max() <= 1, f"{what} seg {e} tag {tag}: scales differ by more than 1 ulp"
        assert np.abs(qg - qr).max() <= 1, f"{what} seg {e} tag {tag}: codes differ by more than one step"


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _run_quant_act(hidden, ids, shared_tag, what):
    tags = list(U.ACT_TAGS) + [shared_tag]
    r = moe.route(_dev(ids), E_ACT)
    b = moe.quant_act(_dev(hidden), r, tags, with_shared=True)
    torch.cuda.synchronize()
    perm = moe_ref.route(ids, E_ACT)[1]
    _check_act(b, U.act_segments(hidden[perm], hidden, ids), tags, True, what)


def _run_slots(mode, routed, shared, shared_tag, what):
    """routed / shared: the activations (quant_slots) or [gate | up] rows (the SiLU modes)."""
    tags = list(U.ACT_TAGS) + [shared_tag]
    r = moe.route(_dev(U.ACT_IDS), E_ACT)
    if mode == "quant_slots":
        b = moe.silu_mul_quant(_dev(routed), _dev(shared), r, tags, activated=True)
        act_r, act_s = routed, shared
    else:
        il = mode == "silu_il"
        b = moe.silu_mul_quant(_dev(U.interleave_gate_up_cols(routed) if il else routed),
                               _dev(U.interleave_gate_up_cols(shared) if il else shared), r, tags, interleaved=il)
        act_r, act_s = moe_ref.silu_mul(routed), moe_ref.silu_mul(shared)
    torch.cuda.synchronize()
    _check_act(b, U.act_segments(act_r, act_s, U.ACT_IDS), tags, mode == "quant_slots", what)


def _inputs(mode, N, Ns, shared_tag, c):
    if mode == "quant_slots":
        return U.act_slot_call(N, Ns, shared_tag, c)
    return U.gen_silu_inputs(T_ACT * TOPK_ACT, N, seed=c), U.gen_silu_inputs(T_ACT, Ns, seed=100 + c)


@pytest.mark.parametrize("shared_tag", U.ACT_TAGS)
@pytest.mark.parametrize("mode", MODES[:2])
def test_act_special_rows(mode, shared_tag):
    """Every special row kind (all zero, one nonzero, amax 2^-24, subnormal scale, amax 65504, exact
    ties, clamping, -0, a zero 128-group) through every tag, bit for bit."""
    W = 512
    for c in range(len(U.ACT_KINDS)):
        if mode == "quant_act":
            for parity in (0, 1):
                hidden, ids = U.act_hidden_call(W, c, parity)
                _run_quant_act(hidden, ids, shared_tag, f"quant_act c={c} parity={parity}")
        else:
            _run_slots(mode, *U.act_slot_call(W, W, shared_tag, c), shared_tag, f"quant_slots c={c}")


@pytest.mark.parametrize("W", U.ACT_WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_act_widths(mode, W):
    """One launch of width W (K, or N = Ns): the widths reach every MAXC instantiation of
    act_quant_kernel in every mode (asserted below and in tests/test_value_edges.py)."""
    i = U.ACT_WIDTHS.index(W)
    plan = U.act_launch_plan(T_ACT * TOPK_ACT, T_ACT, W, W)
    assert len(plan) == 1 and plan[0][0] == "one_launch"
    assert {U.act_launch_plan(T_ACT * TOPK_ACT, T_ACT, w, w)[0][1] for w in U.ACT_WIDTHS} == set(U.ACT_MAXC)
    if mode == "quant_act":
        hidden, ids = U.act_hidden_call(W, i, i % 2)
        _run_quant_act(hidden, ids, i % 4, f"quant_act K={W}")
    else:
        _run_slots(mode, *_inputs(mode, W, W, i % 4, i), i % 4, f"{mode} N=Ns={W}")


@pytest.mark.parametrize("branch", list(U.ACT_BRANCH_WIDTHS))
@pytest.mark.parametrize("mode", MODES[1:])
def test_act_launch_branches(mode, branch):
    """launch_act's three branches: split rows, two launches because a quarter of the shared row is
    wider than the routed row, two launches because the shared row is the narrower one."""
    N, Ns = U.ACT_BRANCH_WIDTHS[branch]
    plan = [p[0] for p in U.act_launch_plan(T_ACT * TOPK_ACT, T_ACT, N, Ns)]
    assert plan == (["split_row"] if branch == "split_row" else ["two_launch"] * 2)
    for tag in U.ACT_TAGS:
        _run_slots(mode, *_inputs(mode, N, Ns, tag, tag), tag, f"{mode} {branch} shared tag {tag}")


@pytest.mark.parametrize("N,Ns", [(1408, 5632), (256, 640)])
@pytest.mark.parametrize("mode", MODES[1:])
def test_act_split_row_peak_in_every_quarter(mode, N, Ns):
    """Split rows: the shared row's maximum in each quarter run in turn and once in the last 128
    columns (the amax crosses the four waves through LDS); Ns = 640 leaves the last quarter empty."""
    assert [p[0] for p in U.act_launch_plan(T_ACT * TOPK_ACT, T_ACT, N, Ns)] == ["split_row"]
    rows = U.gen_split_rows(Ns, seed=5, silu=mode != "quant_slots")
    rows = np.concatenate([rows, rows[:T_ACT - len(rows)]])  # (Ns = 640: four peaks, five tokens)
    for tag in U.ACT_TAGS:
        routed = _inputs(mode, N, Ns, tag, tag)[0]
        _run_slots(mode, routed, rows, tag, f"{mode} split rows Ns={Ns} shared tag {tag}")


# ------------------------------------------------------------------ (f) combine
@pytest.mark.parametrize("topk", U.COMBINE_TOPK)
@pytest.mark.parametrize("H", U.COMBINE_H)
def test_combine_small_and_odd_widths(H, topk):
    """H of one lane, H tails over the 2048-column pass, topk 1 and 8, a zero and a negative weight,
    with and without the shared row and its weight: bit for bit."""
    d = U.gen_combine(3, topk, H, seed=H + topk)
    r = moe.route(_dev(d["ids"]), 8)
    inv = moe_ref.route(d["ids"], 8)[2]
    for sh, sw in ((None, None), (d["shared"], None), (d["shared"], d["shared_w"])):
        out = moe.combine(_dev(d["y"]), r, _dev(d["w"]), None if sh is None else _dev(sh), None if sw is None else _dev(sw))
        torch.cuda.synchronize()
        ref = moe_ref.combine(d["y"], inv, d["w"], topk, sh, sw)
        assert np.array_equal(out.cpu().numpy().view(np.uint16), ref.view(np.uint16)), \
            f"H={H} topk={topk} shared={sh is not None} shared_w={sw is not None}"
