"""The decode forward's MFMA tile on edge values, without a GPU: what tests/test_decode_lp_edges_gpu.py runs is exact,
holds the value classes its docstrings claim, and is sensitive — a kernel wrong in one of the ways named there would
produce different fp16 bits (tests/_decode_lp_edges.wrong_linear restates each wrong kernel on the reference side).

The families (tests/_decode_lp_edges.py): L-a the A quantiser read out, L-b exact sums through a whole layer, L-c the
E4M3 scale ladder, L-d the MX scale range, L-e the geometry (wide tiles, cut batches)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import quantize as qz
from tests import _decode_lp_edges as ed
from tests import _gptoss_ref as gref
from tests._fp8_bf16_edges import mismatch

LB_CASES = ed.LB_CASES


def _differs(p: ed.DownProblem, variant: str, **kw) -> bool:
    (y, ys), (wy, wys) = p.expected, p.wrong(variant, **kw)
    return bool(mismatch(wy, y).any() or mismatch(wys, ys).any())


def _subnormal(y):
    return (y != 0) & (np.abs(y.astype(np.float64)) < 2.0 ** -14)


@pytest.mark.parametrize("K", [640, 1152])
@pytest.mark.parametrize("kind", ed.KINDS)
def test_la_readout_classes_and_sensitivity(kind, K):
    """L-a: every row class of LA_ROWS quantises as the header says, and a quantiser without the floor, with ties away
    from zero, with an Inf block kept, a mis-paired A scale byte or swapped fp8 halves changes output bits."""
    p = ed.la_problem(kind, K)
    rows = p.info["rows"]
    c, s = ed.quant_a(kind, rows)
    i = ed.LA_ROWS.index
    if kind == "e4m3":
        assert s[i("zero")] == 1 and s[i("neg_zero")] == 1
        assert s[i("subnormal")] == 2.0 ** -14 == s[i("below_floor")]  # the floor
        assert np.abs(rows[i("below_floor")].astype(np.float64)).max() < 448 * 2.0 ** -14
        assert (c[i("ties")] == 0x7E).any() and s[i("ties")] == 1 and s[i("ties_small")] == 2.0 ** -5
        y = rows[i("ties")].astype(np.float64)
        assert np.isin(np.abs(y), ed.E4M3_TIES).sum() >= 2 * len(ed.E4M3_TIES)  # every midpoint, both signs
        assert _differs(p, "no_floor")
    else:
        assert (s[i("zero")] == 0).all() and (s[i("neg_zero")] == 0).all() and (c[i("neg_zero")] != 0).all()
        for name in ("inf", "nan"):
            assert (s[i(name)] == 255).sum() == 1 and s[i(name), 3] == 255  # one block only
        lad = np.concatenate([s[i("ladder_lo")], s[i("ladder_hi")]])
        assert (lad[1::2] == 0).all() and lad[0::2].min() < 127 - 24
        assert lad[0::2].max() == 127 + 15 - (8 if kind == "mxfp8" else 2)
        sat, top = (448.0, 256.0) if kind == "mxfp8" else (6.0, 4.0)
        scale = np.repeat(np.exp2(s[i("ties")].astype(np.float64) - 127), 32)
        y = rows[i("ties")].astype(np.float64) / scale
        assert (np.abs(y) > sat).any() and (y > sat).any() and (y < -sat).any()  # above saturation, both signs
        ties = ed.E2M1_TIES if kind == "mxfp4" else (464.0,)
        for t in ties:
            assert (y == t).any() and (y == -t).any(), t
        assert _differs(p, "neighbour", side="a") and _differs(p, "step", side="a")
    y, ys = p.expected
    bad = [i("inf"), i("nan")]
    assert np.isnan(y[bad]).all() and not np.isnan(np.delete(y, bad, axis=0)).any()
    assert np.isnan(ys).all(axis=1).sum() == 2
    assert _differs(p, "quant_tie_away") and _differs(p, "inf_kept")
    if kind != "mxfp4":
        assert _differs(p, "halves")


def _ref_act(case: ed.LayerCase, b1=None, b1s=None):
    """the CPU restatement of the layer's act rows (pair order) and shared act rows"""
    flat, topk = case.ids.reshape(-1), case.ids.shape[1]
    glu = (lambda gu, b: gref.glu(gu, b, act="clamp")) if case.info["clamp"] else (lambda gu, b: gref.glu(gu, b))
    act = np.stack([glu(case.gu_ref(e, case.hidden[p // topk:p // topk + 1]), None if b1 is None else b1[e])[0]
                    for p, e in enumerate(flat)])
    return act.astype(np.float16), glu(case.gu_ref(case.E, case.hidden), b1s).astype(np.float16)


@pytest.mark.parametrize("name,shape,T", LB_CASES)
def test_lb_layer_is_exact_and_sensitive(name, shape, T):
    """L-b: both stages' bounds (the down stage on the CPU restatement of act, with a factor 2 in hand for last-bit
    differences of the device's act, which the GPU test re-checks on the device's own rows); the hidden rows quantise
    to the intended codes and bytes; a weight scale byte taken from the neighbouring block, from step u ^ 1 of the dword
    or — K > 1024 — from the first 16-byte group changes bits."""
    case = ed.layer_case(name, shape, T)
    assert case.bound1 < case.limit(0), case.bound1
    assert case.span1 < ed.SPAN, case.span1
    ed.assert_quantises_to(case.info["hid_kind"], case.hidden, case.info["hcodes"], case.info["hscales"])
    assert T == 1 or len(np.unique(case.info["hscales"])) >= (2 if name == "e4m3" else 4)
    act, act_s = _ref_act(case)
    assert np.isfinite(act).all() and np.isfinite(act_s).all()
    assert case.bound2(act, act_s) < case.limit(1) / 2, case.bound2(act, act_s)
    assert case.span2(act, act_s) < ed.SPAN, case.span2(act, act_s)
    for e, (k1, k2) in enumerate(case.pairs):
        for k, w, x in ((k1, case.w1[e], case.hidden), (k2, case.w2[e], act_s if e == case.E else act[:2])):
            if not w.mx:
                continue
            assert len(np.unique(w.scales)) >= (4 if w is case.w1[e] else 2)
            good = ed.ref_linear(k, x, w)
            K = w.codes.shape[1]  # (K = 128 is one step: no other step's byte to take)
            variants = ("neighbour",) + (("step",) if K > 128 else ()) + (("group",) if K > 1024 else ())
            for v in variants:
                assert mismatch(ed.wrong_linear(v, k, x, w), good).any(), (e, k, v)
    for w in case.w1 + case.w2:  # the w4a16 weights come back from the layer's own quantiser unchanged
        if w.kind == "w4a16":
            c, sz = qz.quant_weightonly(torch.from_numpy(w.codes), 4, -1, False)
            sz = sz.reshape(-1, 2).double().numpy()
            assert np.array_equal(c.numpy() * sz[:, :1] + sz[:, 1:], w.values()) and (np.log2(sz[:, 0]) % 1 == 0).all()
    k1 = case.pairs[case.E][0]
    if k1 in ("e4m3", "mxfp8"):
        assert mismatch(ed.wrong_linear("halves", k1, case.hidden, case.w1[case.E]), case.gu_ref(case.E, case.hidden)).any()


def test_lb_special_cases_are_exact():
    """the biased SwigluClamp case (bounds without the biases: they move act by less than one binade) and the
    interleaved one (every weight block holds a 4 or a 6, so MoEFFN's requantisation returns its byte)"""
    case = ed.layer_case("mxfp8", "c", 5, clamp=True)
    act, act_s = _ref_act(case)
    assert case.bound1 < case.limit(0) and case.bound2(act, act_s) < case.limit(1) / 2
    case = ed.layer_case("mxfp8", "c", 5, anchor=True)
    act, act_s = _ref_act(case)
    assert case.bound1 < case.limit(0) and case.bound2(act, act_s) < case.limit(1) / 2
    for w in case.w1 + case.w2:
        assert w.scales.min() >= 104 and w.scales.max() <= 140  # fp16 holds every value
        c, s = qz.quant_mxfp4(torch.from_numpy(w.values()).half())
        assert np.array_equal(s.numpy(), w.scales) and np.array_equal(c.numpy(), w.packed())


@pytest.mark.parametrize("T", [7, 16])
def test_lc_scale_ladder(T):
    """L-c: exact; the scale products hold a tie, subnormals, zero by underflow and an overflowing one; +-Inf and
    nonzero subnormal outputs occur; a product not rounded on its own or a tie rounded away changes bits."""
    p = ed.lc_problem(T)
    p.assert_exact()
    y, ys = p.expected
    both = np.concatenate([y.ravel(), ys.ravel()])
    assert np.isinf(both).any() and _subnormal(both).any() and not np.isnan(both).any()
    assert (both == np.inf).any() and (both == -np.inf).any()
    sa = np.exp2(np.array(ed.LC_KS, np.float64))
    prod = sa[:, None] * ed.LC_SB.astype(np.float64)[None, :]
    p16 = prod.astype(np.float16).astype(np.float64)
    assert ((p16 == 0) & (prod != 0)).any() and _subnormal(p16).any() and (p16 >= 25600).any()
    half = 2.0 ** -25
    assert (np.abs(p16 - prod) == half).sum() >= 2  # ties on the subnormal grid
    assert _differs(p, "scale_once") and _differs(p, "tie_away")


@pytest.mark.parametrize("T", [1, 7, 16])
@pytest.mark.parametrize("kind", ["mxfp8", "mxfp4"])
def test_ld_scale_range(kind, T):
    """L-d: exact (one byte per row on either side); overflow and nonzero subnormals both occur."""
    p = ed.ld_problem(kind, T)
    p.assert_exact()
    y, ys = p.expected
    both = np.concatenate([y.ravel(), ys.ravel()])
    assert np.isinf(both).any() and _subnormal(both).any() and not np.isnan(both).any()
    e = p.weights[0].scales.astype(int).max() + 131 - 254, p.weights[0].scales.astype(int).min() + 115 - 254
    assert e[0] >= 30 and e[1] <= -40
    assert _differs(p, "tie_away")


def test_le_geometry_rules():
    """L-e: the shapes reach ct = 64 and 128 by geometry()'s rule and C is the smallest candidate that does; K = 4096
    cuts the E4M3 / MXFP8 batch to 14 rows."""
    for ct, C in ed.LE_WIDE_C.items():
        assert ed.decode_ct(64, 16, 4, C, C) == ct and ed.decode_ct(64, 16, 4, C // 2, C // 2) == ct // 2
        assert ed.decode_ct(64, 16, 4, C) == ct  # (without a shared expert too)
    assert ed.decode_ct(4, 16, 2, 1152, 1152) == 32 and ed.decode_ct(60, 16, 4, 1408, 5632) == 64
    assert ed.lp_rb(["e4m3"], 4096) == 14 == ed.lp_rb(["mxfp8"], 4096) and ed.lp_rb(["mxfp4"], 4096) == 16
    assert ed.lp_rb(["e4m3"], 1152) == 16


@pytest.mark.parametrize("kind", ed.KINDS)
def test_le_cut_batches_exact(kind):
    p = ed.le_cut_problem(kind)
    p.assert_exact()
    assert np.isfinite(p.expected[0]).all() and (p.ids == 2).all() and p.act.shape == (64, 4096)
    assert _differs(p, "group") if kind != "e4m3" else _differs(p, "halves")


@pytest.mark.parametrize("ct", [64, 128])
def test_le_wide_tiles_exact(ct):
    p = ed.le_wide_down_problem(ct)
    p.assert_exact()
    assert p.info["ct"] == ed.decode_ct(64, 16, 4, p.H, p.H) == ct
    assert all(len(set(r)) == 4 for r in p.ids.tolist()) and np.isfinite(p.expected[0]).all()
    assert {p.kinds[e] for e in p.ids.reshape(-1)} == set(ed.WIDE_KINDS)
    for k in ("w8a8", "fp16"):  # the rows of the expert_tile kinds are exact in the sense their sums need
        e = p.kinds.index(k)
        rows = p.act[p.ids.reshape(-1) == e]
        a, sa = ed.a_values(k, rows)
        if k == "w8a8":
            assert (np.log2(sa.astype(np.float64)) % 1 == 0).all() and np.array_equal(a * sa.astype(np.float64)[:, None], rows)
            c, s = qz.quant_rtn_sym(torch.from_numpy(p.weights[e].fp16()), 8)
            assert np.array_equal(c.numpy(), p.weights[e].codes) and np.array_equal(s.numpy(), p.weights[e].scales)


@pytest.mark.parametrize("ct", [64, 128])
def test_le_wide_gate_up_layer_exact(ct):
    """L-e (i), gate_up: the 64-expert layer's gate_up sums are exact for every kind whose sum is an f32 one (w8a8 is
    integer arithmetic), and its shape reaches the ct."""
    case = ed.wide_layer_case(ct)
    assert ed.decode_ct(case.E, 16, 4, case.N, case.Ns) == ct == case.info["ct"]
    assert all(len(set(r)) == 4 for r in case.ids.tolist())
    assert {case.pairs[e][0] for e in case.ids.reshape(-1)} == set(ed.WIDE_KINDS)
    assert case.bound1 < case.limit(0) and case.span1 < ed.SPAN, (case.bound1, case.span1)
    ed.assert_quantises_to("mxfp4", case.hidden, case.info["hcodes"], case.info["hscales"])


@pytest.mark.parametrize("kind", ed.KINDS)
def test_lf_dense_down_exact_and_sensitive(kind):
    """L-f: exact; weight bytes of four values per block on the down entry at K = 1152; a byte of the neighbouring
    block, of step u ^ 1 or of the first scale group, or swapped fp8 halves, changes bits; sums cancel (both signs)."""
    p = ed.dense_down_problem(kind)
    p.assert_exact()
    y, _ = p.expected
    assert np.isfinite(y).all() and (y > 0).any() and (y < 0).any()
    if kind != "e4m3":
        assert all(len(np.unique(w.scales)) >= 4 for w in p.weights)
        assert _differs(p, "neighbour") and _differs(p, "step") and _differs(p, "group")
        assert _differs(p, "neighbour", side="a") and _differs(p, "step", side="a") and _differs(p, "group", side="a")
    if kind != "mxfp4":
        assert _differs(p, "halves")
