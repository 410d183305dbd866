"""bf16 layers without a GPU (mxmoe_moe_gate_dt, mxmoe_moe_gather_quant, mxmoe_moe_combine_dt; moe.gate, quant_act,
MoEBlock, GraphForward with bf16 ends): the C ABI's host validation (dummy pointers, refused before any HIP call), the
Python dtype checks, and that the data generators of tests/test_bf16_layer_gpu.py mean what those tests assume."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from tests import _bf16_ref as bref
from tests import _gate_modes_ref as mref
from tests import _gate_ref as ref

FP16, BF16 = nat.DT_FP16, nat.DT_BF16


def _err():
    return nat.lib().mxmoe_gg_last_error()


def _gate(dtype=BF16, hidden=16, w_gate=16, w_sg=None, T=4, H=64, E=384, topk=8, renorm=1, scoring=1, e_bias=None,
          n_group=1, topk_group=1, group_top=1, routed_scale=1.0, logit_bias=None, ids=16, wts=16, shared_w=None,
          logits=None, scores=None):
    return nat.symbol("mxmoe_moe_gate_dt")(dtype, hidden, w_gate, w_sg, T, H, E, topk, renorm, scoring, e_bias, n_group,
                                          topk_group, group_top, routed_scale, logit_bias, ids, wts, shared_w, logits,
                                          scores, None)


def _gather(dtype=BF16, hidden=16, T=4, K=128, topk=2, with_shared=0, sorted_e=16, perm=16, segs=16, nseg=4, mask=1, out=16,
            scales=16):
    return nat.symbol("mxmoe_moe_gather_quant")(dtype, hidden, T, K, topk, with_shared, sorted_e, perm, segs, nseg, mask, out,
                                               scales, None)


def _combine(dtype=BF16, y=16, inv=16, sorted_e=None, w=16, bias=None, shared=None, shared_w=None, shared_bias=None, T=4,
             topk=2, E=8, H=128, out=16):
    return nat.symbol("mxmoe_moe_combine_dt")(dtype, y, inv, sorted_e, w, bias, shared, shared_w, shared_bias, T, topk, E, H,
                                             out, None)


def test_abi_symbols_and_constants():
    lib = nat.lib()
    assert lib.mxmoe_gg_abi_version() == 7 == nat.ABI_VERSION
    assert (nat.DT_FP16, nat.DT_BF16) == (0, 1)
    for fn in nat.DT_SYMBOLS:
        assert fn in nat.EXPORTED_SYMBOLS and hasattr(lib, fn)
    assert lib.mxmoe_moe_gate_dt.argtypes == [ctypes.c_int] + lib.mxmoe_moe_gate_wide.argtypes
    assert lib.mxmoe_moe_gate_dt.argtypes[4] is ctypes.c_int64
    assert lib.mxmoe_moe_combine_dt.argtypes == [ctypes.c_int] + lib.mxmoe_moe_combine_bias.argtypes
    assert lib.mxmoe_moe_gather_quant.argtypes[2] is ctypes.c_int64 and lib.mxmoe_moe_gather_quant.argtypes[10] is ctypes.c_uint32


@pytest.mark.parametrize("call,name", [(_gate, b"mxmoe_moe_gate_dt"), (_gather, b"mxmoe_moe_gather_quant"),
                                       (_combine, b"mxmoe_moe_combine_dt")])
def test_unknown_dtype_is_refused_under_the_entrys_name(call, name):
    for dt in (2, -1, 16):
        assert call(dtype=dt) == nat.MXMOE_GG_ERR_INVALID
        assert name in _err()
        assert call(dtype=dt, T=0) == nat.MXMOE_GG_ERR_INVALID  # (before the empty-batch return)
    for dt in (FP16, BF16):
        assert call(dtype=dt, T=0) == nat.MXMOE_GG_OK


@pytest.mark.parametrize("dt", [FP16, BF16])
def test_gate_dt_keeps_the_wide_entrys_limits(dt):
    for kw in (dict(E=513), dict(E=384, n_group=2), dict(E=384, n_group=8, topk_group=4), dict(E=384, group_top=2),
               dict(E=0), dict(topk=17), dict(H=48), dict(T=-1), dict(hidden=8), dict(w_sg=16), dict(scoring=2),
               dict(scoring=0, e_bias=16), dict(routed_scale=float("inf")), dict(E=60, n_group=8)):
        assert _gate(dtype=dt, **kw) == nat.MXMOE_GG_ERR_INVALID, kw
        assert b"mxmoe_moe_gate_dt" in _err(), kw
    assert _gate(dtype=dt, T=0) == nat.MXMOE_GG_OK
    assert _gate(dtype=dt, T=0, hidden=None, w_gate=None, ids=None, wts=None) == nat.MXMOE_GG_OK
    assert _gate(dtype=dt, T=0, E=512, topk=10, scoring=0, w_sg=16, shared_w=16, logits=16, logit_bias=16) == nat.MXMOE_GG_OK
    assert _gate(dtype=dt, T=0, E=256, topk=8, n_group=8, topk_group=4, group_top=2) == nat.MXMOE_GG_OK  # groups: E <= 256
    assert _gate(dtype=dt, T=0, E=8, topk=2, scoring=0) == nat.MXMOE_GG_OK  # every rule at its default


@pytest.mark.parametrize("dt", [FP16, BF16])
def test_gather_and_combine_validation(dt):
    for kw in (dict(K=100), dict(K=16384 + 128), dict(topk=0), dict(nseg=0), dict(T=-1), dict(hidden=8), dict(out=8),
               dict(hidden=None), dict(perm=None)):
        assert _gather(dtype=dt, **kw) == nat.MXMOE_GG_ERR_INVALID, kw
        assert b"mxmoe_moe_gather_quant" in _err(), kw
    assert _gather(dtype=dt, mask=1 << 5) == nat.MXMOE_GG_ERR_UNSUPPORTED and b"mxmoe_moe_gather_quant" in _err()
    assert _gather(dtype=dt, T=0, mask=(1 << 4) | (1 << 6) | 0xF) == nat.MXMOE_GG_OK
    for kw in (dict(H=12), dict(topk=0), dict(E=0), dict(bias=8), dict(shared_bias=16), dict(bias=16, sorted_e=None),
               dict(y=None), dict(out=8)):
        assert _combine(dtype=dt, **kw) == nat.MXMOE_GG_ERR_INVALID, kw
        assert b"mxmoe_moe_combine_dt" in _err(), kw
    assert _combine(dtype=dt, T=0) == nat.MXMOE_GG_OK
    assert _combine(dtype=dt, T=0, sorted_e=None, bias=None, shared_bias=None) == nat.MXMOE_GG_OK


def test_gate_dtype_checks():
    h = torch.zeros(4, 64, dtype=torch.bfloat16)
    w = torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="w_gate"):
        moe.gate(h, w.half(), 2)  # bf16 hidden, fp16 w_gate
    with pytest.raises(ValueError, match="w_gate"):
        moe.gate(h.half(), w, 2)
    with pytest.raises(ValueError, match="w_shared_gate"):
        moe.gate(h, w, 2, w_shared_gate=torch.zeros(64, dtype=torch.float16))
    with pytest.raises(ValueError, match="hidden"):
        moe.gate(h.float(), w.float(), 2)
    with pytest.raises(ValueError, match="hidden"):
        moe.gate(h.double(), w, 2)


def test_quant_act_refuses_other_dtypes():
    r = moe.Routing(torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32), torch.zeros(4, dtype=torch.int32),
                    [4], 4, 1, 1)
    for dt in (torch.float32, torch.float64, torch.int16):
        with pytest.raises(ValueError, match="fp16 or bf16"):
            moe.quant_act(torch.zeros(4, 128, dtype=dt), r, [moe.ACT_FP16], False)
    with pytest.raises(ValueError, match="fp16 or bf16"):  # the reference-named wrappers inherit the check (before routing)
        moe.quant_act(torch.zeros(4, 128, dtype=torch.float32), r, [moe.ACT_INT8], True)
    with pytest.raises(ValueError, match="out_dtype"):
        moe.combine(torch.zeros(4, 128, dtype=torch.float16), r, torch.ones(4, 1), out_dtype=torch.float32)
    with pytest.raises(ValueError, match="out_dtype"):
        moe.combine_bias(torch.zeros(4, 128, dtype=torch.float16), r, torch.ones(4, 1), None, out_dtype=torch.float32)


class _FFN:  # what MoEBlock and GraphForward.launch's first check read of a MoEFFN
    E, H, has_shared = 8, 64, True


def test_moe_block_and_graph_forward_dtype_checks():
    w16, wb = torch.zeros(8, 64, dtype=torch.float16), torch.zeros(8, 64, dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="w_shared_gate"):
        moe.MoEBlock(_FFN(), wb, 2, w_shared_gate=torch.zeros(64, dtype=torch.float16))
    with pytest.raises(ValueError, match="w_shared_gate"):
        moe.MoEBlock(_FFN(), w16, 2, w_shared_gate=torch.zeros(64, dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="fp16 or bf16"):
        moe.MoEBlock(_FFN(), w16.float(), 2)
    blk = moe.MoEBlock(_FFN(), wb, 2, w_shared_gate=torch.zeros(64, dtype=torch.bfloat16))
    assert blk.w_gate.dtype == torch.bfloat16
    with pytest.raises(ValueError, match="router's dtype"):
        blk.forward(torch.zeros(4, 64, dtype=torch.float16))
    # GraphForward: the dtype must be the block's, and launch refuses a hidden of another one (both before any launch)
    with pytest.raises(ValueError, match="differs from the block"):
        moe.GraphForward(blk, 4, dtype=torch.float16)
    with pytest.raises(ValueError, match="fp16 or bf16"):
        moe.GraphForward(blk, 4, dtype=torch.float32)
    gf = object.__new__(moe.GraphForward)  # (planning needs a device; launch's first check does not)
    gf.ffn, gf.T, gf.topk, gf.block, gf.dtype = _FFN(), 4, 2, None, torch.bfloat16
    with pytest.raises(ValueError, match="bfloat16"):
        gf.launch(torch.zeros(4, 64, dtype=torch.float16))
    gf.dtype = torch.float16
    with pytest.raises(ValueError, match="float16"):
        gf.launch(torch.zeros(4, 64, dtype=torch.bfloat16))


def test_bf16_numpy_helpers_agree_with_torch():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * 10.0 ** rng.integers(-30, 30, 4096),
                        np.array([0.0, -0.0, np.inf, -np.inf, 1e5, 65504.0, 2.0 ** -24, 3 * 2.0 ** -26, 3.3895314e38],
                                 dtype=np.float32),
                        # ties: odd and even bf16 neighbours
                        np.array([0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001], dtype=np.uint32).view(np.float32)])
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert (bref.bf16_bits(x) == want).all()
    assert (bref.bf16_value(want).view(np.uint32) == (want.astype(np.uint32) << 16)).all()
    assert bref.is_bf16(bref.bf16_value(want)) and not bref.is_bf16(np.array([1.0 + 2.0 ** -10], dtype=np.float32))


@pytest.mark.parametrize("shape", [(33, 128, 8), (100, 64, 256), (40, 128, 512)])
def test_exact_data_is_bf16(shape):
    T, H, E = shape
    h16, w16, sg16 = ref.exact_data(T, H, E, seed=0, shared=True)
    hidden, w, sg = bref.exact_data(T, H, E, seed=0, shared=True)
    for a16, a in ((h16, hidden), (w16, w), (sg16, sg)):
        assert bref.is_bf16(a) and (a.astype(np.float16).view(np.uint16) == a16.view(np.uint16)).all()
        t = torch.from_numpy(a16)
        assert torch.equal(t.to(torch.bfloat16).to(torch.float16).view(torch.int16), t.view(torch.int16))  # round trip


@pytest.mark.parametrize("T,H,E", [(40, 256, 32), (40, 128, 384), (8, 2048, 16)])
def test_range_data(T, H, E):
    hidden, w = bref.range_data(T, H, E, seed=3)
    assert bref.is_bf16(hidden) and bref.is_bf16(w)
    x = ref.logits_f64(hidden, w)
    assert (x.astype(np.float32).astype(np.float64) == x).all()                 # exact in f32
    assert (np.abs(x) <= 1.0).all() and (x * 2.0 ** 13 == np.rint(x * 2.0 ** 13)).all()
    assert len(np.unique(x)) > 8                                                 # not a degenerate table
    with np.errstate(over="ignore"):
        h16, w16 = hidden.astype(np.float16), w.astype(np.float16)
    assert (~np.isfinite(h16) | (h16 == 0)).all() and np.isinf(h16).any()        # fp16: +-Inf (or the zeros)
    assert (w16 == 0).all() and (w != 0).any()                                   # fp16: all zero
    with np.errstate(invalid="ignore"):
        assert np.isnan(ref.logits_f64(h16, w16)).any()                          # what an fp16 router would compute


@pytest.mark.parametrize("case", bref.ONEHOT_CASES, ids=str)
def test_by_construction_inputs_keep_their_margins_as_bf16(case):
    """The by-construction cases with their table rounded to bf16: the values are exact in bf16 and in fp16, the logits
    table is w_gate transposed, and the rows the GPU test may leave out (margins below the scores' error bound in the
    f64 reference) stay within the helpers' cap of 20 % — asserted here so the GPU test cannot hide behind the mask."""
    T, E, k, n_group, topk_group, seed, H = case
    (hidden, w, bias), (ids, wts, s, x), ok = bref.onehot_rows(*case)
    assert bref.is_bf16(hidden) and bref.is_bf16(w)
    assert (w.astype(np.float16).astype(np.float32) == w).all()            # the same values as fp16
    assert (x == w.astype(np.float64)[:, :T].T).all()                       # the logits table is w_gate transposed
    assert np.abs(x).max() == 3.0 and len(np.unique(x)) > E // 4            # the table is still spread over [-3, 3]
    dropped = int((~ok).sum())
    print(f"{case}: {dropped} of {T} rows left out")
    assert dropped <= mref.ONEHOT_MAX_DROPPED * T
    group_top = 2 if n_group > 1 else 1
    em, gm = mref.decision_margins(mref.selection_values(s, bias), k, n_group, topk_group, group_top)
    assert (em[ok] >= mref.EXPERT_MARGIN).all() and (gm[ok] >= mref.GROUP_MARGIN).all()
    assert (np.sort(ids, axis=1) != np.sort(ref.select(x, k), axis=1)).any(), "bias and groups must change some row's routing"


def test_gather_edge_rows():
    x = bref.gather_edge_rows(37, 128, seed=1)
    t = torch.from_numpy(x).to(torch.bfloat16)
    assert torch.equal(t.float(), torch.from_numpy(x))
    h = t.to(torch.float16)
    assert (x[0] == 0).all() and np.signbit(x[1, 0::2]).all()
    assert h[1, 0].item() == 0 and np.signbit(h[1, 0::2].numpy()).all()          # -0 stays -0
    sub = h[2, :5].view(torch.int16).tolist()
    assert sub == [16, 1, 0, 2, 0]  # 2^-20 = 16 ulps; 3 * 2^-26 -> 1; the ties 2^-25 -> 0 and 3 * 2^-25 -> 2; 2^-26 -> 0
    assert torch.isinf(h[3, 5]) and torch.isinf(h[3, 125]) and h[3, 125] < 0
    assert not torch.isnan(h).any()


def test_combine_reference_rounds_once_to_bf16():
    y = np.array([[1.0, 2.0 ** -9, -3.0, 0.5]], dtype=np.float16)
    w = np.array([[1.0 + 2.0 ** -8]], dtype=np.float32)  # 1.00390625: y * w = y + y * 2^-8, a tie for y = 1
    acc = bref.combine_acc(y, np.array([0]), None, w, 1)
    assert (acc == y.astype(np.float32) * w).all()
    bits = bref.combine_bf16(y, np.array([0]), None, w, 1)
    assert (bits == torch.from_numpy(acc).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)).all()
    assert bref.bf16_value(bits)[0, 0] == 1.0  # 1 + 2^-8 lies halfway between 1 and 1 + 2^-7: to even
