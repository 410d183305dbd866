"""Weight-only MXFP4 (w4a16_g32_sym_MXFP4: fp16 activations on the MXFP4 B operand) on the host: the
qcfg plumbing, the C-ABI's validation, which variants carry the type, AUTO's choice, the CLI's CPU
reference and the weight preparation (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import SUPPORTED, W4A4_MXFP4, W4A16_MXFP4, Problem, QParams
from tests import _mxfp4_ref as ref

WO3, V2X, V3 = "wo3_64x256_w8_3wg", "v2x_256x256_w8_b3_buf_spread_edma", "v3_256x128_w4_dma_ring3_2wg"


def _names():
    return [ln.split()[1] for ln in nat.list_variants()]


def test_qcfg_round_trip():
    q = QParams(16, 4, 32, True, fmt="MXFP4")
    assert q == W4A16_MXFP4 and q.qcfg == "w4a16_g32_sym_MXFP4" and q.fmt_code == nat.FMT_MXFP4
    assert q.is_weight_only and q.is_quant
    assert QParams.from_qcfg(q.qcfg) == q and SUPPORTED[q.qcfg] == q
    assert QParams.from_qcfg("w4a4_g32_sym_MXFP4") == W4A4_MXFP4 and not W4A4_MXFP4.is_weight_only


def test_problem_dtype_checks():
    a, b = torch.zeros(8, 128, dtype=torch.float16), torch.zeros(16, 64, dtype=torch.uint8)
    c, sc = torch.zeros(8, 16, dtype=torch.float16), torch.zeros(16, 16, dtype=torch.uint8)
    Problem(a, b, c, 8, 16, 128, W4A16_MXFP4, None, sc)  # scale_a None
    with pytest.raises(ValueError, match="A must be"):
        Problem(b[:8], b, c, 8, 16, 128, W4A16_MXFP4, None, sc)
    with pytest.raises(ValueError, match="B"):
        Problem(a, b.to(torch.int8), c, 8, 16, 128, W4A16_MXFP4, None, sc)
    with pytest.raises(ValueError, match="scale_b"):
        Problem(a, b, c, 8, 16, 128, W4A16_MXFP4, None, sc.half())
    with pytest.raises(ValueError, match="64-element"):
        Problem(a[:, :96], b[:, :48], c, 8, 16, 96, W4A16_MXFP4, None, sc)


def _prob(**kw):
    d = dict(A=16, B=16, scale_a=0, scale_b=16, C=16, M=64, N=128, K=256, a_bits=16, w_bits=4, gsize=32, sym=1,
             fmt=nat.FMT_MXFP4)
    d.update(kw)
    return nat.GGProblemC(**d)


def _a4(**kw):
    d = dict(scale_a=16, a_bits=4)
    d.update(kw)
    return _prob(**d)


def _plan(problems, variant, ws_bytes=1 << 20):
    arr = (nat.GGProblemC * len(problems))(*problems)
    info = nat.GGPlanInfo()
    st = nat.lib().mxmoe_gg_plan(arr, len(problems), variant, None, ws_bytes, None, ctypes.byref(info))
    return st, nat.lib().mxmoe_gg_last_error().decode()


@pytest.mark.parametrize("kw,status,msg", [
    (dict(K=96), nat.MXMOE_GG_ERR_INVALID, "K % 64"),
    (dict(scale_b=0), nat.MXMOE_GG_ERR_INVALID, "NULL scale"),
    (dict(scale_b=18), nat.MXMOE_GG_ERR_INVALID, "4-byte aligned"),
    (dict(N=132), nat.MXMOE_GG_ERR_INVALID, "multiple of 8"),
    (dict(a_bits=8), nat.MXMOE_GG_ERR_UNSUPPORTED, "w4a16_g32_sym_MXFP4"),
    (dict(gsize=-1), nat.MXMOE_GG_ERR_UNSUPPORTED, "w4a4_g32_sym_MXFP4"),
    (dict(sym=0), nat.MXMOE_GG_ERR_UNSUPPORTED, "w4a16_g32_sym_MXFP4"),
])
def test_plan_validation(kw, status, msg):
    for variant in (nat.default_variant(), _names().index(WO3)):
        st, err = _plan([_prob(), _prob(**kw)], variant)
        assert st == status, err
        assert msg in err and "problem 1" in err


def test_plan_accepts_null_scale_a():
    for variant in (nat.default_variant(), _names().index(WO3), nat.VARIANT_AUTO):
        st, err = _plan([_prob(scale_a=0), _prob(scale_a=16, K=1408)], variant, ws_bytes=0)
        assert st == nat.MXMOE_GG_ERR_WORKSPACE, err  # passed validation, stopped at the workspace check


def test_variant_support():
    names = _names()
    for name in (WO3, V2X):
        assert nat.variant_supports(names.index(name), "w4a16_g32_sym_MXFP4")
        st, err = _plan([_prob()], names.index(name), ws_bytes=0)
        assert st == nat.MXMOE_GG_ERR_WORKSPACE, (name, err)
    st, err = _plan([_prob()], names.index(V3))
    assert st == nat.MXMOE_GG_ERR_UNSUPPORTED and "does not implement" in err, err
    lines = nat.list_variants()
    assert "w4a16" not in lines[names.index(V3)]
    assert len(lines) == len(names) and all(len(ln) < 2040 for ln in lines)  # no line was cut short
    assert lines[names.index(WO3)].rstrip().endswith("STAGE=2)") and lines[names.index(V2X)].rstrip().endswith("STAGE=2)")
    # wo3 still has no body for the 4-bit-activation type
    st, err = _plan([_a4()], names.index(WO3))
    assert st == nat.MXMOE_GG_ERR_UNSUPPORTED and "does not implement" in err, err


def test_silu_flag_on_wo3_only():
    names = _names()
    fused = _prob(fmt=nat.FMT_MXFP4 | nat.EPI_SILU_MUL)
    st, err = _plan([fused], names.index(WO3), ws_bytes=0)
    assert st == nat.MXMOE_GG_ERR_WORKSPACE, err
    st, err = _plan([fused], names.index(V2X))
    assert st == nat.MXMOE_GG_ERR_UNSUPPORTED and "SiLU epilogue" in err, err


def _auto(*probs):
    arr = (nat.GGProblemC * len(probs))(*probs)
    return _names()[nat.resolve_variant(arr, len(probs))]


def test_auto():
    w8 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=8, N=128, K=256, a_bits=8, w_bits=8, gsize=-1, sym=1)
    for M in (1, 35, 512):
        assert _auto(_prob(M=M, N=2816, K=2048)) == WO3
        assert _auto(_prob(M=M, N=2816, K=2048), w8) == WO3
    assert _auto(_prob(M=513, N=2816, K=2048)) == V2X
    assert _auto(_prob(M=4096, N=2816, K=2048), w8) == V2X
    # beside a 4-bit-activation MXFP4 problem (v2x is the only variant with that body), even an empty one
    assert _auto(_prob(M=8), _a4(M=8)) == V2X
    assert _auto(_prob(M=8), _a4(M=0)) == V2X
    # an empty problem of the new type does not change the choice
    w4 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=4096, N=2816, K=2048, a_bits=4, w_bits=4, gsize=-1, sym=1)
    assert _auto(w4) == V3 and _auto(w4, _prob(M=0)) == V3
    assert _auto(w8) == _auto(w8, _prob(M=0))


def test_plan_info_mask_bit():
    assert nat.lib().mxmoe_gg_abi_version() == 7
    st, err = _plan([_prob()], nat.default_variant(), ws_bytes=0)
    assert st == nat.MXMOE_GG_ERR_WORKSPACE, err


def test_expected_sample_on_cpu():
    from mxmoe_amd.check import expected_sample
    from mxmoe_amd.harness import build_layer_inputs
    from mxmoe_amd.workload import QShape, parse_qstr

    assert parse_qstr("w4a16_g32_sym_MXFP4") == dict(w_bits=4, a_bits=16, gsize=32, sym=True, fmt="MXFP4")
    s = QShape([5, 16, 192], **parse_qstr("w4a16_g32_sym_MXFP4"))
    assert s.qcfg == "w4a16_g32_sym_MXFP4" and QShape.from_json(s.to_json()) == s
    p = build_layer_inputs([s], device="cpu", seed=3).problems[0]
    assert p.A.dtype == torch.float16 and p.A.shape == (5, 192) and p.scale_a is None
    assert p.B.shape == (16, 96) and p.scale_b.shape == (16, 16) and p.scale_b.dtype == torch.uint8
    rows, cols = torch.arange(5), torch.tensor([0, 3, 15])
    want, exact = expected_sample(p, rows, cols)
    b = ref.dequant(p.B.numpy(), qz.unpack_mxfp4_scales(p.scale_b, 192).numpy())
    assert not exact and np.array_equal(want.numpy(), (p.A.numpy().astype(np.float64) @ b.T)[:, [0, 3, 15]])


def test_prepare_weight_shares_the_a4_operand():
    from mxmoe_amd import moe

    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 192, generator=g) * 0.3).half()
    w4, w16 = moe.prepare_weight(w, W4A4_MXFP4), moe.prepare_weight(w, W4A16_MXFP4)
    assert torch.equal(w4.B, w16.B) and torch.equal(w4.scale_b, w16.scale_b)
    assert w16.q == W4A16_MXFP4 and (w16.N, w16.K) == (64, 192)
    codes, sc = ref.quant(w.numpy())
    assert np.array_equal(w16.B.numpy(), codes) and np.array_equal(w16.scale_b.numpy(), ref.pack_scales(sc))
    # the fused-layout weight: the rows (and their scales) interleaved, quantised per row as before
    wi = moe.prepare_weight(w, W4A16_MXFP4, interleave=True)
    idx = torch.arange(64).view(2, 2, 16).transpose(0, 1).reshape(-1)
    assert torch.equal(wi.B, w16.B[idx]) and torch.equal(wi.scale_b, w16.scale_b[idx])
    assert moe.qtag_of(16, 32) == moe.ACT_FP16


def test_a16_view_needs_an_all_a4_layer():
    from mxmoe_amd import moe
    from mxmoe_amd.groupgemm import W8A8

    g = torch.Generator().manual_seed(6)
    gu = [(torch.randn(64, 64, generator=g) * 0.2).half() for _ in range(2)]
    dn = [(torch.randn(64, 32, generator=g) * 0.2).half() for _ in range(2)]
    MX = W4A4_MXFP4
    layer = moe.MoEFFN(gu, dn, [(MX, MX), (MX, MX)], num_routed=2)
    v = layer.a16_view()
    assert not v.fuse_silu and v.tag1 == v.tag2 == [moe.ACT_FP16] * 2
    for a, b in zip(layer.w1 + layer.w2, v.w1 + v.w2):
        assert b.q == W4A16_MXFP4 and a.B.data_ptr() == b.B.data_ptr() and a.scale_b.data_ptr() == b.scale_b.data_ptr()
    assert all(w.q == MX for w in layer.w1 + layer.w2)  # the a4 layer is untouched
    with pytest.raises(ValueError, match="a16_view"):
        moe.MoEFFN(gu, dn, [(MX, MX), (W8A8, W8A8)], num_routed=2).a16_view()
