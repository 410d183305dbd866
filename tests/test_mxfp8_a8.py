"""w4a8_g32_sym_MXFP8 (MXFP8 activations on the MXFP4 B operand) on the host: the quantiser rule against
the numpy restatement, the qcfg plumbing, the C-ABI's validation, which variants carry the type, AUTO's
choice, the CLI's CPU reference, the weight preparation and the layer views (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import SUPPORTED, W4A4_MXFP4, W4A16_MXFP4, Problem, QParams
from tests import _mxfp4_ref as ref4
from tests import _mxfp8_ref as ref
from tests._util import assert_f16_close

QCFG = "w4a8_g32_sym_MXFP8"
WO3, V2X, V3 = "wo3_64x256_w8_3wg", "v2x_256x256_w8_b3_buf_spread_edma", "v3_256x128_w4_dma_ring3_2wg"


def _names():
    return [ln.split()[1] for ln in nat.list_variants()]


def _q():
    from mxmoe_amd.groupgemm import W4A8_MXFP8
    return W4A8_MXFP8


# ------------------------------------------------------------------ the codec and the quantiser

def test_decode_all_codes_against_torch():
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(torch.float8_e4m3fn).double().numpy()
    got = ref.e4m3(codes.numpy())
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).sum() == 2
    ok = ~np.isnan(want)
    assert np.array_equal(got[ok], want[ok]) and np.array_equal(np.signbit(got[ok]), np.signbit(want[ok]))
    dq = qz.dequant_mxfp8(codes.reshape(8, 32), torch.full((8, 1), 127, dtype=torch.uint8)).numpy().reshape(-1)
    assert np.array_equal(dq[ok], want[ok])


def _special_blocks() -> np.ndarray:
    """fp16 [rows, 32] blocks at the quantiser's edges."""
    blocks = []
    z = np.zeros(32, np.float16)
    blocks.append(z.copy())  # all-zero: scale code 0, zero codes
    b = z.copy()
    b[3] = -0.0
    blocks.append(b)  # all-zero with a -0: the sign is kept
    b = z.copy()
    b[:4] = np.array([2.0 ** -24, -(2.0 ** -24), 3 * 2.0 ** -24, 2.0 ** -15], np.float16)  # fp16 subnormals
    blocks.append(b)
    b = z.copy()
    b[1] = 2.0 ** -24  # a lone smallest subnormal
    blocks.append(b)
    blocks.append(np.tile(np.array([65504.0, -65504.0, 3.0e4, -1.0], np.float16), 8))  # amax 65504: saturates
    # amax just below a power of two: 1.9990 * 2^8 = 511.75 > 448 saturates, 1.8 -> 460.8 too; 1.5 -> 384 does not
    blocks.append(np.tile(np.array([1.999, -1.8, 1.75, 1.5, -1.76, 1.0, 0.001, -0.0], np.float16), 4))
    # exact ties between neighbouring e4m3 values (amax 256 -> e = 0, the elements are their own scaled values)
    ties = np.array([256.0, 17.0, 19.0, -21.0, 23.0, 1.0625, 1.1875, -1.3125, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10,
                     -(2.0 ** -10), 2.0 ** -11, 9.0, 11.0, 13.0, 15.0, 36.0, 44.0, 52.0, 60.0, 0.5625, 0.6875, -0.0,
                     0.0, 2.0 ** -9, 2.0 ** -8, 1.5 * 2.0 ** -9, 2.5 * 2.0 ** -9, 240.0, 248.0, 232.0], np.float16)
    blocks.append(ties)
    b = np.linspace(-3, 3, 32).astype(np.float16)
    b[5] = np.inf
    blocks.append(b)
    b = np.linspace(-3, 3, 32).astype(np.float16)
    b[0] = np.nan
    blocks.append(b)
    b = np.linspace(-3, 3, 32).astype(np.float16)
    b[31] = -np.inf
    blocks.append(b)
    return np.stack(blocks)


def test_quant_special_blocks_bit_exact():
    x = _special_blocks()
    codes, sc = qz.quant_mxfp8(torch.from_numpy(x))
    rc, rs = ref.quant(x)
    assert np.array_equal(sc.numpy(), rs) and np.array_equal(codes.numpy(), rc)
    assert rs[0, 0] == 0 and not rc[0].any()  # all-zero block
    assert rs[1, 0] == 0 and rc[1, 3] == 0x80 and rc[1].sum() == 0x80  # -0 keeps its sign
    assert rs[3, 0] == 127 - 24 - 8 and rc[3, 1] == 0x78  # 2^-24 -> 256 under scale 2^-32
    assert rs[4, 0] == 127 + 7 and rc[4, 0] == 0x7E and rc[4, 1] == 0xFE  # 65504 / 128 = 511.75 -> +-448
    assert rc[5, 0] == 0x7E and rc[5, 1] == 0xFE and rc[5, 3] == 0x7C  # saturation below the next power of two
    assert (rs[7:, 0] == 255).all() and not rc[7:].any()  # Inf / NaN: NaN scale, zero codes
    # the ties went to the even code: 17 = 16 + 1 lies between 16 (0x58) and 18 (0x59)
    assert rc[6, 1] == 0x58 and rc[6, 2] == 0x5A  # 19 between 18 (0x59) and 20 (0x5A)


def test_quant_random_bit_exact():
    g = torch.Generator().manual_seed(1)
    x = (torch.randn(24, 96, generator=g) * torch.exp2(torch.randint(-14, 12, (24, 1), generator=g).float())).half()
    codes, sc = qz.quant_mxfp8(x)
    rc, rs = ref.quant(x.numpy())
    assert np.array_equal(codes.numpy(), rc) and np.array_equal(sc.numpy(), rs)
    assert np.array_equal(qz.dequant_mxfp8(codes, sc).numpy(), ref.dequant(rc, rs))
    with pytest.raises(TypeError):
        qz.quant_mxfp8(x.float())
    with pytest.raises(ValueError, match="32"):
        qz.quant_mxfp8(x[:, :48])


def test_gemm_f32_blockwise_is_within_the_project_tolerance():
    g = torch.Generator().manual_seed(2)
    K = 2048
    ac, asc = qz.quant_mxfp8(torch.randn(9, K, generator=g).half())
    bc, bsc = qz.quant_mxfp4(torch.randn(24, K, generator=g).half())
    args = (ac.numpy(), asc.numpy(), bc.numpy(), bsc.numpy())
    assert_f16_close(ref.gemm_f32_blockwise(*args).astype(np.float16), ref.gemm(*args), K)


# ------------------------------------------------------------------ qcfg plumbing

def test_qcfg_round_trip():
    q = QParams(8, 4, 32, True, fmt="MXFP8")
    assert q == _q() and q.qcfg == QCFG and q.fmt_code == nat.FMT_MXFP8 == 5
    assert q.is_quant and not q.is_weight_only and not q.is_fp8
    assert QParams.from_qcfg(QCFG) == q and SUPPORTED[QCFG] == q


def test_parse_qstr_qshape_and_tags():
    from mxmoe_amd import moe
    from mxmoe_amd.workload import QShape, parse_qstr

    assert parse_qstr(QCFG) == dict(w_bits=4, a_bits=8, gsize=32, sym=True, fmt="MXFP8")
    s = QShape([5, 16, 192], **parse_qstr(QCFG))
    assert s.qcfg == QCFG and QShape.from_json(s.to_json()) == s
    assert moe.ACT_MXFP8 == 6 and moe._BITS[6] == 8 and moe.qtag_of(8, 32) == moe.ACT_MXFP8
    assert moe.qtag_of(8, -1) == moe.ACT_INT8 and moe.qtag_of(4, 32) == moe.ACT_MXFP4
    assert moe._tag_mask([moe.ACT_INT8, moe.ACT_MXFP8, moe.ACT_MXFP8]) == 0b1000010


def test_problem_dtype_checks():
    a, b = torch.zeros(8, 128, dtype=torch.uint8), torch.zeros(16, 64, dtype=torch.uint8)
    c, sa, sb = torch.zeros(8, 16, dtype=torch.float16), torch.zeros(8, 16, dtype=torch.uint8), torch.zeros(16, 16, dtype=torch.uint8)
    Problem(a, b, c, 8, 16, 128, _q(), sa, sb)
    Problem(a.view(torch.float8_e4m3fn), b, c, 8, 16, 128, _q(), sa, sb)
    with pytest.raises(ValueError, match="A"):
        Problem(a.half(), b, c, 8, 16, 128, _q(), sa, sb)
    with pytest.raises(ValueError, match="scale_a"):
        Problem(a, b, c, 8, 16, 128, _q(), sa.half(), sb)
    with pytest.raises(ValueError, match="32-element"):
        Problem(a[:, :48], b[:, :24], c, 8, 16, 48, _q(), sa, sb)


def test_segment_scale_accounting():
    from mxmoe_amd import moe

    M8, I8, F16 = moe.ACT_MXFP8, moe.ACT_INT8, moe.ACT_FP16
    segs, _, out, scales = moe._make_segments([3, 5, 0, 2, 4], [0, 3, 8, 8, 10], [1408, 1408, 1408, 1408, 640],
                                              [M8, I8, M8, F16, M8], "cpu")
    row = moe._mx_scale_row(1408)
    assert row == 48 and moe._mx_scale_row(640) == 32
    assert [s.out_off for s in segs] == [0, 3 * 1408, 3 * 1408 + 5 * 1408, 8 * 1408, 8 * 1408 + 2 * 1408 * 2]
    # scale offsets in fp16 elements: the MX blocks start 4-byte aligned (even offsets)
    assert [s.scale_off for s in segs] == [0, 3 * row // 2, 3 * row // 2 + 5 + 1, 3 * row // 2 + 6, 3 * row // 2 + 6]
    assert out.numel() == 8 * 1408 + 2 * 1408 * 2 + 4 * 640 and scales.numel() == 3 * row // 2 + 6 + 4 * 32 // 2
    b = moe.ActBatch(out, scales, segs, [M8, I8, M8, F16, M8])
    assert b.A(0).shape == (3, 1408) and b.A(0).dtype == torch.uint8
    assert b.scale(0).shape == (3, 48) and b.scale(0).dtype == torch.uint8 and b.scale(4).shape == (4, 32)


# ------------------------------------------------------------------ the C-ABI

def _prob(**kw):
    d = dict(A=16, B=16, scale_a=16, scale_b=16, C=16, M=64, N=128, K=256, a_bits=8, w_bits=4, gsize=32, sym=1,
             fmt=nat.FMT_MXFP8)
    d.update(kw)
    return nat.GGProblemC(**d)


def _a4(**kw):
    d = dict(a_bits=4, fmt=nat.FMT_MXFP4)
    d.update(kw)
    return _prob(**d)


def _plan(problems, variant, ws_bytes=1 << 20):
    arr = (nat.GGProblemC * len(problems))(*problems)
    info = nat.GGPlanInfo()
    st = nat.lib().mxmoe_gg_plan(arr, len(problems), variant, None, ws_bytes, None, ctypes.byref(info))
    return st, nat.lib().mxmoe_gg_last_error().decode()


@pytest.mark.parametrize("kw,status,msg", [
    (dict(w_bits=8), nat.MXMOE_GG_ERR_UNSUPPORTED, QCFG),
    (dict(gsize=-1), nat.MXMOE_GG_ERR_UNSUPPORTED, QCFG),
    (dict(sym=0), nat.MXMOE_GG_ERR_UNSUPPORTED, QCFG),
    (dict(a_bits=4), nat.MXMOE_GG_ERR_UNSUPPORTED, QCFG),
    (dict(K=48), nat.MXMOE_GG_ERR_INVALID, QCFG),
    (dict(scale_a=0), nat.MXMOE_GG_ERR_INVALID, "NULL scale"),
    (dict(scale_b=0), nat.MXMOE_GG_ERR_INVALID, "NULL scale"),
    (dict(scale_a=18), nat.MXMOE_GG_ERR_INVALID, QCFG + " scales must be 4-byte aligned"),
    (dict(scale_b=18), nat.MXMOE_GG_ERR_INVALID, "4-byte aligned"),
    (dict(N=132), nat.MXMOE_GG_ERR_INVALID, "multiple of 8"),
    (dict(ldb=32), nat.MXMOE_GG_ERR_INVALID, "lda/ldb"),  # 64 B < the 128-B B row of K = 256
])
def test_plan_validation(kw, status, msg):
    for variant in (nat.default_variant(), _names().index(WO3)):
        st, err = _plan([_prob(), _prob(**kw)], variant)
        assert st == status, err
        assert msg in err and "problem 1" in err


def test_plan_accepts_the_type_and_dense_b_rows_of_half_a_bytes():
    for variant in (nat.default_variant(), _names().index(WO3), nat.VARIANT_AUTO):
        st, err = _plan([_prob(), _prob(K=1408, M=0), _prob(K=96, ldb=24)], variant, ws_bytes=0)
        assert st == nat.MXMOE_GG_ERR_WORKSPACE, err  # passed validation, stopped at the workspace check
    assert nat.lib().mxmoe_gg_abi_version() == 7


def test_variant_support():
    names = _names()
    for name in (WO3, V2X):
        assert nat.variant_supports(names.index(name), QCFG)
        st, err = _plan([_prob()], names.index(name), ws_bytes=0)
        assert st == nat.MXMOE_GG_ERR_WORKSPACE, (name, err)
    assert not nat.variant_supports(names.index(V3), QCFG)
    st, err = _plan([_prob()], names.index(V3))
    assert st == nat.MXMOE_GG_ERR_UNSUPPORTED and "does not implement" in err, err
    lines = nat.list_variants()
    assert f" {QCFG}=TileConfig(BM=64, BN=128, BK=128," in lines[names.index(WO3)]
    assert f" {QCFG}=TileConfig(BM=256, BN=256, BK=128," in lines[names.index(V2X)]


def test_silu_flag_on_both_kernels():
    names = _names()
    fused = _prob(fmt=nat.FMT_MXFP8 | nat.EPI_SILU_MUL)
    for name in (WO3, V2X):
        st, err = _plan([fused], names.index(name), ws_bytes=0)
        assert st == nat.MXMOE_GG_ERR_WORKSPACE, (name, err)
    st, err = _plan([_prob(fmt=nat.FMT_MXFP8 | nat.EPI_SILU_MUL, N=136)], names.index(V2X))
    assert st == nat.MXMOE_GG_ERR_INVALID and "N % 32" in err, err
    # the 4-bit-activation type keeps refusing the flag
    st, err = _plan([_a4(fmt=nat.FMT_MXFP4 | nat.EPI_SILU_MUL)], names.index(V2X))
    assert st == nat.MXMOE_GG_ERR_UNSUPPORTED and "SiLU epilogue" in err, err


def _auto(*probs):
    arr = (nat.GGProblemC * len(probs))(*probs)
    return _names()[nat.resolve_variant(arr, len(probs))]


def test_auto():
    w8 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=8, N=128, K=256, a_bits=8, w_bits=8, gsize=-1, sym=1)
    # both sides of the row limit (weighted mean M), alone and beside a w8a8 problem
    for M in (1, 16, 35):
        assert _auto(_prob(M=M, N=2816, K=2048)) == WO3
        assert _auto(_prob(M=M, N=2816, K=2048), w8) == WO3
    for M in (1024, 4096):
        assert _auto(_prob(M=M, N=2816, K=2048)) == V2X
        assert _auto(_prob(M=M, N=2816, K=2048), w8) == V2X
    # beside a 4-bit-activation MXFP4 problem (v2x is the only variant with that body), even an empty one
    assert _auto(_prob(M=8), _a4(M=8)) == V2X
    assert _auto(_prob(M=8), _a4(M=0)) == V2X
    # bf16, E4M3 and g128 problems keep v2x
    bf = nat.GGProblemC(A=16, B=16, C=16, M=8, N=128, K=256, a_bits=16, w_bits=16, gsize=-1, sym=1, fmt=nat.FMT_BF16)
    e4 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=8, N=128, K=256, a_bits=8, w_bits=8, gsize=-1, sym=1,
                        fmt=nat.FMT_E4M3)
    g128 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=8, N=128, K=256, a_bits=4, w_bits=4, gsize=128, sym=1)
    for other in (bf, e4, g128):
        assert _auto(_prob(M=8), other) == V2X
    # an empty problem of the new type does not change the choice
    w4 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=4096, N=2816, K=2048, a_bits=4, w_bits=4, gsize=-1, sym=1)
    assert _auto(w4) == V3 and _auto(w4, _prob(M=0)) == V3
    assert _auto(w8) == _auto(w8, _prob(M=0))
    assert _auto(_a4(M=8)) == _auto(_a4(M=8), _prob(M=0)) == V2X


def test_act_quant_tag_mask():
    fn = nat.lib().mxmoe_moe_act_quant
    err = nat.lib().mxmoe_gg_last_error
    for mask in (1 << 6, 0x5F):  # T = 0: checked and accepted
        assert fn(0, None, None, 0, 2, 128, 0, None, None, None, 1, mask, None, None, None) == nat.MXMOE_GG_OK
    for mask in (1 << 5, 1 << 7, (1 << 6) | (1 << 5)):
        assert fn(0, None, None, 0, 2, 128, 0, None, None, None, 1, mask, None, None, None) == nat.MXMOE_GG_ERR_UNSUPPORTED
        assert b"unknown activation tag" in err()


# ------------------------------------------------------------------ the CLI's reference, weights, views

def test_expected_sample_on_cpu():
    from mxmoe_amd.check import expected_sample
    from mxmoe_amd.harness import build_layer_inputs
    from mxmoe_amd.workload import QShape, parse_qstr

    s = QShape([5, 16, 192], **parse_qstr(QCFG))
    li = build_layer_inputs([s], device="cpu", seed=3)
    p = li.problems[0]
    assert p.A.dtype == torch.uint8 and p.A.shape == (5, 192) and p.scale_a.shape == (5, 16)
    assert p.B.shape == (16, 96) and p.scale_b.shape == (16, 16) and p.scale_b.dtype == torch.uint8
    assert li.bytes_algorithmic() == 5 * 192 + 16 * 96 + 2 * 5 * 16 + (5 + 16) * 6
    rows, cols = torch.arange(5), torch.tensor([0, 3, 15])
    want, exact = expected_sample(p, rows, cols)
    full = ref.gemm(p.A.numpy(), qz.unpack_mxfp4_scales(p.scale_a, 192).numpy(), p.B.numpy(),
                    qz.unpack_mxfp4_scales(p.scale_b, 192).numpy())
    assert not exact and np.array_equal(want.numpy(), full[:, [0, 3, 15]])


def test_prepare_weight_shares_tensors_across_the_three_mx_types():
    from mxmoe_amd import moe

    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 192, generator=g) * 0.3).half()
    w4, w16, w8 = (moe.prepare_weight(w, q) for q in (W4A4_MXFP4, W4A16_MXFP4, _q()))
    assert torch.equal(w4.B, w8.B) and torch.equal(w4.scale_b, w8.scale_b)
    assert torch.equal(w16.B, w8.B) and torch.equal(w16.scale_b, w8.scale_b)
    assert w8.q == _q() and (w8.N, w8.K) == (64, 192)
    codes, sc = ref4.quant(w.numpy())
    assert np.array_equal(w8.B.numpy(), codes) and np.array_equal(w8.scale_b.numpy(), ref4.pack_scales(sc))
    wi = moe.prepare_weight(w, _q(), interleave=True)
    idx = torch.arange(64).view(2, 2, 16).transpose(0, 1).reshape(-1)
    assert torch.equal(wi.B, w8.B[idx]) and torch.equal(wi.scale_b, w8.scale_b[idx])


def test_a8_view():
    from mxmoe_amd import moe
    from mxmoe_amd.groupgemm import W8A8

    g = torch.Generator().manual_seed(6)
    gu = [(torch.randn(64, 64, generator=g) * 0.2).half() for _ in range(2)]
    dn = [(torch.randn(64, 32, generator=g) * 0.2).half() for _ in range(2)]
    for MX in (W4A4_MXFP4, W4A16_MXFP4):
        layer = moe.MoEFFN(gu, dn, [(MX, MX), (MX, MX)], num_routed=2)
        v = layer.a8_view()
        assert v.fuse_silu == layer.fuse_silu and v.tag1 == v.tag2 == [moe.ACT_MXFP8] * 2
        assert all(q == (_q(), _q()) for q in v.qcfg)
        for a, b in zip(layer.w1 + layer.w2, v.w1 + v.w2):
            assert b.q == _q() and a.B.data_ptr() == b.B.data_ptr() and a.scale_b.data_ptr() == b.scale_b.data_ptr()
        assert all(w.q == MX for w in layer.w1 + layer.w2)  # the source layer is untouched
    with pytest.raises(ValueError, match="a8_view"):
        moe.MoEFFN(gu, dn, [(W4A4_MXFP4,) * 2, (W8A8, W8A8)], num_routed=2).a8_view()
    with pytest.raises(ValueError, match="a8_view"):
        moe.MoEFFN(gu, dn, [(W4A4_MXFP4,) * 2, (W4A16_MXFP4,) * 2], num_routed=2).a8_view()
    # the type given directly: the layer fuses the SiLU epilogue (interleaved gate_up weights)
    direct = moe.MoEFFN(gu, dn, [(_q(), _q())] * 2, num_routed=2)
    assert direct.fuse_silu and direct.tag1 == [moe.ACT_MXFP8] * 2
    plain = moe.MoEFFN(gu, dn, [(W4A4_MXFP4,) * 2] * 2, num_routed=2).a8_view()
    idx = torch.arange(64).view(2, 2, 16).transpose(0, 1).reshape(-1)
    assert torch.equal(direct.w1[0].B, plain.w1[0].B[idx]) and torch.equal(direct.w2[0].B, plain.w2[0].B)
