"""w6a6_g32_sym_MXFP6 on the host: the e2m3 quantiser rule, the device image, the qcfg plumbing, the planner's
validation and the activation entries' tag mask (no GPU)."""
import ctypes

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import SUPPORTED, W6A6_MXFP6, QParams

QCFG = "w6a6_g32_sym_MXFP6"
V2X = "v2x_256x256_w8_b3_buf_spread_edma"
GRID = [m / 8 for m in range(8)] + [2.0 ** (e - 1) * (1 + m / 8) for e in (1, 2, 3) for m in range(8)]


def _codes_of(x):
    c, s = qz.quant_mxfp6(x)
    return qz.unpack_mxfp6_codes(c), s


def test_every_code_survives_a_round_trip():
    codes = torch.arange(64, dtype=torch.uint8).reshape(2, 32)  # a block of positive codes, a block of negative ones
    v = qz.dequant_mxfp6(qz._pack6(codes), torch.full((2, 1), 127, dtype=torch.uint8))
    assert v[0].tolist() == GRID and v[1, 1:].tolist() == [-g for g in GRID[1:]] and torch.signbit(v[1, 0])
    for shift, scale in ((0, 127), (-9, 118)):  # amax 7.5 * 2^shift: e = shift
        got, s = _codes_of((v * 2.0 ** shift).half())
        assert (got == codes).all() and (s == scale).all()


@pytest.mark.parametrize("x,code", [  # ties between neighbours go to the even code; beyond 7.5 saturates
    (0.0625, 0), (0.1875, 2), (1.0625, 8), (1.9375, 16), (2.125, 16), (2.375, 18), (3.875, 24), (4.25, 24), (4.75, 26),
    (7.25, 30), (7.75, 31), (-0.0625, 32), (-0.1875, 34), (-7.75, 63), (-0.0, 32)])
def test_ties_to_even_and_saturation(x, code):
    row = torch.zeros(1, 32, dtype=torch.float16)
    for amax, mul, scale in ((7.5, 1.0, 127), (60000.0, 2.0 ** 13, 140)):  # e = 0 | e = 13 (60000 / 2^13 = 7.32 -> 7.5)
        row[0, 0], row[0, 1] = amax, x * mul
        got, s = _codes_of(row)
        assert s.item() == scale and got[0, 0] == 31 and got[0, 1] == code


def test_zero_and_nonfinite_blocks_and_the_device_image():
    x = torch.zeros(4, 128, dtype=torch.float16)
    x[0, 5] = -0.0
    x[1, 3], x[1, 40] = float("inf"), 1.0
    x[2, 63], x[2, 0] = float("nan"), 2.0
    x[3, 0] = 2.0 ** -24  # the smallest subnormal: e = -26, the element becomes 4
    codes, s = _codes_of(x)
    assert s[:, :2].tolist() == [[0, 0], [255, 125], [126, 255], [101, 0]]
    assert codes[0, 5] == 32 and codes[0].sum() == 32  # -0 keeps its sign under scale code 0
    assert not codes[1, :32].any() and not codes[2, 32:64].any()  # Inf / NaN blocks: zero codes
    assert codes[1, 40] == 24 and codes[2, 0] == 24 and codes[3, 0] == 24
    v = qz.dequant_mxfp6(*qz.quant_mxfp6(x))
    assert torch.isnan(v[1, :32]).all() and torch.isnan(v[2, 32:64]).all() and v[3, 0] == 2.0 ** -24 and v[1, 40] == 1.0
    c = torch.randint(0, 256, (5, 288), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    img = qz.pack_mxfp6(c)
    assert (qz.unpack_mxfp6(img) == c).all()
    blk = c[:, 96 + 48:96 + 72]  # K step 1, block 2: its first 16 bytes at 96 + 32, its last 8 at 96 + 64 + 16
    assert (img[:, 128:144] == blk[:, :16]).all() and (img[:, 176:184] == blk[:, 16:]).all()


def test_qcfg_round_trip_tags_and_weights():
    q = QParams(6, 6, 32, True, "MXFP6")
    assert q == W6A6_MXFP6 and q.qcfg == QCFG and q.fmt_code == nat.FMT_MXFP6 == 6
    assert QParams.from_qcfg(QCFG) == q and SUPPORTED[QCFG] == q
    assert moe.ACT_MXFP6 == 12 and moe.qtag_of(6, 32, "MXFP6") == moe.ACT_MXFP6 == moe.act_tag(q)
    assert moe._BITS[12] == 6 and moe._scale_elems(12, 1408) == 24 and QCFG not in moe.MoEFFN.FUSE_QCFGS
    segs, _, out, _ = moe._make_segments([3, 2], [0, 3], [256, 128], [12, 12], "cpu")
    assert [s.out_off for s in segs] == [0, 3 * 192] and out.numel() == 3 * 192 + 2 * 96
    w = moe.prepare_weight(torch.ones(8, 128, dtype=torch.float16), q)
    w2 = moe.prepare_weight_mx6(*qz.quant_mxfp6(torch.ones(8, 128, dtype=torch.float16)))
    assert w.B.shape == (8, 96) and w.scale_b.shape == (8, 16) and (w2.B == w.B).all() and (w2.scale_b == w.scale_b).all()
    one = torch.ones(256, 128, dtype=torch.float16)
    assert not moe.MoEFFN([one], [one[:128]], [(q, q)], num_routed=1).fuse_silu  # the plain gate_up layout
    with pytest.raises(ValueError, match="fuse_silu"):
        moe.MoEFFN([one], [one[:128]], [(q, q)], num_routed=1, fuse_silu=True)


@pytest.mark.parametrize("kw,variant,status,msg", [
    (dict(), "auto", nat.MXMOE_GG_ERR_WORKSPACE, ""),  # passes validation, stops at the (empty) workspace
    (dict(K=160), V2X, nat.MXMOE_GG_ERR_INVALID, QCFG + " needs K % 128"),
    (dict(scale_a=18), V2X, nat.MXMOE_GG_ERR_INVALID, "MXFP6 scales must be 4-byte aligned"),
    (dict(a_bits=4), V2X, nat.MXMOE_GG_ERR_UNSUPPORTED, QCFG),
    (dict(), "wo3_64x256_w8_3wg", nat.MXMOE_GG_ERR_UNSUPPORTED, "does not implement"),
    (dict(), "v3_256x128_w4_dma_ring3_2wg", nat.MXMOE_GG_ERR_UNSUPPORTED, "does not implement"),
    (dict(fmt=nat.FMT_MXFP6 | nat.EPI_SILU_MUL), V2X, nat.MXMOE_GG_ERR_UNSUPPORTED, "SiLU epilogue"),
])
def test_plan_validation(kw, variant, status, msg):
    d = dict(A=16, B=16, scale_a=16, scale_b=16, C=16, M=64, N=128, K=256, a_bits=6, w_bits=6, gsize=32, sym=1,
             fmt=nat.FMT_MXFP6)
    arr = (nat.GGProblemC * 2)(nat.GGProblemC(**d), nat.GGProblemC(**dict(d, **kw)))
    names = [ln.split()[1] for ln in nat.list_variants()]
    if variant == "auto":
        assert nat.resolve_variant(arr, 2) == names.index(V2X)
    st = nat.lib().mxmoe_gg_plan(arr, 2, nat.VARIANT_AUTO if variant == "auto" else names.index(variant), None, 0, None,
                                 ctypes.byref(nat.GGPlanInfo()))
    err = nat.lib().mxmoe_gg_last_error().decode()
    assert st == status and msg in err, err


def test_tag_mask_bit_12_on_the_three_activation_entries():
    lib = nat.lib()
    glu = nat.MoeGluC(nat.GLU_SILU, 0.0, 0.0, None, None)
    entries = [  # T = 0: the mask is checked, nothing is launched
        lambda m: lib.mxmoe_moe_act_quant(0, None, None, 0, 2, 128, 0, None, None, None, 1, m, None, None, None),
        lambda m: nat.symbol("mxmoe_moe_gather_quant")(nat.DT_BF16, None, 0, 128, 2, 0, None, None, None, 1, m, None, None, None),
        lambda m: nat.symbol("mxmoe_moe_glu_quant")(ctypes.byref(glu), None, None, 0, 2, 128, 0, None, None, 1, m, None, None, None),
    ]
    for call in entries:
        assert call(1 << 12) == nat.MXMOE_GG_OK and call(0x155F) == nat.MXMOE_GG_OK
        assert call(1 << 11) == nat.MXMOE_GG_ERR_UNSUPPORTED and call(1 << 13) == nat.MXMOE_GG_ERR_UNSUPPORTED
