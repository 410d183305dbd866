"""MXFP4 (w4a4_g32_sym_MXFP4) on the host: the e2m1 / e8m0 formats, the RTN quantiser, the scale
layouts, the qcfg plumbing and the C-ABI's validation (no GPU)."""
import ctypes

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import SUPPORTED, W4A4_MXFP4, Problem, QParams
from tests import _mxfp4_ref as ref
from tests._util import assert_f16_close


def _q(x):
    c, s = qz.quant_mxfp4(torch.as_tensor(np.asarray(x, np.float16)))
    return c.numpy(), s.numpy()


def _block(vals, fill=0.0):
    b = np.full((1, 32), fill, np.float16)
    b[0, : len(vals)] = vals
    return b


def test_e8m0_decode_matches_torch():
    codes = torch.arange(255, dtype=torch.uint8)
    want = codes.view(torch.float8_e8m0fnu).to(torch.float64)
    assert torch.equal(qz.e8m0_decode(codes), want)
    assert np.array_equal(ref.e8m0(codes.numpy()), want.numpy())
    nan = torch.tensor([255], dtype=torch.uint8)
    assert torch.isnan(nan.view(torch.float8_e8m0fnu).float()).all()
    assert torch.isnan(qz.e8m0_decode(nan)).all() and np.isnan(ref.e8m0(nan.numpy())).all()


def test_code_table():
    want = [0, .5, 1, 1.5, 2, 3, 4, 6, -0.0, -.5, -1, -1.5, -2, -3, -4, -6]
    codes = torch.tensor([[(2 * i) | ((2 * i + 1) << 4) for i in range(8)] * 2], dtype=torch.uint8)  # nibbles 0..15, twice
    got = qz.dequant_mxfp4(codes, torch.tensor([[127]], dtype=torch.uint8)).numpy()[0]
    assert np.array_equal(got[:16], want) and np.array_equal(np.signbit(got[:16]), np.signbit(want))
    assert np.array_equal(ref.CODE_VALUES, want)
    assert np.array_equal(ref.dequant(codes.numpy(), np.array([[127]], np.uint8))[0][:16], want)


def test_quant_ties_go_to_the_even_code():
    # amax 6 -> e = 0: the elements are their own grid coordinates
    ties = [0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0]
    want = [0.0, 1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 6.0]
    for sign in (1.0, -1.0):
        c, s = _q(_block([sign * t for t in ties]))
        assert s[0, 0] == 127
        got = ref.elements(c)[0, :8]
        assert np.array_equal(got, [sign * w for w in want])
        assert np.array_equal(np.signbit(got), [sign < 0] * 8)  # values that round to 0 keep their sign


def test_quant_saturates():
    c, s = _q(_block([7.5, -7.5, 6.5, 1.0]))
    assert s[0, 0] == 127  # floor(log2 7.5) - 2 = 0
    assert np.array_equal(ref.elements(c)[0, :4], [6.0, -6.0, 6.0, 1.0])


def test_quant_special_blocks():
    c, s = _q(np.zeros((1, 32), np.float16))
    assert s[0, 0] == 0 and not c.any()  # all-zero block: e = -127
    c, s = _q(_block([2.0 ** -24]))  # the smallest fp16 subnormal: e = -26, element = 4
    assert s[0, 0] == 127 - 26 and ref.elements(c)[0, 0] == 4.0
    c, s = _q(_block([65504.0, -65504.0]))  # e = 15 - 2; 65504 / 2^13 = 7.996 -> 6
    assert s[0, 0] == 127 + 13 and np.array_equal(ref.elements(c)[0, :2], [6.0, -6.0])
    c, s = _q(_block([-0.0, 4.0]))
    assert nibbles0(c)[0] == 8 and nibbles0(c)[1] == 6  # -0 keeps its sign
    for bad in (np.nan, np.inf, -np.inf):
        x = np.concatenate([_block([1.0, bad, 3.0]), _block([1.0, 2.0])], axis=1)
        c, s = _q(x)
        assert s[0, 0] == 255 and not c[0, :16].any()  # NaN scale, all-zero codes
        assert s[0, 1] == 126 and np.array_equal(ref.elements(c)[0, 32:34], [2.0, 4.0])  # the next block is untouched


def nibbles0(c):
    return ref.nibbles(c)[0]


def test_quant_scale_formula_power_of_two_sweep():
    for p in range(-24, 16):
        for m in (1.0, 1.5, 1.999):
            amax = np.float16(m * 2.0 ** p)
            if amax == 0 or not np.isfinite(amax):
                continue
            c, s = _q(_block([amax]))
            want_e = int(np.floor(np.log2(float(amax)))) - 2
            assert s[0, 0] == want_e + 127, (p, m)


def test_quant_matches_the_restatement():
    rng = np.random.default_rng(0)
    x = (rng.standard_normal((6, 128)) * np.exp2(rng.integers(-20, 12, (6, 1)))).astype(np.float16)
    x[2, 32:64] = 0
    x[3, 5] = -0.0
    c, s = _q(x)
    rc, rs = ref.quant(x)
    assert np.array_equal(c, rc) and np.array_equal(s, rs)


def test_dequant_quant_is_idempotent():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal((8, 96)) * np.exp2(rng.integers(-16, 10, (8, 3)).repeat(32, axis=1))).astype(np.float16)
    c, s = qz.quant_mxfp4(torch.as_tensor(x))
    d = qz.dequant_mxfp4(c, s)
    assert torch.equal(d.half().double(), d)  # representable in fp16
    c2, s2 = qz.quant_mxfp4(d.half())
    assert torch.equal(c, c2) and torch.equal(s, s2)
    assert np.array_equal(d.numpy(), ref.dequant(c.numpy(), s.numpy()))


@pytest.mark.parametrize("K", [32, 96, 512, 544, 1408, 2048])
def test_scale_pack_round_trip(K):
    nb = K // 32
    rng = np.random.default_rng(K)
    s = torch.as_tensor(rng.integers(0, 255, (5, nb), dtype=np.uint8))
    dev = qz.pack_mxfp4_scales(s)
    G = (nb + 15) // 16
    assert dev.shape == (5, 16 * G) and dev.dtype == torch.uint8
    assert np.array_equal(dev.numpy(), ref.pack_scales(s.numpy()))
    assert torch.equal(qz.unpack_mxfp4_scales(dev, K), s)
    # the pads (blocks past K/32) are 2^0, never NaN
    canon = dev.reshape(5, G, 4, 4).transpose(2, 3).reshape(5, 16 * G)
    assert (canon[:, nb:] == 127).all()


def test_scale_pack_layout_example():
    s = torch.arange(16, dtype=torch.uint8)[None]
    assert qz.pack_mxfp4_scales(s)[0].tolist() == [0, 4, 8, 12, 1, 5, 9, 13, 2, 6, 10, 14, 3, 7, 11, 15]


def test_qcfg_round_trip():
    q = QParams(4, 4, 32, True, fmt="MXFP4")
    assert q == W4A4_MXFP4 and q.qcfg == "w4a4_g32_sym_MXFP4" and q.fmt_code == nat.FMT_MXFP4 == 4
    assert QParams.from_qcfg(q.qcfg) == q and SUPPORTED[q.qcfg] == q
    assert QParams.from_qcfg("w4a4_g-1_sym").fmt == ""


def test_problem_validation():
    z8, zh = torch.zeros(64, 16, dtype=torch.uint8), torch.zeros(64, 64, dtype=torch.float16)
    sc = torch.zeros(64, 16, dtype=torch.uint8)
    Problem(z8, z8, zh, 64, 64, 32, W4A4_MXFP4, sc, sc)
    with pytest.raises(ValueError, match="multiple of the 32-element"):
        Problem(z8, z8, zh, 64, 64, 48, W4A4_MXFP4, sc, sc)
    with pytest.raises(ValueError, match="scale_a"):
        Problem(z8, z8, zh, 64, 64, 32, W4A4_MXFP4, sc.half(), sc)


def _prob(**kw):
    d = dict(A=16, B=16, scale_a=16, scale_b=16, C=16, M=64, N=128, K=256, a_bits=4, w_bits=4, gsize=32, sym=1,
             fmt=nat.FMT_MXFP4)
    d.update(kw)
    return nat.GGProblemC(**d)


def _plan(problems, variant, ws_bytes=1 << 20):
    arr = (nat.GGProblemC * len(problems))(*problems)
    info = nat.GGPlanInfo()
    st = nat.lib().mxmoe_gg_plan(arr, len(problems), variant, None, ws_bytes, None, ctypes.byref(info))
    return st, nat.lib().mxmoe_gg_last_error().decode()


def test_plan_accepts_mxfp4():
    st, err = _plan([_prob()], nat.default_variant(), ws_bytes=0)
    assert st == nat.MXMOE_GG_ERR_WORKSPACE, err  # passed validation, stopped at the workspace check
    st, err = _plan([_prob(K=1408), _prob(K=32)], nat.VARIANT_AUTO, ws_bytes=0)
    assert st == nat.MXMOE_GG_ERR_WORKSPACE, err


@pytest.mark.parametrize("kw,status,msg", [
    (dict(gsize=-1), nat.MXMOE_GG_ERR_UNSUPPORTED, "w4a4_g32_sym_MXFP4"),
    (dict(a_bits=8), nat.MXMOE_GG_ERR_UNSUPPORTED, "w4a4_g32_sym_MXFP4"),
    (dict(K=48), nat.MXMOE_GG_ERR_INVALID, "multiple of 32"),
    (dict(scale_a=0), nat.MXMOE_GG_ERR_INVALID, "NULL scale"),
    (dict(scale_b=0), nat.MXMOE_GG_ERR_INVALID, "NULL scale"),
    (dict(scale_b=18), nat.MXMOE_GG_ERR_INVALID, "4-byte aligned"),
    (dict(fmt=nat.FMT_MXFP4 | nat.EPI_SILU_MUL), nat.MXMOE_GG_ERR_UNSUPPORTED, "SiLU epilogue"),
])
def test_plan_validation(kw, status, msg):
    st, err = _plan([_prob(), _prob(**kw)], nat.default_variant())
    assert st == status, err
    assert msg in err and "problem 1" in err


def test_forced_small_kernels_do_not_implement_mxfp4():
    names = [ln.split()[1] for ln in nat.list_variants()]
    for name in ("v3_256x128_w4_dma_ring3_2wg", "wo3_64x256_w8_3wg"):
        st, err = _plan([_prob()], names.index(name))
        assert st == nat.MXMOE_GG_ERR_UNSUPPORTED and "does not implement" in err, (name, err)


def test_auto_sends_mxfp4_to_v2x_at_every_batch_size():
    w8 = nat.GGProblemC(A=16, B=16, scale_a=16, scale_b=16, C=16, M=8, N=128, K=256, a_bits=8, w_bits=8, gsize=-1, sym=1)
    for M in (8, 64, 4096):
        for probs in ([_prob(M=M)], [_prob(M=M), w8], [w8, _prob(M=M, K=5632)]):
            arr = (nat.GGProblemC * len(probs))(*probs)
            assert nat.resolve_variant(arr, len(probs)) == nat.default_variant()
    assert nat.variant_supports(nat.default_variant(), "w4a4_g32_sym_MXFP4")
    # an EMPTY MXFP4 problem beside small w8a8 ones still counts: the call plans on v2x, not on wo3
    probs = [_prob(M=0), w8]
    arr = (nat.GGProblemC * 2)(*probs)
    assert nat.resolve_variant(arr, 2) == nat.default_variant()
    st, err = _plan(probs, nat.VARIANT_AUTO, ws_bytes=0)
    assert st == nat.MXMOE_GG_ERR_WORKSPACE, err


def test_abi_version_is_still_7():
    assert nat.lib().mxmoe_gg_abi_version() == 7


def test_blockwise_f32_accumulation_is_within_tolerance():
    """The kernel's arithmetic (f32 accumulation block by block) against the f64 reference at K = 2048."""
    rng = np.random.default_rng(2)
    K = 2048
    a = rng.standard_normal((24, K)).astype(np.float16)
    b = (0.05 * rng.standard_normal((40, K))).astype(np.float16)
    ac, asc = _q(a)
    bc, bsc = _q(b)
    want = ref.gemm(ac, asc, bc, bsc)
    got = ref.gemm_f32_blockwise(ac, asc, bc, bsc).astype(np.float16)
    assert_f16_close(got, want, K)


def test_qtag_of_mxfp4():
    from mxmoe_amd import moe

    assert moe.qtag_of(4, 32) == moe.ACT_MXFP4 == 4
    assert moe._BITS[moe.ACT_MXFP4] == 4


def test_segment_scale_accounting():
    """An MXFP4 segment's scale block is rows x 16 G bytes at an even fp16-element offset."""
    from mxmoe_amd import moe

    segs, _, out, scales = moe._make_segments([3, 5, 2], [0, 3, 8], [128, 1408, 128],
                                              [moe.ACT_INT8, moe.ACT_MXFP4, moe.ACT_INT8], "cpu")
    assert [s.scale_off for s in segs] == [0, 4, 4 + 5 * 48 // 2]  # 3 -> 4: aligned; 1408 / 32 = 44 blocks -> 48 bytes
    assert scales.numel() == 4 + 120 + 2
    b = moe.ActBatch(out, scales, segs, [moe.ACT_INT8, moe.ACT_MXFP4, moe.ACT_INT8])
    assert b.scale(1).dtype == torch.uint8 and b.scale(1).shape == (5, 48)
    assert b.A(1).shape == (5, 704)


def test_cli_plumbing_on_the_host():
    """--qstr parsing, the layer-input builder and the CLI's CPU reference, on a CPU tensor set."""
    from mxmoe_amd.check import expected_sample
    from mxmoe_amd.harness import build_layer_inputs
    from mxmoe_amd.workload import QShape, parse_qstr

    assert parse_qstr("w4a4_g32_sym_MXFP4") == dict(w_bits=4, a_bits=4, gsize=32, sym=True, fmt="MXFP4")
    s = QShape([5, 16, 96], **parse_qstr("w4a4_g32_sym_MXFP4"))
    assert s.qcfg == "w4a4_g32_sym_MXFP4" and QShape.from_json(s.to_json()) == s
    p = build_layer_inputs([s], device="cpu", seed=3).problems[0]
    assert p.A.shape == (5, 48) and p.scale_a.shape == (5, 16) and p.scale_b.shape == (16, 16)
    rows, cols = torch.arange(5), torch.tensor([0, 3, 15])
    want, exact = expected_sample(p, rows, cols)
    a = ref.dequant(p.A.numpy(), qz.unpack_mxfp4_scales(p.scale_a, 96).numpy())
    b = ref.dequant(p.B.numpy(), qz.unpack_mxfp4_scales(p.scale_b, 96).numpy())
    assert not exact and np.array_equal(want.numpy(), (a @ b.T)[:, [0, 3, 15]])


def test_act_quant_entry_validation():
    """mxmoe_moe_act_quant: the named entry points' checks, plus the mode and the tag mask."""
    fn = nat.lib().mxmoe_moe_act_quant
    err = nat.lib().mxmoe_gg_last_error
    for mode in range(4):
        assert fn(mode, None, None, 4, 2, 100, 0, None, None, None, 1, 1 << 4, None, None, None) == nat.MXMOE_GG_ERR_INVALID
        assert b"128" in err()
        assert fn(mode, None, None, 4, 2, 128, 0, None, None, None, 1, 1 << 4, None, None, None) == nat.MXMOE_GG_ERR_INVALID
        assert b"NULL or misaligned" in err()
        assert fn(mode, None, None, 0, 2, 128, 0, None, None, None, 1, 0x1F, None, None, None) == nat.MXMOE_GG_OK  # T = 0
    assert fn(4, None, None, 0, 2, 128, 0, None, None, None, 1, 1, None, None, None) == nat.MXMOE_GG_ERR_INVALID
    assert fn(0, None, None, 0, 2, 128, 0, None, None, None, 1, 1 << 5, None, None, None) == nat.MXMOE_GG_ERR_UNSUPPORTED
    assert b"unknown activation tag" in err()


def test_tag_mask():
    from mxmoe_amd import moe

    assert moe._tag_mask([moe.ACT_INT8, moe.ACT_MXFP4, moe.ACT_INT8]) == 0b10010
