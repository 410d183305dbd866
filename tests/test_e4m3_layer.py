"""FP8 MoE layers on the host (no GPU): the numpy reference of the per-token e4m3 activation tag against the oracle,
the kernel's replacement for the f32 division checked exhaustively against the division, the C-ABI's tag mask and
segment sizes, the tag tables, the weight preparation and what the layer classes make of w8a8_g-1_sym_E4M3 experts."""
import warnings

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import FP16, W4A4, W8A8, W8A8_E4M3
from oracle import oracle
from tests import _e4m3_layer_ref as ref
from tests._decode_util import cpu_ffn

QCFG = "w8a8_g-1_sym_E4M3"


# ------------------------------------------------------------------ the reference quantiser and the division

def _finite_rows():
    """Every edge row the GPU file feeds to the quantiser (tests/test_e4m3_layer_gpu.py draws them with these
    arguments), random rows over 30 binades among them."""
    rows = [ref.edge_rows(W, seed, tail=tail) for W in (128, 640, 1024, 2176) for seed in (0, 1, 2)
            for tail in (False, True)]
    rows.append(ref.edge_rows(16384, 1))
    # and as the bf16 gather sees them: rounded to bf16, kept inside fp16's range, converted back
    rows += [torch.from_numpy(x).to(torch.bfloat16).clamp(-65280, 65280).to(torch.float16).numpy() for x in list(rows)]
    return rows


def test_reference_equals_the_oracle_on_every_finite_edge_row():
    n = 0
    for x in _finite_rows():
        codes, sbits = ref.quant(x)
        oc, os_ = oracle.quant_e4m3(x)
        assert np.array_equal(sbits, os_.view(np.uint16)), x.shape
        assert np.array_equal(codes, oc), x.shape
        tc, ts = qz.quant_e4m3(torch.from_numpy(x))
        assert np.array_equal(codes, tc.numpy()) and np.array_equal(sbits, ts.numpy().view(np.uint16))
        n += x.shape[0]
    assert n >= 100
    # what the rows are there for
    x = ref.edge_rows(128)
    codes, sbits = ref.quant(x)
    k = {name: i for i, name in enumerate(ref.EDGE_KINDS)}
    assert sbits[k["zero"]] == 0x3C00 and not codes[k["zero"]].any()
    assert sbits[k["lone_tiny"]] == 0x0400 and not codes[k["lone_tiny"]].any()  # 2^-10: the tie goes to 0
    assert codes[k["amax_max"], 0] == 0x7E and codes[k["amax_max"], 1] == 0xFE
    t = codes[k["ties"]]
    assert sbits[k["ties"]] == 0x3C00 and list(t[:8]) == [0x7E, 0x58, 0x5A, 0xD8, 0x80, 0x00, 0x02, 0x7E]
    for name, down in (("scale_down", True), ("scale_up", False)):
        a = ref.scale_rounding_amax(down)
        s = np.array([sbits[k[name]]], np.uint16).view(np.float16)[0]
        assert (float(a) / float(s) > 448) == down and codes[k[name], 0] == 0x7E and codes[k[name], 1] == 0xFE


def test_reference_non_finite_rows():
    x = ref.edge_rows(128)
    x[2, 5], x[4, 127], x[7, 0] = np.inf, np.nan, -np.inf
    codes, sbits = ref.quant(x)
    want_c, want_s = ref.quant(ref.edge_rows(128))
    for r in range(x.shape[0]):
        if r in (2, 4, 7):
            assert sbits[r] == ref.NAN_SCALE and not codes[r].any()
        else:
            assert sbits[r] == want_s[r] and np.array_equal(codes[r], want_c[r])


def test_pack_is_pack_e4m3():
    codes = np.arange(256, dtype=np.uint8).reshape(2, 128)
    assert np.array_equal(ref.pack(codes), qz.pack_e4m3(torch.from_numpy(codes)).numpy().view(np.uint8))


def test_kernel_quotient_gives_the_divisions_codes_for_every_significand_pair():
    """The kernel computes q' = q + (x - q s) r (r the correctly rounded 1 / s, q = x r) where the tag's rule has the
    correctly rounded f32 quotient. Both sequences commute with scaling x or s by a power of two (no intermediate
    leaves the normal f32 range: |x| in [2^-24, 65504], s in [2^-14, 146.25]), and so do e4m3's rounding points up to
    the exponent: a point where the code changes — a grid midpoint, a binade's end, the clamp at 448, the subnormal
    grid's midpoints — is a value of at most 5 significant bits. So the codes agree for every fp16 x and every
    normal fp16 s if, for every pair of 11-bit significands, q' and the quotient are the same f32 or lie strictly
    inside the same cell of the 5-significant-bit grid. All 1024 x 1024 pairs are checked."""
    m = (1024 + np.arange(1024, dtype=np.float32)) / np.float32(1024)
    x, s = np.meshgrid(m, m, indexing="ij")
    qk, qd = ref.kernel_quotient(x, s), (x / s).astype(np.float32)

    def cell(v):
        f, ex = np.frexp(v.astype(np.float64))
        t = f * 32  # [16, 32): 5 significant bits
        return ex, np.floor(t), t == np.floor(t)

    (ek, ck, gk), (ed, cd, gd) = cell(qk), cell(qd)
    same_cell = (ek == ed) & (ck == cd) & ~gk & ~gd
    assert ((qk == qd) | same_cell).all()
    # where the quotient is a grid value (the exact cases) the sequence returns it exactly
    assert np.array_equal(qk[gd], qd[gd]) and gd.sum() >= 1024


def test_kernel_quotient_codes_on_real_operands():
    """The same check without the scaling argument, on the codes themselves: every finite fp16 dividend (both zeros
    and the subnormals included) against divisors from every binade a scale can lie in, 2^-14 up to fp16(65504 / 448)."""
    x = np.arange(0x10000, dtype=np.uint32).astype(np.uint16).view(np.float16)
    x = x[np.isfinite(x)].astype(np.float32)
    mant = np.array([0, 1, 341, 1023], np.uint16)
    sb = np.concatenate([(np.uint16(e << 10) | mant) for e in range(1, 23)]).astype(np.uint16)
    top = (np.float32(65504) / np.float32(448)).astype(np.float16)
    s = np.concatenate([sb.view(np.float16), [top]]).astype(np.float16)
    s = s[s <= top].astype(np.float32)
    assert s.min() == 2.0 ** -14 and s.max() == 146.25
    for sv in s:
        qk = ref.kernel_quotient(x, np.full_like(x, sv))
        qd = (x / sv).astype(np.float32)
        assert np.array_equal(np.signbit(qk), np.signbit(x))  # -0 stays -0
        assert np.array_equal(ref.e4m3_rn_sat(qk), ref.e4m3_rn_sat(qd)), sv


# ------------------------------------------------------------------ the C-ABI: tag mask and segments

def _entries():
    lib = nat.lib()
    glu = nat.MoeGluC(nat.GLU_SILU, 0.0, 0.0, None, None)
    import ctypes
    return {
        "mxmoe_moe_act_quant": lambda mask: lib.mxmoe_moe_act_quant(0, None, None, 0, 2, 128, 0, None, None, None, 1, mask,
                                                                    None, None, None),
        "mxmoe_moe_gather_quant": lambda mask: nat.symbol("mxmoe_moe_gather_quant")(nat.DT_BF16, None, 0, 128, 2, 0, None,
                                                                                    None, None, 1, mask, None, None, None),
        "mxmoe_moe_glu_quant": lambda mask: nat.symbol("mxmoe_moe_glu_quant")(ctypes.byref(glu), None, None, 0, 2, 128, 0,
                                                                              None, None, 1, mask, None, None, None),
    }


def test_tag_mask_on_the_three_entries():
    err = nat.lib().mxmoe_gg_last_error
    for name, call in _entries().items():
        for mask in (1 << 8, 0x15F):  # T = 0: checked and accepted
            assert call(mask) == nat.MXMOE_GG_OK, (name, mask, err())
        for mask in (1 << 5, 1 << 7, 1 << 9, (1 << 8) | (1 << 7)):
            assert call(mask) == nat.MXMOE_GG_ERR_UNSUPPORTED, (name, mask)
            assert b"unknown activation tag" in err() and name.encode() in err()
    assert nat.lib().mxmoe_gg_abi_version() == 7


@pytest.mark.parametrize("shared", [True, False])
def test_segments_host_equals_make_segments(shared):
    F, I8, E8, M8 = moe.ACT_FP16, moe.ACT_INT8, moe.ACT_E4M3, moe.ACT_MXFP8
    tags = [E8, F, I8, E8, M8, E8, I8] + ([E8] if shared else [])
    counts = [3, 2, 0, 5, 1, 0, 7]
    T, topk, W, Ws, ldc = 9, 2, 640, 2176, 1280
    first = list(np.cumsum([0] + counts[:-1]))
    rows = counts + ([T] if shared else [])
    want, _, out, scales = moe._make_segments(rows, first + ([T * topk] if shared else []),
                                              [W] * len(counts) + ([Ws] if shared else []), tags, "cpu")
    segs, dyn, status = nat.segments_host(counts, T, topk, tags, W, Ws if shared else 0, ldc)
    assert status == 0
    for f, _ in nat.MoeSegC._fields_:
        assert [getattr(s, f) for s in segs] == [getattr(s, f) for s in want], f
    assert [(d.rows, d.a_off, d.sa_off) for d in dyn] == [(s.rows, s.out_off, 2 * s.scale_off) for s in want]
    # an E4M3 segment: one byte per element and one fp16 scale per row, as an INT8 one
    assert segs[1].out_off - segs[0].out_off == 3 * W and segs[1].scale_off - segs[0].scale_off == 3
    assert segs[4].out_off - segs[3].out_off == 5 * W and segs[4].scale_off - segs[3].scale_off == 5
    last = segs[-1]
    assert out.numel() == last.out_off + -(-(last.rows * last.width) // 16) * 16
    assert scales.numel() == last.scale_off + last.rows


# ------------------------------------------------------------------ the tag tables, the weights, the layer classes

def test_qtag_of_both_forms():
    assert moe.ACT_E4M3 == 8 and moe._BITS[8] == 8 and moe._scale_elems(8, 640) == 1
    assert moe.qtag_of(8, -1, "E4M3") == moe.ACT_E4M3
    assert moe.qtag_of(8, -1) == moe.qtag_of(8, -1, "") == moe.ACT_INT8
    q = W8A8_E4M3
    assert q.qcfg == QCFG and moe.qtag_of(q.a_bits, q.gsize, q.fmt) == 8
    # every other type is what it was, with or without its fmt
    for a, g, fmt, tag in ((16, -1, "", 0), (16, -1, "bf16", 0), (4, -1, "", 2), (4, 128, "", 3), (4, 32, "MXFP4", 4),
                           (8, 32, "MXFP8", 6), (16, 32, "MXFP4", 0)):
        assert moe.qtag_of(a, g) == moe.qtag_of(a, g, fmt) == tag
    with pytest.raises(ValueError):
        moe.qtag_of(8, 128, "E4M3")
    assert moe._tag_mask([8, 1, 8, 6]) == 0x142


def test_prepare_weight_and_prepare_weight_e4m3():
    g = torch.Generator().manual_seed(3)
    w = (torch.randn(48, 256, generator=g) * torch.exp2(torch.randint(-6, 3, (48, 1), generator=g).float())).half()
    w[5] = 0
    pw = moe.prepare_weight(w, W8A8_E4M3)
    oc, os_ = oracle.quant_e4m3(w.numpy())
    assert pw.q == W8A8_E4M3 and (pw.N, pw.K) == (48, 256) and pw.scale_out_of_range == 0
    assert pw.B.dtype == torch.uint8 and np.array_equal(pw.B.numpy(), ref.pack(oc))
    assert pw.scale_b.dtype == torch.float16 and np.array_equal(pw.scale_b.numpy().view(np.uint16), os_.view(np.uint16))
    # weights that already are FP8: the same operand from the logical codes and the scales, nothing requantised
    codes = torch.from_numpy(oc)
    for c, s in ((codes, pw.scale_b), (codes.view(torch.float8_e4m3fn), pw.scale_b.float()),
                 (codes, pw.scale_b.float().view(48, 1))):
        with warnings.catch_warnings():
            warnings.simplefilter("error")
            e = moe.prepare_weight_e4m3(c, s)
        assert torch.equal(e.B, pw.B) and torch.equal(e.scale_b, pw.scale_b) and e.q == W8A8_E4M3
        assert (e.N, e.K, e.scale_out_of_range) == (48, 256, 0)
    # interleaved rows (the fused layout is not E4M3's, but prepare_weight's row order is the same for every type)
    wi = moe.prepare_weight(w[:32], W8A8_E4M3, interleave=True)
    assert torch.equal(wi.B, pw.B[:32][torch.arange(32).view(2, 1, 16).transpose(0, 1).reshape(-1)])
    # f32 scales that fp16 cannot hold: counted, and warned about once
    s32 = pw.scale_b.float().clone()
    s32[0] *= 1 + 2.0 ** -13  # rounds to another value
    s32[1] = 2.0 ** -20       # subnormal as fp16
    s32[2] = 1.0e6            # beyond 65504
    with pytest.warns(UserWarning, match="3 of 48 scales") as rec:
        e = moe.prepare_weight_e4m3(codes, s32)
    assert len(rec) == 1 and e.scale_out_of_range == 3 and torch.equal(e.scale_b[3:], pw.scale_b[3:])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert moe.prepare_weight_e4m3(codes, s32, warn=False).scale_out_of_range == 3
    for bad_c, bad_s in ((codes.to(torch.int8), pw.scale_b), (codes, pw.scale_b[:47]), (codes, pw.scale_b.double()),
                         (codes[:, :255], pw.scale_b)):
        with pytest.raises(ValueError, match="prepare_weight_e4m3"):
            moe.prepare_weight_e4m3(bad_c, bad_s)


def test_layer_classes():
    E8 = W8A8_E4M3
    ffn = cpu_ffn([(E8, E8)] * 3)
    assert ffn.tag1 == ffn.tag2 == [8, 8, 8] and ffn.fuse_silu is False and ffn.gate_up_layout() == "plain"
    assert all(w.q == E8 and w.B.dtype == torch.uint8 and w.scale_b.dtype == torch.float16 for w in ffn.w1 + ffn.w2)
    with pytest.raises(ValueError, match="fuse_silu"):
        cpu_ffn([(E8, E8)] * 3, fuse_silu=True)
    with pytest.raises(ValueError, match="fuse_silu"):  # one E4M3 gate_up is enough
        cpu_ffn([(W8A8, W8A8), (E8, W8A8), (W8A8, W8A8)], fuse_silu=True)
    mixed = cpu_ffn([(E8, W8A8), (W8A8, E8), (FP16, W4A4)])
    assert mixed.tag1 == [8, 1, 0] and mixed.tag2 == [1, 8, 2] and mixed.fuse_silu is False
    fused = cpu_ffn([(W8A8, E8), (W8A8, E8), (FP16, E8)])  # E4M3 down projections alone keep the epilogue
    assert fused.fuse_silu is True and fused.tag2 == [8, 8, 8]
    # prepared FP8 weights go in as they are
    w1 = [moe.prepare_weight_e4m3(w.B.view(-1, 2).flip(1).reshape(w.B.shape), w.scale_b) for w in ffn.w1]
    again = moe.MoEFFN(w1, ffn.w2, [(E8, E8)] * 3, num_routed=2)
    assert all(torch.equal(a.B, b.B) for a, b in zip(again.w1, ffn.w1)) and again.tag1 == [8, 8, 8]
    for cls in (moe.DecodeForward, moe.DecodeForwardEx, moe.DecodeForwardWo):
        with pytest.raises(ValueError, match=QCFG.replace("-", r"\-")):
            cls(ffn, 4, 2, device="cpu")
        with pytest.raises(ValueError, match=QCFG.replace("-", r"\-")):
            cls(mixed, 4, 2, device="cpu")
