"""The decode forward with integer weight-only experts without a GPU (mxmoe_moe_decode_gate_up_wo,
mxmoe_moe_decode_down_wo; moe.DecodeForwardWo): the C ABI's host validation (dummy pointers, every refusal made before
any HIP call and reported under the entry's name), DecodeForwardWo's constructor on CPU-built layers, and the
K -> (lane, step, run) and K -> LDS-byte maps the weight-only kernel body hard-codes, restated in plain Python."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe, quantize
from mxmoe_amd.groupgemm import (FP16, W2A16_G128_ASYM, W4A4, W4A4_G128, W4A4_MXFP4, W4A8_MXFP8, W4A16_ASYM,
                                 W4A16_G128_SYM, W8A8, W8A16_ASYM, QParams)
from tests._decode_util import cpu_ffn, entry_down, entry_gate_up, err

INVALID, UNSUPPORTED, OK = nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_OK
ALL_KINDS = (1 << 12) - 1
ROOT = Path(__file__).resolve().parent.parent
NAMES = {4: "W4A16", 5: "W8A16", 6: "W4A16_G128", 7: "W8A16_G128", 8: "W4A16_ASYM", 9: "W8A16_ASYM",
         10: "W4A16_G128_ASYM", 11: "W8A16_G128_ASYM"}


def _gate_up(**kw):
    return entry_gate_up("wo", **dict(dict(mask=ALL_KINDS), **kw))


def _down(**kw):
    return entry_down("wo", **dict(dict(mask=ALL_KINDS), **kw))


ENTRIES = [(_gate_up, b"mxmoe_moe_decode_gate_up_wo"), (_down, b"mxmoe_moe_decode_down_wo")]


def test_abi_symbols_and_constants():
    """The two entries are exported, declared and bound; ABI 7; the record is still 40 bytes; the eight kinds are
    4 + (w_bits == 8) + 2 * (gsize == 128) + 4 * asym, in the binding, in the header and in DecodeForwardWo.KINDS."""
    lib = nat.lib()
    assert lib.mxmoe_gg_abi_version() == 7 == nat.ABI_VERSION  # additive: no version bump
    assert nat.DECODE_WO_SYMBOLS == ("mxmoe_moe_decode_gate_up_wo", "mxmoe_moe_decode_down_wo")
    header = (ROOT / "include" / "mxmoe_moe.h").read_text()
    declared = set(re.findall(r"^int (mxmoe_moe_\w+)\(", header, flags=re.M))
    for fn in nat.DECODE_WO_SYMBOLS:
        assert fn in nat.EXPORTED_SYMBOLS and hasattr(lib, fn) and fn in declared
    assert declared <= set(nat.EXPORTED_SYMBOLS)
    assert ctypes.sizeof(nat.MoeDecodeExpertC) == 40
    assert lib.mxmoe_moe_decode_gate_up_wo.argtypes == lib.mxmoe_moe_decode_gate_up_ex.argtypes
    assert lib.mxmoe_moe_decode_down_wo.argtypes == lib.mxmoe_moe_decode_down_ex.argtypes
    seen = set()
    for bits in (4, 8):
        for gsize in (-1, 128):
            for sym in (True, False):
                kind = 4 + (bits == 8) + 2 * (gsize == 128) + 4 * (not sym)
                seen.add(kind)
                assert nat.decode_wo_kind(bits, gsize, sym) == kind == getattr(nat, "DECODE_" + NAMES[kind])
                assert re.search(rf"\bMXMOE_DECODE_{NAMES[kind]} = {kind}\b", header), kind
                qcfg = QParams(16, bits, gsize, sym).qcfg
                assert moe.DecodeForwardWo.KINDS[qcfg] == kind
                assert qcfg not in moe.DecodeForwardEx.KINDS and qcfg not in moe.DecodeForward.KINDS
    assert seen == set(range(4, 12))
    assert {k: v for k, v in moe.DecodeForwardWo.KINDS.items() if v < 4} == moe.DecodeForwardEx.KINDS
    assert moe.DecodeForwardWo.ENTRIES == nat.DECODE_WO_SYMBOLS and moe.DecodeForwardWo.TAKES_GLU
    with pytest.raises(ValueError):
        nat.decode_wo_kind(2, 128, False)
    with pytest.raises(ValueError):
        nat.decode_wo_kind(4, 64, True)


@pytest.mark.parametrize("call,name", ENTRIES)
def test_limits_are_refused_before_any_hip_call(call, name):
    """Everything the _ex entries check, under the _wo entry's name; T = 0 is OK with no launch."""
    for kw in (dict(T=17), dict(T=-1), dict(H=192), dict(H=0), dict(H=16384 + 128), dict(N=100), dict(Ns=200), dict(Ns=0),
               dict(topk=0), dict(topk=17, E=32), dict(topk=5, E=4), dict(E=0), dict(act=8), dict(act_shared=24),
               dict(ids=2), dict(experts=4), dict(status=2), dict(mask=0), dict(ids=None), dict(experts=None),
               dict(act=None), dict(act_shared=None)):
        assert call(**kw) == INVALID, kw
        assert name in err(), kw
    assert call(T=0) == OK
    assert call(T=0, with_shared=0, Ns=0, act_shared=None) == OK
    assert call(T=0, H=16384, N=16384, Ns=16384, topk=16, E=16) == OK


@pytest.mark.parametrize("call,name", ENTRIES)
def test_kind_bits(call, name):
    """Kind bits 0 to 11 are kinds here; bit 12 and above is MXMOE_GG_ERR_UNSUPPORTED, also for an empty batch; an
    empty mask is MXMOE_GG_ERR_INVALID. The four older entries refuse what they refused."""
    for mask in [1 << k for k in range(12)] + [ALL_KINDS, 0b100100010011]:
        assert call(mask=mask, T=0) == OK, mask
    for mask in (1 << 12, ALL_KINDS | 1 << 12, 1 << 31):
        assert call(mask=mask) == UNSUPPORTED, mask
        assert name in err() and b"kind" in err()
        assert call(mask=mask, T=0) == UNSUPPORTED
    assert call(mask=0, T=0) == INVALID and name in err()
    ex = nat.symbol("mxmoe_moe_decode_down_ex")
    first = nat.symbol("mxmoe_moe_decode_down")
    args = (0, 2, 4, 1, 16, 16)
    tail = (256, 128, 256, 16, 16, 16, 16, None, None)
    assert ex(*args, 1 << 4, *tail) == UNSUPPORTED and ex(*args, 1 << 3, *tail) == OK
    assert first(*args, 1 << 3, *tail) == UNSUPPORTED and first(*args, 0b111, *tail) == OK


def test_entry_specific_refusals():
    """gate_up_wo: dtype, layout, hidden and the glu checks; down_wo: y / ys."""
    import math

    name = b"mxmoe_moe_decode_gate_up_wo"
    glu = lambda act=nat.GLU_SWIGLU_CLAMP, alpha=1.702, limit=7.0, bias_routed=32, bias_shared=64: \
        nat.MoeGluC(act, alpha, limit, bias_routed, bias_shared)
    for kw in (dict(dtype=2), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(hidden=8), dict(hidden=None)):
        assert _gate_up(**kw) == INVALID, kw
        assert name in err(), kw
    for g in (glu(act=2), glu(act=-1), glu(alpha=math.inf), glu(alpha=math.nan), glu(limit=0.0), glu(limit=-1.0),
              glu(limit=math.inf), glu(limit=math.nan), glu(bias_routed=8), glu(bias_shared=24)):
        assert _gate_up(glu=g) == INVALID
        assert name in err()
        assert _gate_up(glu=g, T=0) == INVALID  # (before the empty-batch return)
    assert _gate_up(glu=glu(), with_shared=0, act_shared=None) == INVALID  # bias_shared without a shared expert
    assert name in err() and b"bias_shared" in err()
    assert _gate_up(glu=glu(), T=0) == OK
    assert _gate_up(glu=None, dtype=nat.DT_BF16, layout=nat.DECODE_GU_INTERLEAVED, T=0) == OK
    for kw in (dict(y=8), dict(ys=4), dict(y=None), dict(ys=None)):
        assert _down(**kw) == INVALID, kw
        assert b"mxmoe_moe_decode_down_wo" in err(), kw
    assert _down(with_shared=0, ys=None, act_shared=None, T=0) == OK


def _record(df, e):
    return nat.MoeDecodeExpertC.from_buffer_copy(bytes(df.experts[40 * e:40 * e + 40].tolist()))


def test_decode_forward_wo_on_cpu_built_layers():
    """DecodeForwardWo constructs for the w4a16_asym + w8a8 scheme (masks, the layer's own tensors in the records, the
    interleaved layout), a g128 sym layer and a biased w8a16 layer; the other two classes refuse those layers."""
    scheme = cpu_ffn([(W4A16_ASYM, W8A8), (W8A8, W4A16_ASYM), (W4A16_ASYM, W4A16_ASYM)])
    df = moe.DecodeForwardWo(scheme, 4, 2)
    both = 1 << nat.DECODE_W8A8 | 1 << nat.DECODE_W4A16_ASYM
    assert df.mask1 == both == df.mask2 and df._glu is None
    assert scheme.fuse_silu and df.layout == nat.DECODE_GU_INTERLEAVED
    assert df.experts.numel() == 40 * 3 and df.act.shape == (8, 128)
    for e, (k1, k2) in enumerate([(8, 1), (1, 8), (8, 8)]):
        rec = _record(df, e)
        w1, w2 = scheme.w1[e], scheme.w2[e]
        assert (rec.b1, rec.sb1, rec.kind1) == (w1.B.data_ptr(), w1.scale_b.data_ptr(), k1)
        assert (rec.b2, rec.sb2, rec.kind2) == (w2.B.data_ptr(), w2.scale_b.data_ptr(), k2)
    assert scheme.w1[0].scale_b.numel() == 256 * 2 and scheme.w2[1].scale_b.numel() == 256 * 2  # [1][rows][2]
    g128 = cpu_ffn([(W4A16_G128_SYM, W4A16_G128_SYM)] * 3)
    df = moe.DecodeForwardWo(g128, 16, 2)
    assert df.mask1 == df.mask2 == 1 << nat.DECODE_W4A16_G128
    assert g128.w1[0].scale_b.numel() == 2 * 256 and g128.w2[0].scale_b.numel() == 1 * 256  # [K / 128][rows]
    biased = cpu_ffn([(W8A16_ASYM, W8A16_ASYM)] * 3, down_bias=[torch.zeros(256) for _ in range(3)])
    df = moe.DecodeForwardWo(biased, 4, 2)
    assert df._glu is not None and df.layout == nat.DECODE_GU_PLAIN
    assert df.mask1 == df.mask2 == 1 << nat.DECODE_W8A16_ASYM
    plain = moe.DecodeForwardWo(cpu_ffn([(W8A8, W4A4), (FP16, W8A8), (W4A4, FP16)]), 4, 2)  # a layer DecodeForward takes
    assert plain.mask1 == 0b111 == plain.mask2 and plain._glu is None
    for cls in (moe.DecodeForward, moe.DecodeForwardEx):
        with pytest.raises(ValueError, match="w4a16_g-1_asym"):
            cls(scheme, 4, 2)
        with pytest.raises(ValueError, match="w4a16_g128_sym"):
            cls(g128, 4, 2)


def test_decode_forward_wo_refusals():
    """w2a16, w4a4_g128_sym, the a4 / a8 MX forms and T = 17 are refused by name; so is a scale buffer of the wrong size."""
    for q, name in ((W2A16_G128_ASYM, "w2a16_g128_asym"), (W4A4_G128, "w4a4_g128_sym"), (W4A4_MXFP4, "w4a4_g32_sym_MXFP4"),
                    (W4A8_MXFP8, "w4a8_g32_sym_MXFP8")):
        with pytest.raises(ValueError, match=name):
            moe.DecodeForwardWo(cpu_ffn([(W8A8, W8A8), (W8A8, q), (W8A8, W8A8)]), 4, 2)
    with pytest.raises(ValueError, match="w4a16_g64_sym"):
        moe.DecodeForwardWo(cpu_ffn([(QParams(16, 4, 64, True), W8A8)] * 3), 4, 2)
    ok = cpu_ffn([(W4A16_ASYM, W4A16_G128_SYM)] * 3)
    with pytest.raises(ValueError, match="T = 17"):
        moe.DecodeForwardWo(ok, 17, 2)
    moe.DecodeForwardWo(ok, 16, 2)
    ok.w2[1].scale_b = ok.w2[1].scale_b[:-1]
    with pytest.raises(ValueError, match="scale buffer"):
        moe.DecodeForwardWo(ok, 16, 2)


# ---- the kernel's maps, in plain Python (mxmoe_amd/csrc/moe_decode.h, "WeightOnly" and "fp16 A") -------------------------
def run_k(bits, s, lane, j):
    """first K of run j of lane `lane` (of a quarter-wave) at step s"""
    if bits == 4:
        return 512 * s + 64 * (lane >> 1) + 32 * (j & 1) + 8 * (2 * (lane & 1) + (j >> 1))
    return 256 * s + 64 * (lane >> 2) + 32 * j + 8 * (lane & 3)


def run_lds_byte(bits, s, lane, j):
    """LDS byte of the run's 8 fp16 A elements inside the row"""
    return (1024 if bits == 4 else 512) * s + 256 * j + 16 * lane


def run_codes(bits, row_bytes, s, lane, j):
    """the 8 codes of the run, K ascending, from the lane's 16 bytes [256 s + 16 lane, + 16) of the packed row"""
    b = row_bytes[256 * s + 16 * lane:256 * s + 16 * lane + 16]
    if bits == 8:
        return b[8 * j:8 * j + 8]
    word = int.from_bytes(bytes(b[4 * j:4 * j + 4]), "little")
    out = []
    for q in range(4):  # codes 2q, 2q + 1 at bits 4q and 16 + 4q
        out += [(word >> (4 * q)) & 15, (word >> (16 + 4 * q)) & 15]
    return out


def quant_row_source(bits, piece, copy_lane):
    """stage_f16: first K of the 8 elements that lane `copy_lane` (of 64) stores at LDS byte 1024 piece + 16 copy_lane"""
    lane, j = copy_lane & 15, copy_lane >> 4
    if bits == 4:
        return 512 * piece + 64 * (lane >> 1) + 32 * (j & 1) + 8 * (2 * (lane & 1) + (j >> 1))
    return 512 * piece + 256 * (j >> 1) + 64 * (lane >> 2) + 32 * (j & 1) + 8 * (lane & 3)


@pytest.mark.parametrize("K", [384, 640, 2176])
@pytest.mark.parametrize("bits", [4, 8])
def test_k_maps(bits, K):
    """The maps as the kernel's comments state them, restated above in Python, against the weight layout — not the
    kernel's own constants, which only the GPU read-back test (tests/test_decode_wo_gpu.py) exercises; this test also
    passes without the kernel. Every K of a row is held by exactly one (step, lane, run), with the codes
    quantize.unpack_weightonly_mi355x
    gives; the lanes past the row's end are those of the last step only, a whole number of lanes; the A row's permuted
    copy puts K where the run reads it, and the pad behind the row maps to no K (zeros); the g128 group of a lane's
    runs is 4 s + (lane >> 2) / 2 s + (lane >> 3)."""
    g = torch.Generator().manual_seed(K + bits)
    codes = torch.randint(0, 1 << bits, (2, K), generator=g, dtype=torch.uint8)
    packed = quantize.pack_weightonly_mi355x(codes, bits)
    assert torch.equal(quantize.unpack_weightonly_mi355x(packed, bits, K), codes)
    KB = K * bits // 8
    assert packed.shape == (2, KB) and KB % 16 == 0
    steps, runs, step_lds = -(-KB // 256), (4 if bits == 4 else 2), (1024 if bits == 4 else 512)
    hits = torch.zeros(K, dtype=torch.int32)
    lds_of_k = {}
    for s in range(steps):
        for lane in range(16):
            inside = 256 * s + 16 * lane < KB
            assert inside or s == steps - 1  # a lane past the end: only inside the last step
            for j in range(runs):
                k, byte = run_k(bits, s, lane, j), run_lds_byte(bits, s, lane, j)
                assert byte + 16 <= steps * step_lds <= -(-2 * K // 1024) * 1024  # inside the padded LDS row
                if not inside:
                    assert k >= K  # its codes are zeroed and its A bytes are the pad
                    lds_of_k[byte] = None
                    continue
                assert k % 8 == 0 and k + 8 <= K
                hits[k:k + 8] += 1
                lds_of_k[byte] = k
                for r in range(2):
                    assert run_codes(bits, packed[r].tolist(), s, lane, j) == codes[r, k:k + 8].tolist(), (s, lane, j)
                assert k // 128 == (4 * s + (lane >> 2) if bits == 4 else 2 * s + (lane >> 3))
    assert (hits == 1).all()
    assert sorted(lds_of_k) == list(range(0, steps * step_lds, 16))  # every 16-byte slot of the steps, once
    # stage_f16's copy: passes of 1024 bytes, lane c stores slot c
    for piece in range(-(-2 * K // 1024)):
        for c in range(64):
            byte, k = 1024 * piece + 16 * c, quant_row_source(bits, piece, c)
            if byte in lds_of_k and lds_of_k[byte] is not None:
                assert k == lds_of_k[byte], (piece, c)
            else:
                assert k >= K  # stored as zeros
    # conflict-free reads: the 16 lanes of a quarter read 16 consecutive 16-byte slots
    for j in range(runs):
        assert [run_lds_byte(bits, 1, lane, j) - run_lds_byte(bits, 1, 0, j) for lane in range(16)] == list(range(0, 256, 16))


def test_f64_to_f16_rounds_once():
    """quantize._f64_to_f16 (the last step of dequant_weightonly, the read-back test's reference) rounds an exact
    float64 value to fp16 once. The tie cases are written out by hand: 1 + 2^-11 lies exactly between the fp16
    neighbours 1 and 1 + 2^-10, so a value just above it rounds up and one just below it rounds down — but float32
    keeps 24 bits, rounds both onto the tie itself, and the second rounding (to even) then gives 1 for both. numpy's
    float64 -> float16 conversion rounds once and is the second witness, on random sums of the read-back test's form."""
    import numpy as np

    tie = 1.0 + 2.0 ** -11
    v = torch.tensor([tie + 2.0 ** -30, tie - 2.0 ** -30, tie, -(tie + 2.0 ** -30), 3.0 + 2.0 ** -10, 3.0 + 2.0 ** -10 + 2.0 ** -30,
                      2.0 ** -24 * (1.5 + 2.0 ** -20), 2.0 ** -24 * (0.5 + 2.0 ** -20), 2.0 ** -24 * 0.5, 65504.0, 0.0],
                     dtype=torch.float64)
    want = [1.0 + 2.0 ** -10, 1.0, 1.0, -(1.0 + 2.0 ** -10), 3.0, 3.0 + 2.0 ** -9,
            2.0 ** -23, 2.0 ** -24, 0.0, 65504.0, 0.0]
    assert quantize._f64_to_f16(v).tolist() == want
    assert v.half().tolist()[:2] == [1.0, 1.0]  # what the conversion through float32 gives: the first is one ulp off
    g = torch.Generator().manual_seed(11)
    f16 = lambda hi: (torch.randint(0, hi << 10, (200000,), generator=g, dtype=torch.int32) |
                      torch.randint(0, 2, (200000,), generator=g, dtype=torch.int32) << 15).to(torch.int16).view(torch.float16)
    x = torch.randint(0, 256, (200000,), generator=g).double() * f16(20).double() + f16(24).double()  # u * scale + zp
    direct = torch.from_numpy(x.numpy().astype(np.float16))
    assert torch.equal(quantize._f64_to_f16(x).view(torch.int16), direct.view(torch.int16))
    assert not torch.equal(x.half().view(torch.int16), direct.view(torch.int16))  # the draw does hold double-rounding cases
