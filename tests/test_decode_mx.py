"""The decode forward for gpt-oss layers without a GPU (mxmoe_moe_decode_gate_up_ex, mxmoe_moe_decode_down_ex;
moe.DecodeForwardEx): the C ABI's host validation (dummy pointers, every refusal made before any HIP call and reported
under the entry's name), DecodeForwardEx's constructor on CPU-built layers, and the lane -> scale-byte map the
W4A16_MX kernel hard-codes."""
from __future__ import annotations

import ctypes
import math
import re
from pathlib import Path

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe, quantize
from mxmoe_amd.groupgemm import FP16, W4A4_G128, W4A4_MXFP4, W4A8_MXFP8, W4A16_MXFP4, W8A8
from tests._decode_util import cpu_ffn, entry_down, entry_gate_up, err

INVALID, UNSUPPORTED, OK = nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_OK
ALL_KINDS = 0b1111
ROOT = Path(__file__).resolve().parent.parent


def _glu(act=nat.GLU_SWIGLU_CLAMP, alpha=1.702, limit=7.0, bias_routed=32, bias_shared=64):
    return nat.MoeGluC(act, alpha, limit, bias_routed, bias_shared)


def _gate_up(**kw):
    return entry_gate_up("ex", **dict(dict(mask=ALL_KINDS), **kw))


def _down(**kw):
    return entry_down("ex", **dict(dict(mask=ALL_KINDS), **kw))


ENTRIES = [(_gate_up, b"mxmoe_moe_decode_gate_up_ex"), (_down, b"mxmoe_moe_decode_down_ex")]


def test_abi_symbols_and_constants():
    """★ 1. The two entries are exported, declared and bound; ABI 7; the record is still 40 bytes; kind 3."""
    lib = nat.lib()
    assert lib.mxmoe_gg_abi_version() == 7 == nat.ABI_VERSION  # additive: no version bump
    assert nat.DECODE_EX_SYMBOLS == ("mxmoe_moe_decode_gate_up_ex", "mxmoe_moe_decode_down_ex")
    header = (ROOT / "include" / "mxmoe_moe.h").read_text()
    declared = set(re.findall(r"^int (mxmoe_moe_\w+)\(", header, flags=re.M))
    for fn in nat.DECODE_EX_SYMBOLS + nat.DECODE_SYMBOLS:
        assert fn in nat.EXPORTED_SYMBOLS and hasattr(lib, fn) and fn in declared
    assert declared <= set(nat.EXPORTED_SYMBOLS)  # the header declares nothing the binding does not list
    assert nat.DECODE_W4A16_MX == 3 and "MXMOE_DECODE_W4A16_MX = 3" in header
    assert moe.DecodeForwardEx.KINDS["w4a16_g32_sym_MXFP4"] == 3 and "w4a16_g32_sym_MXFP4" not in moe.DecodeForward.KINDS
    assert ctypes.sizeof(nat.MoeDecodeExpertC) == 40
    assert lib.mxmoe_moe_decode_gate_up_ex.argtypes[3] is ctypes.c_int64
    assert lib.mxmoe_moe_decode_down_ex.argtypes[0] is ctypes.c_int64


@pytest.mark.parametrize("call,name", ENTRIES)
def test_limits_are_refused_before_any_hip_call(call, name):
    """★ 1. Everything the first two entries check, under the _ex entry's name; T = 0 is OK with no launch."""
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
    """★ 1. Kind bit 3 is a kind here; a bit >= 4 is MXMOE_GG_ERR_UNSUPPORTED, also for an empty batch."""
    for mask in (1 << 3, ALL_KINDS, 0b1001, 1, 6):
        assert call(mask=mask, T=0) == OK, mask
    for mask in (1 << 4, ALL_KINDS | 1 << 4, 1 << 31):
        assert call(mask=mask) == UNSUPPORTED, mask
        assert name in err() and b"kind" in err()
        assert call(mask=mask, T=0) == UNSUPPORTED


def test_entry_specific_refusals():
    """★ 1. gate_up_ex: dtype, layout, hidden and the glu checks of mxmoe_moe_glu_quant; down_ex: y / ys."""
    name = b"mxmoe_moe_decode_gate_up_ex"
    for kw in (dict(dtype=2), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(hidden=8), dict(hidden=None)):
        assert _gate_up(**kw) == INVALID, kw
        assert name in err(), kw
    for glu in (_glu(act=2), _glu(act=-1), _glu(alpha=math.inf), _glu(alpha=math.nan), _glu(limit=0.0), _glu(limit=-1.0),
                _glu(limit=math.inf), _glu(limit=math.nan), _glu(bias_routed=8), _glu(bias_shared=24)):
        assert _gate_up(glu=glu) == INVALID, (glu.act, glu.alpha, glu.limit, glu.bias_routed, glu.bias_shared)
        assert name in err()
        assert _gate_up(glu=glu, T=0) == INVALID  # (before the empty-batch return)
    assert _gate_up(glu=_glu(), with_shared=0, act_shared=None) == INVALID  # bias_shared without a shared expert
    assert name in err() and b"bias_shared" in err()
    assert _gate_up(glu=_glu(), T=0) == OK
    assert _gate_up(glu=_glu(bias_shared=None), with_shared=0, act_shared=None, T=0) == OK
    assert _gate_up(glu=_glu(act=nat.GLU_SILU, alpha=math.nan, limit=-1.0, bias_routed=None, bias_shared=None), T=0) == OK
    assert _gate_up(glu=None, dtype=nat.DT_BF16, layout=nat.DECODE_GU_INTERLEAVED, T=0) == OK
    for kw in (dict(y=8), dict(ys=4), dict(y=None), dict(ys=None)):
        assert _down(**kw) == INVALID, kw
        assert b"mxmoe_moe_decode_down_ex" in err(), kw
    assert _down(with_shared=0, ys=None, act_shared=None, T=0) == OK


def _gptoss(E=4, H=256, N=128, act_bits=16, seed=3):
    g = torch.Generator().manual_seed(seed)
    u8 = lambda *shape, lo=0, hi=256: torch.randint(lo, hi, shape, generator=g, dtype=torch.uint8)
    return moe.gptoss_layer(u8(E, 2 * N, H // 32, 16), u8(E, 2 * N, H // 32, lo=118, hi=127), torch.rand(E, 2 * N, generator=g) - 0.5,
                            u8(E, H, N // 32, 16), u8(E, H, N // 32, lo=118, hi=127), torch.rand(E, H, generator=g) - 0.5,
                            act_bits=act_bits)


def test_decode_forward_ex_on_cpu_built_layers():
    """★ 2. DecodeForwardEx constructs for a biased w8a8 layer, an fp16 SwigluClamp layer and a gptoss_layer (which
    DecodeForward still refuses), and refuses the a4 / a8 MX forms and g128 naming the qcfg."""
    biased = cpu_ffn([(W8A8, W8A8)] * 3, down_bias=[torch.zeros(256) for _ in range(3)])
    gated = cpu_ffn([(FP16, FP16)] * 3, activation=moe.SwigluClamp())
    oss = _gptoss()
    assert biased.biased_or_gated and gated.biased_or_gated and oss.biased_or_gated
    for layer, E in ((biased, 2), (gated, 2), (oss, 4)):
        df = moe.DecodeForwardEx(layer, 4, 2)
        assert df._glu is not None and df.layout == nat.DECODE_GU_PLAIN and df.act.shape == (8, layer.N)
        assert df.experts.numel() == 40 * len(layer.w1) and df.inv_slot.tolist() == list(range(8))
    df = moe.DecodeForwardEx(oss, 16, 4)
    assert df.mask1 == df.mask2 == 1 << nat.DECODE_W4A16_MX
    rec = nat.MoeDecodeExpertC.from_buffer_copy(bytes(df.experts[40:80].tolist()))  # the layer's own tensors, no copy
    assert (rec.b1, rec.sb1, rec.kind1) == (oss.w1[1].B.data_ptr(), oss.w1[1].scale_b.data_ptr(), 3)
    assert (rec.b2, rec.sb2, rec.kind2) == (oss.w2[1].B.data_ptr(), oss.w2[1].scale_b.data_ptr(), 3)
    assert df._glu.act == nat.GLU_SWIGLU_CLAMP and df._glu.bias_routed == oss.b1.data_ptr()
    mixed = moe.DecodeForwardEx(cpu_ffn([(W4A16_MXFP4, W8A8), (FP16, W4A16_MXFP4), (W8A8, W8A8)]), 4, 2)
    assert mixed.mask1 == 0b1011 and mixed.mask2 == 0b1010 and mixed._glu is None
    plain = moe.DecodeForwardEx(cpu_ffn([(W8A8, W8A8)] * 3), 4, 2)  # a layer DecodeForward takes: its layout and no glu
    assert plain._glu is None and plain.layout == nat.DECODE_GU_INTERLEAVED
    with pytest.raises(ValueError, match="bias"):
        moe.DecodeForward(biased, 4, 2)
    with pytest.raises(ValueError, match="activation"):
        moe.DecodeForward(gated, 4, 2)
    with pytest.raises(ValueError):
        moe.DecodeForward(oss, 4, 2)
    with pytest.raises(ValueError, match="w4a4_g32_sym_MXFP4"):
        moe.DecodeForwardEx(cpu_ffn([(W8A8, W8A8), (W4A4_MXFP4, W4A4_MXFP4), (W8A8, W8A8)]), 4, 2)
    with pytest.raises(ValueError, match="w4a4_g32_sym_MXFP4"):
        moe.DecodeForwardEx(_gptoss(act_bits=4), 4, 2)
    with pytest.raises(ValueError, match="w4a8_g32_sym_MXFP8"):
        moe.DecodeForwardEx(_gptoss(act_bits=8), 4, 2)
    with pytest.raises(ValueError, match="w4a8_g32_sym_MXFP8"):
        moe.DecodeForwardEx(cpu_ffn([(W8A8, W8A8), (W8A8, W4A8_MXFP8), (W8A8, W8A8)]), 4, 2)
    with pytest.raises(ValueError, match="w4a4_g128_sym"):
        moe.DecodeForwardEx(cpu_ffn([(W8A8, W8A8), (W8A8, W4A4_G128), (W8A8, W8A8)]), 4, 2)
    with pytest.raises(ValueError, match="T = 17"):
        moe.DecodeForwardEx(oss, 17, 2)


@pytest.mark.parametrize("K", [384, 640, 2944])
def test_lane_to_scale_byte_map(K):
    """★ 3. Lane l of a quarter-wave at step s owns MX block 16 s + l of a weight row and reads device scale byte
    16 s + 4 (l & 3) + (l >> 2): against pack_mxfp4_scales / unpack_mxfp4_scales. A row has 16 ceil(K / 512) device
    bytes, as many 16-byte groups as the weight row has 256-byte steps, and the bytes past K / 32 are 127."""
    nb, steps = K // 32, -(-K // 512)
    g = torch.Generator().manual_seed(K)
    canon = torch.randint(0, 255, (3, nb), generator=g, dtype=torch.uint8)
    dev = quantize.pack_mxfp4_scales(canon)
    assert dev.shape == (3, 16 * steps) and steps == -(-(K // 2) // 256)
    assert torch.equal(quantize.unpack_mxfp4_scales(dev, K), canon)
    seen = set()
    for s in range(steps):
        for lane in range(16):
            block, byte = 16 * s + lane, 16 * s + 4 * (lane & 3) + (lane >> 2)
            seen.add(byte)
            if block < nb:
                assert torch.equal(dev[:, byte], canon[:, block]), (s, lane)
            else:
                assert (dev[:, byte] == 127).all(), (s, lane)
    assert seen == set(range(16 * steps))
