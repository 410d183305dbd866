"""The decode forward on the fp16 MFMA without a GPU (mxmoe_moe_decode_gate_up_a16, mxmoe_moe_decode_down_a16;
moe.DecodeForwardA16): the two entries' export, declaration and binding, their host refusals (dummy pointers, every
refusal made before any HIP call and reported under the entry's name) and the class's constructor on CPU-built layers."""
from __future__ import annotations

import ctypes
import re
from pathlib import Path

import pytest

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import W2A16_G128_ASYM, W4A16_ASYM, W4A16_G128_SYM, W4A16_MXFP4, W8A8
from tests._decode_util import cpu_ffn, err

INVALID, UNSUPPORTED, OK = nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_OK
ROOT = Path(__file__).resolve().parent.parent


def _gate_up(T=4, mask=(1 << 12) - 1, H=256, hidden=16):
    return nat.symbol("mxmoe_moe_decode_gate_up_a16")(None, nat.DT_FP16, hidden, T, 2, 4, 1, 16, 16, mask, H, 128, 256,
                                                      nat.DECODE_GU_PLAIN, 16, 16, None, None)


def _down(T=4, mask=(1 << 12) - 1, H=256, hidden=16):  # (hidden: the act pointer here)
    return nat.symbol("mxmoe_moe_decode_down_a16")(T, 2, 4, 1, 16, 16, mask, H, 128, 256, hidden, 16, 16, 16, None, None)


def test_symbols_are_exported_declared_and_bound():
    lib = nat.lib()
    assert lib.mxmoe_gg_abi_version() == 7 == nat.ABI_VERSION and ctypes.sizeof(nat.MoeDecodeExpertC) == 40
    assert nat.DECODE_A16_SYMBOLS == ("mxmoe_moe_decode_gate_up_a16", "mxmoe_moe_decode_down_a16")
    declared = set(re.findall(r"^int (mxmoe_moe_\w+)\(", (ROOT / "include" / "mxmoe_moe.h").read_text(), flags=re.M))
    for fn, wo in zip(nat.DECODE_A16_SYMBOLS, nat.DECODE_WO_SYMBOLS):
        assert fn in nat.EXPORTED_SYMBOLS and fn in declared and hasattr(lib, fn)
        assert getattr(lib, fn).argtypes == getattr(lib, wo).argtypes and getattr(lib, fn).restype is ctypes.c_int
    cls = moe.DecodeForwardA16
    assert cls.ENTRIES == nat.DECODE_A16_SYMBOLS and cls.KINDS == moe.DecodeForwardWo.KINDS and cls.TAKES_GLU and cls.TAKES_MX


@pytest.mark.parametrize("call,name", [(_gate_up, b"mxmoe_moe_decode_gate_up_a16"), (_down, b"mxmoe_moe_decode_down_a16")])
def test_host_refusals(call, name):
    """Kind bits 0..11 are kinds; bits 12 and 15 are UNSUPPORTED; T = 17, H = 192 and a misaligned pointer are INVALID;
    T = 0 is OK with no launch."""
    for mask in (1 << 12, 1 << 15):
        assert call(mask=mask) == UNSUPPORTED and name in err() and b"kind" in err()
    for kw in (dict(T=17), dict(H=192), dict(hidden=8)):
        assert call(**kw) == INVALID and name in err(), kw
    for mask in [1 << k for k in range(12)] + [(1 << 12) - 1]:
        assert call(T=0, mask=mask) == OK


def test_class_takes_and_refuses_by_name():
    """The scheme w4a16 + w8a8, a g128 layer and an MXFP4 layer construct with DecodeForwardWo's masks; an a8_view()
    layer, w2a16 and T = 17 are refused by name."""
    scheme = cpu_ffn([(W4A16_ASYM, W8A8), (W8A8, W4A16_ASYM), (W4A16_G128_SYM, W4A16_G128_SYM)])
    df, wo = moe.DecodeForwardA16(scheme, 16, 2), moe.DecodeForwardWo(scheme, 16, 2)
    assert (df.mask1, df.mask2, df.layout) == (wo.mask1, wo.mask2, wo.layout) and bytes(df.experts.tolist()) == bytes(wo.experts.tolist())
    mx = cpu_ffn([(W4A16_MXFP4, W4A16_MXFP4)] * 3)
    assert moe.DecodeForwardA16(mx, 4, 2).mask1 == 1 << nat.DECODE_W4A16_MX
    with pytest.raises(ValueError, match="w4a8_g32_sym_MXFP8"):
        moe.DecodeForwardA16(mx.a8_view(), 4, 2)
    with pytest.raises(ValueError, match="w2a16_g128_asym"):
        moe.DecodeForwardA16(cpu_ffn([(W8A8, W2A16_G128_ASYM)] * 3), 4, 2)
    with pytest.raises(ValueError, match="T = 17"):
        moe.DecodeForwardA16(scheme, 17, 2)
