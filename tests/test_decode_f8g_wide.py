"""The wide decode forward for block-scaled FP8 experts without a GPU (mxmoe_moe_decode_quant_f8g,
mxmoe_moe_decode_gate_up_f8g_wide, mxmoe_moe_decode_down_f8g_wide; moe.DecodeForwardF8gWide): the C ABI's host
validation on made-up addresses and the class's constructor on CPU-built layers."""
from __future__ import annotations

import re
from pathlib import Path

import pytest

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W8A8_G128_E4M3 as QG
from tests._decode_util import cpu_ffn, err

UNSUPPORTED, INVALID, OK = nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_OK
BIT = 1 << 15


def _gate_up(T=4, H=256, mask=BIT, layout=nat.DECODE_GU_PLAIN):
    return nat.symbol("mxmoe_moe_decode_gate_up_f8g_wide")(None, 16, 16, T, 2, 4, 1, 16, 16, mask, H, 128, 256, layout, 16, 16,
                                                           None, None)


def _down(T=4, H=256, mask=BIT, layout=None):
    return nat.symbol("mxmoe_moe_decode_down_f8g_wide")(T, 2, 4, 1, 16, 16, mask, H, 128, 256, 16, 16, 16, 16, 16, 16, None, None)


def test_symbols():
    header = (Path(__file__).resolve().parent.parent / "include" / "mxmoe_moe.h").read_text()
    assert len(nat.DECODE_F8G_WIDE_SYMBOLS) == 3
    for fn in nat.DECODE_F8G_WIDE_SYMBOLS:
        assert fn in nat.EXPORTED_SYMBOLS and re.search(rf"^int {fn}\(", header, flags=re.M) and nat.symbol(fn)
    assert nat.DECODE_WIDE_MAX_T == 64 and re.search(r"\bMXMOE_DECODE_WIDE_MAX_T = 64\b", header)
    assert nat.DECODE_MAX_T == 16


@pytest.mark.parametrize("call,name", [(_gate_up, b"mxmoe_moe_decode_gate_up_f8g_wide"),
                                       (_down, b"mxmoe_moe_decode_down_f8g_wide")])
def test_host_refusals(call, name):
    """Refused before any HIP call (the addresses are made up), under the entry's name; T = 0 is accepted."""
    cases = [(dict(mask=m), UNSUPPORTED) for m in (0, 1 << 12, BIT | 1)] + [(dict(H=192), INVALID), (dict(T=65), INVALID)]
    if call is _gate_up:
        cases.append((dict(layout=nat.DECODE_GU_INTERLEAVED), UNSUPPORTED))
    for kw, code in cases:
        assert call(**kw) == code, kw
        assert name in err(), kw
    assert call(T=0) == OK
    quant = nat.symbol("mxmoe_moe_decode_quant_f8g")
    assert quant(nat.DT_FP16, 16, 1025, 128, 16, 16, None, 0, 0, None, None, None) == INVALID
    assert quant(nat.DT_FP16, 16, 4, 192, 16, 16, None, 0, 0, None, None, None) == INVALID
    assert quant(nat.DT_FP16, None, 0, 0, None, None, None, 0, 0, None, None, None) == OK


@pytest.mark.parametrize("fn,args", [
    ("mxmoe_moe_decode_gate_up_f8g_wide", (None, 16, 16, 64, 2, 4, 1, 16, 16, BIT, 256, 128, 256, 0, 8, 16, None, None)),
    ("mxmoe_moe_decode_down_f8g_wide", (64, 2, 4, 1, 16, 16, BIT, 256, 128, 256, 16, 16, 16, 16, 8, 16, None, None))])
def test_t64_passes_the_size_checks(fn, args):
    """T = 64 gets as far as the pointer checks (a misaligned output), which follow the checks of T."""
    assert nat.symbol(fn)(*args) == INVALID and b"misaligned" in err()


def test_class_on_cpu_layers():
    ffn = cpu_ffn([(QG, QG)] * 3)
    df = moe.DecodeForwardF8gWide(ffn, 64, 2)
    assert df.mask1 == df.mask2 == BIT and df.layout == nat.DECODE_GU_PLAIN and df.MAX_T == 64
    assert df.codes_hidden.shape == (64, ffn.H) and df.scales_hidden.shape == (64, ffn.H // 128)
    assert df.codes_act.shape == (128, ffn.N) and df.scales_act_shared.shape == (64, ffn.Ns // 128)
    with pytest.raises(ValueError, match="T = 65"):
        moe.DecodeForwardF8gWide(ffn, 65, 2)
    with pytest.raises(ValueError, match="fp16"):
        moe.DecodeForwardF8gWide(cpu_ffn([(QG, QG), (QG, FP16), (QG, QG)]), 4, 2)
    ffn.w2[1].scale_b = ffn.w2[1].scale_b.half()
    with pytest.raises(ValueError, match="scale buffer of a w8a8_g128_sym_E4M3"):
        moe.DecodeForwardF8gWide(ffn, 64, 2)
