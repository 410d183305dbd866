"""The decode forward for block-scaled FP8 experts without a GPU (mxmoe_moe_decode_gate_up_f8g,
mxmoe_moe_decode_down_f8g; moe.DecodeForwardF8g): the C ABI's host validation on made-up addresses and the class's
constructor on CPU-built layers."""
from __future__ import annotations

import re
from pathlib import Path

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W8A8_E4M3, W8A8_G128_E4M3
from tests._decode_util import cpu_ffn, err

UNSUPPORTED, INVALID, OK = nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_OK
QG, BIT = W8A8_G128_E4M3, 1 << 15


def _gate_up(T=4, H=256, mask=BIT, layout=nat.DECODE_GU_PLAIN):
    return nat.symbol("mxmoe_moe_decode_gate_up_f8g")(None, nat.DT_FP16, 16, T, 2, 4, 1, 16, 16, mask, H, 128, 256, layout,
                                                      16, 16, None, None)


def _down(T=4, H=256, mask=BIT, layout=None):
    return nat.symbol("mxmoe_moe_decode_down_f8g")(T, 2, 4, 1, 16, 16, mask, H, 128, 256, 16, 16, 16, 16, None, None)


def test_symbols():
    lib = nat.lib()
    assert nat.DECODE_F8G_SYMBOLS == ("mxmoe_moe_decode_gate_up_f8g", "mxmoe_moe_decode_down_f8g")
    header = (Path(__file__).resolve().parent.parent / "include" / "mxmoe_moe.h").read_text()
    for fn, lp in zip(nat.DECODE_F8G_SYMBOLS, nat.DECODE_LP_SYMBOLS):
        assert fn in nat.EXPORTED_SYMBOLS and re.search(rf"^int {fn}\(", header, flags=re.M)
        assert getattr(lib, fn).argtypes == getattr(lib, lp).argtypes
    assert nat.DECODE_W8A8_G128_E4M3 == 15 and re.search(r"\bMXMOE_DECODE_W8A8_G128_E4M3 = 15\b", header)
    assert moe.DecodeForwardF8g.KINDS == {"w8a8_g128_sym_E4M3": 15}


@pytest.mark.parametrize("call,name", [(_gate_up, b"mxmoe_moe_decode_gate_up_f8g"), (_down, b"mxmoe_moe_decode_down_f8g")])
def test_host_refusals(call, name):
    """Refused before any HIP call (the addresses are made up), under the entry's name; T = 0 is accepted."""
    cases = [(dict(mask=m), UNSUPPORTED) for m in (0, 1 << 12, BIT | 1, 1 << 16)] + [(dict(H=192), INVALID), (dict(T=17), INVALID)]
    if call is _gate_up:
        cases.append((dict(layout=nat.DECODE_GU_INTERLEAVED), UNSUPPORTED))
    for kw, code in cases:
        assert call(**kw) == code, kw
        assert name in err(), kw
    assert call(T=0) == OK


def test_class_on_cpu_layers():
    for other in (FP16, W8A8_E4M3):  # a layer holding another type: refused, naming it
        with pytest.raises(ValueError, match=other.qcfg.replace("-", r"\-")):
            moe.DecodeForwardF8g(cpu_ffn([(QG, QG), (QG, other), (QG, QG)]), 4, 2)
    ffn = cpu_ffn([(QG, QG)] * 3)
    df = moe.DecodeForwardF8g(ffn, 16, 2)
    assert df.mask1 == df.mask2 == BIT and df.layout == nat.DECODE_GU_PLAIN
    rec = nat.MoeDecodeExpertC.from_buffer_copy(bytes(df.experts[80:120].tolist()))
    assert (rec.b1, rec.sb2, rec.kind1, rec.kind2) == (ffn.w1[2].B.data_ptr(), ffn.w2[2].scale_b.data_ptr(), 15, 15)
    for cls in (moe.DecodeForward, moe.DecodeForwardEx, moe.DecodeForwardWo, moe.DecodeForwardLp):
        with pytest.raises(ValueError, match=QG.qcfg):
            cls(ffn, 4, 2)
    sb = ffn.w2[1].scale_b
    for wrong in (sb.half(), sb.flatten()[:-1], torch.cat([sb.flatten(), sb.flatten()])):
        ffn.w2[1].scale_b = wrong
        with pytest.raises(ValueError, match="scale buffer of a w8a8_g128_sym_E4M3"):
            moe.DecodeForwardF8g(ffn, 16, 2)
