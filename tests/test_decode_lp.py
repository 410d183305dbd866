"""The decode forward on MFMA without a GPU (mxmoe_moe_decode_gate_up_lp, mxmoe_moe_decode_down_lp;
moe.DecodeForwardLp): the C ABI's host validation on made-up addresses and the class's constructor on CPU-built layers.

The expert records live in device memory, so the entries cannot see a weight's or an e8m0 row's address: a misaligned
one is refused by the class, which builds the records (the last two cases of test_refusals_by_name)."""
from __future__ import annotations

import re
from pathlib import Path

import pytest

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import (W2A16_G128_ASYM, W4A4_G128, W4A4_MXFP4, W4A8_MXFP8, W4A16_ASYM, W8A8, W8A8_E4M3,
                                 SUPPORTED)
from tests._decode_util import cpu_ffn, err

INVALID, UNSUPPORTED, OK = nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_OK
ALL_KINDS = (1 << 15) - 1
NEW = {"w8a8_g-1_sym_E4M3": 12, "w4a8_g32_sym_MXFP8": 13, "w4a4_g32_sym_MXFP4": 14}


def _gate_up(T=4, H=256, mask=ALL_KINDS, act=16):
    return nat.symbol("mxmoe_moe_decode_gate_up_lp")(None, nat.DT_FP16, 16, T, 2, 4, 1, 16, 16, mask, H, 128, 256,
                                                     nat.DECODE_GU_PLAIN, act, 16, None, None)


def _down(T=4, H=256, mask=ALL_KINDS, act=16):
    return nat.symbol("mxmoe_moe_decode_down_lp")(T, 2, 4, 1, 16, 16, mask, H, 128, 256, act, 16, 16, 16, None, None)


def test_symbols_and_kinds():
    """The two entries are exported, declared and bound with the _wo entries' signatures; ABI 7; each of the fifteen
    qcfgs maps to its constant, in the class, the binding and the header."""
    lib = nat.lib()
    assert lib.mxmoe_gg_abi_version() == 7 == nat.ABI_VERSION
    assert nat.DECODE_LP_SYMBOLS == ("mxmoe_moe_decode_gate_up_lp", "mxmoe_moe_decode_down_lp")
    header = (Path(__file__).resolve().parent.parent / "include" / "mxmoe_moe.h").read_text()
    for fn, wo in zip(nat.DECODE_LP_SYMBOLS, nat.DECODE_WO_SYMBOLS):
        assert fn in nat.EXPORTED_SYMBOLS and re.search(rf"^int {fn}\(", header, flags=re.M)
        assert getattr(lib, fn).argtypes == getattr(lib, wo).argtypes
    kinds = moe.DecodeForwardLp.KINDS
    assert {k: v for k, v in kinds.items() if v < 12} == moe.DecodeForwardWo.KINDS
    assert {k: v for k, v in kinds.items() if v >= 12} == NEW and sorted(kinds.values()) == list(range(15))
    for qcfg, kind in NEW.items():
        name = {12: "W8A8_E4M3", 13: "W4A8_MXFP8", 14: "W4A4_MXFP4"}[kind]
        assert getattr(nat, "DECODE_" + name) == kind and re.search(rf"\bMXMOE_DECODE_{name} = {kind}\b", header)
        assert qcfg in SUPPORTED and qcfg not in moe.DecodeForwardWo.KINDS


@pytest.mark.parametrize("call,name", [(_gate_up, b"mxmoe_moe_decode_gate_up_lp"), (_down, b"mxmoe_moe_decode_down_lp")])
def test_host_refusals(call, name):
    """Refused before any HIP call, under the entry's name; kinds 0 to 14 are kinds here."""
    for kw, code in ((dict(T=17), INVALID), (dict(H=192), INVALID), (dict(act=8), INVALID), (dict(mask=0), INVALID),
                     (dict(mask=1 << 15), UNSUPPORTED), (dict(mask=ALL_KINDS | 1 << 15, T=0), UNSUPPORTED)):
        assert call(**kw) == code, kw
        assert name in err(), kw
    for mask in [1 << k for k in range(15)] + [ALL_KINDS]:
        assert call(mask=mask, T=0) == OK, mask


def test_constructs_on_cpu_layers():
    """One layer per new type and a mixed one: masks, layouts and the layer's own tensors in the records."""
    for q, kind in ((W8A8_E4M3, 12), (W4A8_MXFP8, 13), (W4A4_MXFP4, 14)):
        ffn = cpu_ffn([(q, q)] * 3)
        df = moe.DecodeForwardLp(ffn, 16, 2)
        assert df.mask1 == df.mask2 == 1 << kind
        assert df.layout == (nat.DECODE_GU_INTERLEAVED if q is W4A8_MXFP8 else nat.DECODE_GU_PLAIN)
        rec = nat.MoeDecodeExpertC.from_buffer_copy(bytes(df.experts[80:120].tolist()))
        assert (rec.b1, rec.sb2, rec.kind1, rec.kind2) == (ffn.w1[2].B.data_ptr(), ffn.w2[2].scale_b.data_ptr(), kind, kind)
        for cls in (moe.DecodeForward, moe.DecodeForwardEx, moe.DecodeForwardWo):
            with pytest.raises(ValueError, match=q.qcfg):
                cls(ffn, 4, 2)
    mixed = moe.DecodeForwardLp(cpu_ffn([(W8A8_E4M3, W4A4_MXFP4), (W4A16_ASYM, W8A8_E4M3), (W4A8_MXFP8, W8A8)]), 4, 2)
    assert mixed.mask1 == 1 << 12 | 1 << 8 | 1 << 13 and mixed.mask2 == 1 << 14 | 1 << 12 | 1 << 1


def test_refusals_by_name():
    for q in (W4A4_G128, W2A16_G128_ASYM):
        with pytest.raises(ValueError, match=q.qcfg):
            moe.DecodeForwardLp(cpu_ffn([(W8A8_E4M3, q)] * 3), 4, 2)
    ok = cpu_ffn([(W8A8_E4M3, W4A8_MXFP8)] * 3)
    with pytest.raises(ValueError, match="T = 17"):
        moe.DecodeForwardLp(ok, 17, 2)
    w1, w2 = ok.w1[1], ok.w2[1]
    w1.scale_b = w1.scale_b[:-1]
    with pytest.raises(ValueError, match="scale buffer of a w8a8_g-1_sym_E4M3"):
        moe.DecodeForwardLp(ok, 16, 2)
    ok.w1[1] = cpu_ffn([(W8A8_E4M3, W4A8_MXFP8)] * 3).w1[1]
    rows = w2.scale_b
    w2.scale_b = rows.flatten().clone().new_zeros(rows.numel() + 4)[1:1 + rows.numel()].view(rows.shape)  # address % 4 == 1
    with pytest.raises(ValueError, match="e8m0 rows"):
        moe.DecodeForwardLp(ok, 16, 2)
    w2.scale_b = rows
    w2.B = w2.B.flatten().new_zeros(w2.B.numel() + 16)[8:8 + w2.B.numel()].view(w2.B.shape)  # address % 16 == 8
    with pytest.raises(ValueError, match="16-byte aligned"):
        moe.DecodeForwardLp(ok, 16, 2)
