"""The decode forward without a GPU (mxmoe_moe_decode_gate_up, mxmoe_moe_decode_down; moe.DecodeForward): the C
ABI's host validation (dummy pointers, every refusal made before any HIP call and reported under the entry's name) and
DecodeForward's ValueErrors."""
from __future__ import annotations

import ctypes

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W4A4_G128, W4A4_MXFP4, W8A8
from tests._decode_util import cpu_ffn, entry_down, entry_gate_up, err

INVALID, UNSUPPORTED, OK = nat.MXMOE_GG_ERR_INVALID, nat.MXMOE_GG_ERR_UNSUPPORTED, nat.MXMOE_GG_OK
ALL_KINDS = 0b111


def _gate_up(**kw):
    return entry_gate_up("first", **dict(dict(mask=ALL_KINDS), **kw))


def _down(**kw):
    return entry_down("first", **dict(dict(mask=ALL_KINDS), **kw))


ENTRIES = [(_gate_up, b"mxmoe_moe_decode_gate_up"), (_down, b"mxmoe_moe_decode_down")]


def test_abi_symbols_and_constants():
    lib = nat.lib()
    assert lib.mxmoe_gg_abi_version() == 7 == nat.ABI_VERSION  # additive: no version bump
    for fn in nat.DECODE_SYMBOLS:
        assert fn in nat.EXPORTED_SYMBOLS and hasattr(lib, fn)
    assert nat.DECODE_MAX_T == 16 == moe.DecodeForward.MAX_T
    assert (nat.DECODE_FP16, nat.DECODE_W8A8, nat.DECODE_W4A4) == (0, 1, 2)
    assert ctypes.sizeof(nat.MoeDecodeExpertC) == 40  # four pointers and two int32
    assert lib.mxmoe_moe_decode_gate_up.argtypes[2] is ctypes.c_int64 and lib.mxmoe_moe_decode_down.argtypes[0] is ctypes.c_int64


@pytest.mark.parametrize("call,name", ENTRIES)
def test_limits_are_refused_before_any_hip_call(call, name):
    """★ The issue's refusals (T = 17, H = 192, a misaligned pointer) and every other limit: MXMOE_GG_ERR_INVALID under
    the entry's name, on a host without a GPU."""
    for kw in (dict(T=17), dict(T=-1), dict(H=192), dict(H=0), dict(H=16384 + 128), dict(N=100), dict(Ns=200), dict(Ns=0),
               dict(topk=0), dict(topk=17, E=32), dict(topk=5, E=4), dict(E=0), dict(act=8), dict(act_shared=24),
               dict(ids=2), dict(experts=4), dict(status=2), dict(mask=0), dict(ids=None), dict(experts=None),
               dict(act=None), dict(act_shared=None)):
        assert call(**kw) == INVALID, kw
        assert name in err(), kw
    assert call(T=0) == OK  # no launch
    assert call(T=0, with_shared=0, Ns=0, act_shared=None) == OK  # N_shared is not looked at without a shared expert
    assert call(T=0, H=16384, N=16384, Ns=16384, topk=16, E=16) == OK


@pytest.mark.parametrize("call,name", ENTRIES)
def test_unknown_kind_is_unsupported(call, name):
    """★ A kind that does not exist (a bit beyond the three kinds in kind_mask): MXMOE_GG_ERR_UNSUPPORTED, also for an
    empty batch."""
    for mask in (1 << 3, ALL_KINDS | 1 << 4, 1 << 31):
        assert call(mask=mask) == UNSUPPORTED, mask
        assert name in err() and b"kind" in err()
        assert call(mask=mask, T=0) == UNSUPPORTED
    for mask in (1, 2, 4, 3, 6, 7):
        assert call(mask=mask, T=0) == OK


def test_entry_specific_refusals():
    """★ gate_up: an unknown dtype, an unknown layout, a misaligned hidden; down: a misaligned or missing y / ys."""
    for kw in (dict(dtype=2), dict(dtype=-1), dict(layout=2), dict(layout=-1), dict(hidden=8), dict(hidden=None)):
        assert _gate_up(**kw) == INVALID, kw
        assert b"mxmoe_moe_decode_gate_up" in err(), kw
    assert _gate_up(dtype=2, T=0) == INVALID  # (before the empty-batch return)
    assert _gate_up(dtype=nat.DT_BF16, layout=nat.DECODE_GU_INTERLEAVED, T=0) == OK
    for kw in (dict(y=8), dict(ys=4), dict(y=None), dict(ys=None)):
        assert _down(**kw) == INVALID, kw
        assert b"mxmoe_moe_decode_down" in err(), kw
    assert _down(with_shared=0, ys=None, act_shared=None, T=0) == OK


def test_decode_forward_value_errors():
    """★ DecodeForward refuses, naming the reason: T = 17 (and 0), an MX qcfg, g128, a layer with a bias, a topk beyond
    the experts, a dtype that is neither fp16 nor bf16."""
    ok = cpu_ffn([(W8A8, W4A4), (FP16, W8A8), (W4A4, FP16)])
    with pytest.raises(ValueError, match="T = 17"):
        moe.DecodeForward(ok, 17, 2)
    with pytest.raises(ValueError, match="T = 0"):
        moe.DecodeForward(ok, 0, 2)
    with pytest.raises(ValueError, match="topk"):
        moe.DecodeForward(ok, 4, 3)
    with pytest.raises(ValueError, match="topk"):
        moe.DecodeForward(ok, 4)
    with pytest.raises(ValueError, match="dtype"):
        moe.DecodeForward(ok, 4, 2, dtype=torch.float32)
    with pytest.raises(ValueError, match="w4a4_g32_sym_MXFP4"):
        moe.DecodeForward(cpu_ffn([(W8A8, W8A8), (W4A4_MXFP4, W4A4_MXFP4), (W8A8, W8A8)]), 4, 2)
    with pytest.raises(ValueError, match="w4a4_g128_sym"):
        moe.DecodeForward(cpu_ffn([(W8A8, W8A8), (W8A8, W4A4_G128), (W8A8, W8A8)]), 4, 2)
    biased = cpu_ffn([(W8A8, W8A8)] * 3, down_bias=[torch.zeros(256) for _ in range(3)])
    assert biased.biased_or_gated
    with pytest.raises(ValueError, match="bias"):
        moe.DecodeForward(biased, 4, 2)
    gated = cpu_ffn([(FP16, FP16)] * 3, activation=moe.SwigluClamp())
    with pytest.raises(ValueError, match="activation"):
        moe.DecodeForward(gated, 4, 2)
