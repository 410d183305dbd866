"""The router (mxmoe_moe_gate / moe.gate) without a GPU: the numpy reference of tests/_gate_ref.py
against torch's softmax -> topk, its tie rule, the C-ABI's host validation (before any HIP call) and
moe.gate's argument checks."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from tests import _gate_ref as ref


@pytest.mark.parametrize("renorm", [False, True])
def test_reference_matches_torch(renorm):
    T, H, E, k = 64, 128, 60, 4
    hidden, w = ref.random_data(T, H, E, seed=3)
    ids, wts, _, x = ref.gate(hidden, w, k, renormalize=renorm)
    srt = np.sort(x, axis=1)
    assert (np.diff(srt, axis=1) > 0).all(), "the logits of a row must be pairwise distinct for this comparison"
    tx = torch.from_numpy(x)
    tw, ti = torch.topk(torch.softmax(tx, dim=-1), k, dim=-1)
    if renorm:
        tw = tw / tw.sum(dim=-1, keepdim=True)
    assert (ids == ti.numpy()).all()
    assert np.abs(wts - tw.numpy()).max() <= 1e-12


def test_reference_tie_rule():
    T, H, E, k = 5, 64, 12, 3
    hidden = np.zeros((T, H), dtype=np.float16)
    _, w = ref.random_data(T, H, E, seed=4)
    ids, wts, _, _ = ref.gate(hidden, w, k)
    assert (ids == np.arange(k, dtype=np.int32)[None, :]).all()
    assert (wts == 1.0 / E).all()
    _, wts, _, _ = ref.gate(hidden, w, k, renormalize=True)
    assert np.abs(wts - 1.0 / k).max() <= 1e-15
    # -0 and +0 are equal logits: the lower index wins
    x = np.array([[0.0, -0.0, 1.0, -0.0]])
    assert ref.select(x, 3).tolist() == [[2, 0, 1]]


def _call(hidden=16, w_gate=16, w_sg=None, T=4, H=64, E=8, topk=2, renorm=0, ids=16, wts=16, shared_w=None,
          logits=None):
    st = nat.lib().mxmoe_moe_gate(hidden, w_gate, w_sg, T, H, E, topk, renorm, ids, wts, shared_w, logits, None)
    return st, nat.lib().mxmoe_gg_last_error()


@pytest.mark.parametrize("kw", [
    dict(E=0), dict(E=257), dict(topk=0), dict(E=8, topk=9), dict(E=64, topk=17), dict(H=48), dict(T=-1),
    dict(hidden=8), dict(w_gate=24), dict(w_sg=16), dict(shared_w=16), dict(w_sg=8, shared_w=16),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_abi_validation_before_any_hip_call(kw):
    """Dummy (never dereferenced) pointers: every bad argument is refused on the host."""
    st, err = _call(**kw)
    assert st == nat.MXMOE_GG_ERR_INVALID
    assert err and b"mxmoe_moe_gate" in err


def test_abi_empty_batch_is_ok():
    assert _call(T=0)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, hidden=None, w_gate=None, ids=None, wts=None)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, w_sg=16, shared_w=16, logits=16)[0] == nat.MXMOE_GG_OK
    assert "mxmoe_moe_gate" in nat.EXPORTED_SYMBOLS
    assert nat.lib().mxmoe_moe_gate.argtypes[3] is ctypes.c_int64


def test_gate_argument_checks():
    h = torch.zeros(4, 64, dtype=torch.float16)
    w = torch.zeros(8, 64, dtype=torch.float16)
    with pytest.raises(ValueError, match="hidden"):
        moe.gate(h.float(), w, 2)
    with pytest.raises(ValueError, match="w_gate"):
        moe.gate(h, torch.zeros(64, 8, dtype=torch.float16).t(), 2)  # transposed view: not contiguous
    with pytest.raises(ValueError, match="w_gate"):
        moe.gate(h, torch.zeros(8, 32, dtype=torch.float16), 2)
    with pytest.raises(ValueError, match="w_shared_gate"):
        moe.gate(h, w, 2, w_shared_gate=torch.zeros(32, dtype=torch.float16))
    with pytest.raises(ValueError, match="hidden"):
        moe.gate(h[:, ::2], w, 2)
