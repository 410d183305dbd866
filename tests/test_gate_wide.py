"""The router for more than 256 experts (mxmoe_moe_gate_wide, moe.gate / moe.MoEBlock with E > 256) without a GPU:
the C ABI's host validation (before any HIP call), the Python argument checks, the margins of the by-construction
inputs the GPU test compares end to end, and the bench's torch composite on the two new models."""
from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.moe_bench import GATE_MODELS, gate_composite
from tests import _gate_modes_ref as mref
from tests import _gate_ref as ref
from tests import _gate_wide_ref as wref


def _call(hidden=16, w_gate=16, w_sg=None, T=4, H=64, E=384, topk=8, renorm=1, scoring=1, e_bias=None, n_group=1,
          topk_group=1, group_top=1, routed_scale=1.0, logit_bias=None, ids=16, wts=16, shared_w=None, logits=None,
          scores=None):
    st = nat.symbol("mxmoe_moe_gate_wide")(hidden, w_gate, w_sg, T, H, E, topk, renorm, scoring, e_bias, n_group,
                                          topk_group, group_top, routed_scale, logit_bias, ids, wts, shared_w, logits,
                                          scores, None)
    return st, nat.lib().mxmoe_gg_last_error()


@pytest.mark.parametrize("kw", [
    dict(E=0), dict(E=513), dict(E=1024),
    dict(E=384, n_group=2), dict(E=384, n_group=2, topk_group=2), dict(E=512, n_group=8, topk_group=4, group_top=2),
    dict(E=384, topk_group=2), dict(E=384, group_top=2),
    dict(topk=17), dict(topk=0), dict(H=48), dict(T=-1),
    dict(hidden=8), dict(logit_bias=18), dict(e_bias=18), dict(scores=6),
    dict(w_sg=16), dict(shared_w=16),
    dict(scoring=0, e_bias=16), dict(scoring=0, scores=16), dict(scoring=2), dict(routed_scale=float("nan")),
    # E <= 256 is mxmoe_moe_gate_ex2's path: its refusals, under this entry point's name
    dict(E=64, topk=17), dict(E=60, n_group=8), dict(E=64, n_group=4, topk_group=5), dict(E=256, H=48),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_abi_validation_before_any_hip_call(kw):
    """Dummy (never dereferenced) pointers: every bad argument is refused on the host."""
    st, err = _call(**kw)
    assert st == nat.MXMOE_GG_ERR_INVALID
    assert err and b"mxmoe_moe_gate_wide" in err


def test_abi_empty_batch_is_ok():
    assert _call(T=0)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, hidden=None, w_gate=None, ids=None, wts=None)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, E=512, topk=10, scoring=0, w_sg=16, shared_w=16, logits=16, logit_bias=16)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, E=257, topk=16, e_bias=16, scores=16, routed_scale=2.827)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, E=256, topk=8, n_group=8, topk_group=4, group_top=2)[0] == nat.MXMOE_GG_OK  # groups: E <= 256
    assert "mxmoe_moe_gate_wide" in nat.EXPORTED_SYMBOLS
    fn = nat.lib().mxmoe_moe_gate_wide
    assert fn.argtypes == nat.lib().mxmoe_moe_gate_ex2.argtypes and fn.argtypes[3] is ctypes.c_int64
    assert nat.lib().mxmoe_gg_abi_version() == 7


def test_older_entry_points_keep_their_limit():
    lib = nat.lib()
    st = lib.mxmoe_moe_gate_ex2(16, 16, None, 4, 64, 384, 8, 1, 1, None, 1, 1, 1, 1.0, None, 16, 16, None, None, None, None)
    assert st == nat.MXMOE_GG_ERR_INVALID and b"mxmoe_moe_gate_ex2" in lib.mxmoe_gg_last_error()
    st = lib.mxmoe_moe_gate(16, 16, None, 4, 64, 384, 8, 1, 16, 16, None, None, None)
    assert st == nat.MXMOE_GG_ERR_INVALID and b"mxmoe_moe_gate" in lib.mxmoe_gg_last_error()


def test_gate_argument_checks():
    h = torch.zeros(4, 64, dtype=torch.float16)
    w = torch.zeros(384, 64, dtype=torch.float16)
    b = torch.zeros(384, dtype=torch.float32)
    for kw in (dict(n_group=8), dict(n_group=8, topk_group=4, scoring="sigmoid", e_bias=b), dict(n_group=2, topk_group=2),
               dict(topk_group=2), dict(scoring="sigmoid", group_top=2), dict(e_bias=b), dict(scoring="sigmoid", e_bias=b[:256])):
        with pytest.raises(ValueError):
            moe.gate(h, w, 8, **kw)
    with pytest.raises(ValueError, match="512"):
        moe.gate(h, torch.zeros(513, 64, dtype=torch.float16), 8)
    with pytest.raises(ValueError, match="groups"):
        moe.gate_routing_args(384, 8, n_group=8, topk_group=4)
    assert moe.gate_routing_args(384, 8, "sigmoid", b, routed_scaling_factor=2.827) == (1, False)
    assert moe.gate_routing_args(512, 10) == (1, True)
    assert moe.gate_routing_args(256, 8, "sigmoid", None, 8, 4) == (2, False)  # 256 experts: groups as before


class _FFN:  # what MoEBlock reads of a MoEFFN before any launch
    E, H, has_shared = 384, 64, False


def test_moe_block_argument_checks():
    w = torch.zeros(384, 64, dtype=torch.float16)
    with pytest.raises(ValueError):
        moe.MoEBlock(_FFN(), w, 8, n_group=8, topk_group=4)
    blk = moe.MoEBlock(_FFN(), w, 8, renormalize=True, scoring="sigmoid", e_bias=torch.zeros(384), routed_scaling_factor=2.827)
    assert blk.routing["scoring"] == "sigmoid" and blk.routing["n_group"] == 1


@pytest.mark.parametrize("case", wref.WIDE_ONEHOT_CASES, ids=str)
def test_by_construction_inputs_keep_their_margins(case):
    """The rows the GPU test may leave out (a v gap below 2e-4 in the f64 reference) are at most 20 % of the rows and
    the logits are exact in fp16: asserted here so the GPU test cannot hide behind it."""
    T, E, k, n_group, topk_group, seed = case
    (hidden, w, bias), (ids, wts, s, x), ok = mref.onehot_rows(T, E, k, n_group, topk_group, seed=seed)
    assert (x == w.astype(np.float64)[:, :T].T).all()  # the logits table is w_gate transposed, exactly
    assert (np.sort(x, axis=1) == np.sort(np.linspace(-3.0, 3.0, E).astype(np.float16).astype(np.float64))[None, :]).all()
    dropped = int((~ok).sum())
    print(f"{case}: {dropped} of {T} rows left out")
    assert dropped <= mref.ONEHOT_MAX_DROPPED * T
    em, _ = mref.decision_margins(mref.selection_values(s, bias), k)
    assert (em[ok] >= mref.EXPERT_MARGIN).all()
    assert (np.sort(ids, axis=1) != np.sort(ref.select(x, k), axis=1)).any(), "the bias must change some row's routing"


@pytest.mark.parametrize("model", ["kimi_k2", "qwen3_next"])
def test_bench_composite_routes_as_the_reference(model):
    """moe_bench.gate_composite (gate_bench's yardstick) on the two models with more than 256 experts, on the CPU at small
    T, on the rows whose f64 margins exceed what f64 rounding in either implementation can move."""
    m = GATE_MODELS[model]
    E, k, routing = m["E"], m["topk"], dict(m["routing"])
    assert E > 256 and routing.get("n_group", 1) == 1
    moe.gate_routing_args(E, k, **{kk: v for kk, v in routing.items()})
    hidden, w = ref.random_data(32, 128, E, seed=14)
    x = ref.logits_f64(hidden, w)
    bias = mref.bias_data(E, np.random.default_rng(15)) if m.get("bias") else None
    renorm = bool(m.get("renormalize", False))
    scale = routing.pop("routed_scaling_factor", 1.0)
    ids, wts, s, _ = mref.gate(hidden, w, k, e_bias=bias, renormalize=renorm, routed_scale=scale, **routing)
    v = x if s is None else mref.selection_values(s, bias)
    em, _ = mref.decision_margins(v, k)
    ok = em > 1e-9
    assert ok.sum() >= 0.9 * len(ok)
    ti, tw = gate_composite(torch.from_numpy(x), k, renorm, None if bias is None else torch.from_numpy(bias).double(),
                                routed_scaling_factor=scale, **routing)
    assert ti.dtype == torch.int32 and (ids[ok] == ti.numpy()[ok]).all()
    assert np.abs(wts[ok] - tw.numpy()[ok]).max() <= 1e-12 * scale
