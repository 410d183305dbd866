"""The router's other routing rules (mxmoe_moe_gate_ex / moe.gate's scoring, e_bias, n_group, topk_group,
group_top, routed_scaling_factor) without a GPU: the numpy reference of tests/_gate_modes_ref.py
against a torch restatement of the public DeepSeek-V3 and DeepSeek-V2 routing code, its tie rules,
the C-ABI's host validation (before any HIP call), the Python argument checks, and the margins of the
by-construction inputs the GPU test compares end to end."""
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


def _hf_noaux_tc(logits, bias, topk, n_group, topk_group, norm_topk_prob, scale):
    """DeepSeek-V3's MoEGate.forward (topk_method "noaux_tc", scoring_func "sigmoid") as published,
    on given logits; its topk calls are sorted=False there (order unspecified), sorted here."""
    T, E = logits.shape
    scores = logits.sigmoid()
    scores_for_choice = scores.view(T, -1) + bias.unsqueeze(0)
    group_scores = scores_for_choice.view(T, n_group, -1).topk(2, dim=-1)[0].sum(dim=-1)
    group_idx = torch.topk(group_scores, k=topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(T, n_group, E // n_group).reshape(T, -1)
    tmp_scores = scores_for_choice.masked_fill(~score_mask.bool(), 0.0)
    topk_idx = torch.topk(tmp_scores, k=topk, dim=-1, sorted=True)[1]
    topk_weight = scores.gather(1, topk_idx)
    if topk > 1 and norm_topk_prob:
        topk_weight = topk_weight / (topk_weight.sum(dim=-1, keepdim=True) + 1e-20)
    return topk_idx, topk_weight * scale, tmp_scores


def _hf_group_limited_greedy(logits, topk, n_group, topk_group, scale):
    """DeepSeek-V2's MoEGate.forward (topk_method "group_limited_greedy", softmax scores, no
    norm_topk_prob) as published, on given logits; sorted as above."""
    T, E = logits.shape
    scores = logits.softmax(dim=-1)
    group_scores = scores.view(T, n_group, -1).max(dim=-1).values
    group_idx = torch.topk(group_scores, k=topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    score_mask = group_mask.unsqueeze(-1).expand(T, n_group, E // n_group).reshape(T, -1)
    tmp_scores = scores.masked_fill(~score_mask.bool(), 0.0)
    topk_weight, topk_idx = torch.topk(tmp_scores, k=topk, dim=-1, sorted=True)
    return topk_idx, topk_weight * scale, tmp_scores


@pytest.mark.parametrize("E,k,n_group,topk_group", [(256, 8, 8, 4), (64, 6, 1, 1)])
def test_reference_matches_deepseek_v3(E, k, n_group, topk_group):
    T, H = 64, 128
    hidden, w = ref.random_data(T, H, E, seed=11)
    bias = mref.bias_data(E, np.random.default_rng(12))
    group_top = 2 if n_group > 1 else 1
    ids, wts, s, x = mref.gate(hidden, w, k, scoring="sigmoid", e_bias=bias, n_group=n_group, topk_group=topk_group,
                               group_top=group_top, renormalize=True, routed_scale=2.5)
    v = mref.selection_values(s, bias)
    # the inputs: every chosen v is positive, so the published 0.0 fill and the -inf fill agree, and
    # every decision (group boundary, the order of the chosen experts, the boundary behind them) has a margin
    assert (np.take_along_axis(v, ids.astype(np.int64), axis=1) > 0).all()
    em, gm = mref.decision_margins(v, k, n_group, topk_group, group_top)
    assert (em > 1e-9).all() and (gm > 1e-9).all()
    if n_group == 1:  # GLM-4.5-style: one group, where the published group stage keeps everything
        n_group_t, topk_group_t = 1, 1
    else:
        n_group_t, topk_group_t = n_group, topk_group
    ti, tw, _ = _hf_noaux_tc(torch.from_numpy(x), torch.from_numpy(bias.astype(np.float64)), k, n_group_t, topk_group_t,
                             True, 2.5)
    assert (ids == ti.numpy()).all()
    assert np.abs(wts - tw.numpy()).max() <= 1e-12
    plain = ref.select(x, k)
    assert (np.sort(ids, axis=1) != np.sort(plain, axis=1)).any(), "the bias / the groups must change some row's routing"


def test_reference_matches_deepseek_v2():
    T, H, E, k, n_group, topk_group = 64, 128, 160, 6, 8, 3
    hidden, w = ref.random_data(T, H, E, seed=13)
    ids, wts, s, x = mref.gate(hidden, w, k, n_group=n_group, topk_group=topk_group, routed_scale=16.0)
    assert s is None
    ti, tw, tmp = _hf_group_limited_greedy(torch.from_numpy(x), k, n_group, topk_group, 16.0)
    assert (tmp.gather(1, ti) > 0).all()  # every chosen probability is positive: the two fills agree
    em, gm = mref.decision_margins(x, k, n_group, topk_group, 1)
    assert (em > 1e-9).all() and (gm > 1e-9).all()
    assert (ids == ti.numpy()).all()
    assert np.abs(wts - tw.numpy()).max() <= 1e-12
    assert (np.sort(ids, axis=1) != np.sort(ref.select(x, k), axis=1)).any()


@pytest.mark.parametrize("model", ["ds3", "ds2_full"])
def test_bench_composite_routes_as_the_reference(model):
    """moe_bench.gate_composite (gate_bench's yardstick for the two new models) on the CPU, small T."""
    m = GATE_MODELS[model]
    E, k, routing = m["E"], m["topk"], dict(m["routing"])
    hidden, w = ref.random_data(32, 128, E, seed=14)
    x = ref.logits_f64(hidden, w)
    bias = mref.bias_data(E, np.random.default_rng(15)) if m.get("bias") else None
    renorm = bool(m.get("renormalize", False))
    scale = routing.pop("routed_scaling_factor")
    ids, wts, _, _ = mref.gate(hidden, w, k, e_bias=bias, renormalize=renorm, routed_scale=scale, **routing)
    ti, tw = gate_composite(torch.from_numpy(x), k, renorm, None if bias is None else torch.from_numpy(bias).double(),
                                routed_scaling_factor=scale, **routing)
    assert ti.dtype == torch.int32 and (ids == ti.numpy()).all()
    assert np.abs(wts - tw.numpy()).max() <= 1e-12 * scale


def test_reference_tie_rules():
    # equal group scores: the lower group wins; equal v: the lower index; inside the kept groups only
    v = np.zeros((1, 16))
    assert mref.select(v, 3, n_group=4, topk_group=2, group_top=2).tolist() == [[0, 1, 2]]
    assert mref.select(v, 6, n_group=4, topk_group=2, group_top=1).tolist() == [[0, 1, 2, 3, 4, 5]]
    v = np.zeros((1, 16))
    v[0, [6, 14]] = 1.0  # groups 1 and 3 tie above groups 0 and 2, which tie too
    assert mref.kept_groups(v, 4, 3, 1).tolist() == [[True, True, False, True]]
    assert mref.select(v, 4, n_group=4, topk_group=3, group_top=1).tolist() == [[6, 14, 0, 1]]
    # -0 == +0, for experts and for group scores
    v = np.array([[-0.0, 0.0, -1.0, -1.0, 0.0, -0.0, -1.0, -1.0]])
    assert mref.select(v, 2, n_group=2, topk_group=1, group_top=1).tolist() == [[0, 1]]
    assert mref.select(v, 2, n_group=2, topk_group=1, group_top=2).tolist() == [[0, 1]]
    # top-2 sums: group 1 holds the largest v, group 0 the largest sum
    v = np.array([[0.6, 0.6, 0.0, 0.0, 0.9, 0.1, 0.0, 0.0]])
    assert mref.select(v, 1, n_group=2, topk_group=1, group_top=1).tolist() == [[4]]
    assert mref.select(v, 1, n_group=2, topk_group=1, group_top=2).tolist() == [[0]]
    # groups of 20 straddle the 16-column blocks: experts 20-39 are group 1
    v = np.zeros((1, 160), dtype=np.float32)
    v[0, 39] = 2.0
    v[0, 40] = 1.0
    v[0, 20] = 0.5
    assert mref.kept_groups(v, 8, 2, 2).tolist() == [[False, True, True] + [False] * 5]
    assert mref.select(v, 4, n_group=8, topk_group=2, group_top=2).tolist() == [[39, 40, 20, 21]]
    # a dropped group's expert is never selected, even above every kept v (the -inf fill, not 0.0)
    v = np.array([[-0.1, -0.2, -0.3, -0.4, -0.9, 0.05, -0.9, -0.9]])
    assert mref.select(v, 2, n_group=2, topk_group=1, group_top=2).tolist() == [[0, 1]]
    # weights: the unbiased scores, renormalised over the chosen ones, scaled
    s = np.array([[0.5, 0.25, 0.125, 0.125]])
    ids = np.array([[0, 1]], dtype=np.int32)
    assert mref.sigmoid_weights(s, ids, False, 2.0).tolist() == [[1.0, 0.5]]
    assert np.abs(mref.sigmoid_weights(s, ids, True, 3.0) - [[2.0, 1.0]]).max() <= 1e-15


def _call(hidden=16, w_gate=16, w_sg=None, T=4, H=64, E=64, topk=4, renorm=0, scoring=1, e_bias=None, n_group=4,
          topk_group=2, group_top=2, routed_scale=1.0, ids=16, wts=16, shared_w=None, logits=None, scores=None):
    st = nat.lib().mxmoe_moe_gate_ex(hidden, w_gate, w_sg, T, H, E, topk, renorm, scoring, e_bias, n_group, topk_group,
                                     group_top, routed_scale, ids, wts, shared_w, logits, scores, None)
    return st, nat.lib().mxmoe_gg_last_error()


@pytest.mark.parametrize("kw", [
    dict(E=60, n_group=8),                       # E % n_group != 0
    dict(E=24, n_group=4),                       # gs = 6
    dict(E=72, n_group=9, topk_group=2),         # n_group = 9
    dict(n_group=0), dict(topk_group=5), dict(topk_group=0), dict(n_group=1, topk_group=2),
    dict(E=32, n_group=8, topk_group=1, topk=5, group_top=1),  # topk > topk_group * gs
    dict(scoring=0, group_top=1, e_bias=16),     # softmax with a bias
    dict(scoring=0, group_top=2),                # softmax with group_top 2
    dict(scoring=0, group_top=1, scores=16),     # softmax with a scores output
    dict(group_top=3), dict(group_top=0),
    dict(routed_scale=float("nan")), dict(routed_scale=float("inf")), dict(routed_scale=float("-inf")),
    dict(scoring=2), dict(scoring=-1),
    dict(e_bias=18), dict(scores=6),             # misaligned
    # and what mxmoe_moe_gate refuses
    dict(E=257, n_group=1, topk_group=1), dict(topk=0), dict(topk=17), dict(H=48), dict(T=-1), dict(hidden=8),
    dict(w_sg=16), dict(shared_w=16),
], ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_abi_validation_before_any_hip_call(kw):
    """Dummy (never dereferenced) pointers: every bad argument is refused on the host."""
    st, err = _call(**kw)
    assert st == nat.MXMOE_GG_ERR_INVALID
    assert err and b"mxmoe_moe_gate_ex" in err


def test_abi_empty_batch_is_ok():
    assert _call(T=0)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, hidden=None, w_gate=None, ids=None, wts=None)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, e_bias=16, scores=16, logits=16, w_sg=16, shared_w=16, routed_scale=2.5)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, E=160, topk=6, n_group=8, topk_group=3, scoring=0, group_top=1, routed_scale=16.0)[0] == nat.MXMOE_GG_OK
    assert _call(T=0, n_group=1, topk_group=1, group_top=1)[0] == nat.MXMOE_GG_OK
    assert "mxmoe_moe_gate_ex" in nat.EXPORTED_SYMBOLS
    assert nat.lib().mxmoe_moe_gate_ex.argtypes[3] is ctypes.c_int64
    assert nat.lib().mxmoe_moe_gate_ex.argtypes[13] is ctypes.c_float
    assert nat.lib().mxmoe_gg_abi_version() == 7


def test_gate_argument_checks():
    h = torch.zeros(4, 64, dtype=torch.float16)
    w = torch.zeros(64, 64, dtype=torch.float16)
    b = torch.zeros(64, dtype=torch.float32)
    bad = [
        dict(scoring="tanh"), dict(n_group=9), dict(n_group=3), dict(n_group=16), dict(n_group=4, topk_group=5),
        dict(n_group=1, topk_group=2), dict(n_group=8, topk_group=1, scoring="sigmoid"),  # topk 10 > 8 experts kept
        dict(e_bias=b), dict(group_top=2), dict(return_scores=True),                      # softmax takes none of them
        dict(scoring="sigmoid", group_top=3), dict(scoring="sigmoid", e_bias=b.double()),
        dict(scoring="sigmoid", e_bias=b[:32]), dict(scoring="sigmoid", e_bias=torch.zeros(128)[::2]),
        dict(routed_scaling_factor=float("nan")), dict(routed_scaling_factor=float("inf")),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            moe.gate(h, w, 10, **kw)
    with pytest.raises(ValueError, match="hidden"):
        moe.gate(h.float(), w, 2, scoring="sigmoid")
    with pytest.raises(ValueError, match="out must hold 5"):
        moe.gate(h, w, 2, scoring="sigmoid", return_logits=True, return_scores=True, out=(None,) * 4)
    assert moe.gate_routing_args(64, 6, "sigmoid", b, 8, 3) == (2, False)
    assert moe.gate_routing_args(64, 6, "sigmoid", b) == (1, False)
    assert moe.gate_routing_args(64, 6, "softmax", None, 8, 3, None, 16.0) == (1, False)
    assert moe.gate_routing_args(64, 6) == (1, True)
    assert moe.gate_routing_args(64, 6, routed_scaling_factor=2.0) == (1, False)


class _FFN:  # what MoEBlock reads of a MoEFFN before any launch
    E, H, has_shared = 64, 64, False


def test_moe_block_argument_checks():
    w = torch.zeros(64, 64, dtype=torch.float16)
    b = torch.zeros(64, dtype=torch.float32)
    for kw in (dict(scoring="tanh"), dict(n_group=3), dict(n_group=4, topk_group=5), dict(e_bias=b), dict(group_top=2),
               dict(scoring="sigmoid", group_top=3), dict(scoring="sigmoid", e_bias=b[:8]),
               dict(routed_scaling_factor=float("nan")), dict(n_group=8, topk_group=1)):
        with pytest.raises(ValueError):
            moe.MoEBlock(_FFN(), w, 10, **kw)
    blk = moe.MoEBlock(_FFN(), w, 8, renormalize=True, scoring="sigmoid", e_bias=b, n_group=8, topk_group=4,
                       routed_scaling_factor=2.5)
    assert blk.routing["scoring"] == "sigmoid" and blk.routing["n_group"] == 8 and blk.routing["e_bias"] is not None


@pytest.mark.parametrize("case", mref.ONEHOT_CASES, ids=str)
def test_by_construction_inputs_keep_their_margins(case):
    """The rows the GPU test may leave out (a v gap below 2e-4 or a group-score gap below 4e-4 in the
    f64 reference) are at most 20 % of the rows, the logits are exact in fp16 and the routing differs
    from a plain top-k of the logits in every row: asserted here so the GPU test cannot hide behind it."""
    T, E, k, n_group, topk_group = case
    (hidden, w, bias), (ids, wts, s, x), ok = mref.onehot_rows(*case)
    assert (x == w.astype(np.float64)[:, :T].T).all()  # the logits table is w_gate transposed, exactly
    assert (np.sort(x, axis=1) == np.sort(np.linspace(-3.0, 3.0, E).astype(np.float16).astype(np.float64))[None, :]).all()
    assert (np.abs(bias * 256 - np.rint(bias * 256)) == 0).all() and np.abs(bias).max() <= 0.25
    dropped = int((~ok).sum())
    print(f"{case}: {dropped} of {T} rows left out")
    assert dropped <= mref.ONEHOT_MAX_DROPPED * T
    assert (np.sort(ids, axis=1) != np.sort(ref.select(x, k), axis=1)).any(axis=1).all()
    em, gm = mref.decision_margins(mref.selection_values(s, bias), k, n_group, topk_group, 2 if n_group > 1 else 1)
    assert (em[ok] >= mref.EXPERT_MARGIN).all() and (gm[ok] >= mref.GROUP_MARGIN).all()
