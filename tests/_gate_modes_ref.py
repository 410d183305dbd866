"""CPU reference of the router's other routing rules (mxmoe_moe_gate_ex, include/mxmoe_moe.h): sigmoid
scores with a selection bias, group-limited top-k and a scaling factor on the weights. numpy; the
arithmetic runs in the dtype of the values handed in (f64 from the f64 logits, or f32 on a kernel's
own f32 scores, where one add for v and one add for a top-2 group sum make the routing exactly
reproducible). Logits, the plain softmax weights and the shared gate are tests/_gate_ref.py's.

Tie rule everywhere: stable sorts on the negated value, so among equal values (-0 == +0) the lower
index wins - for experts and for groups.
"""
from __future__ import annotations

import numpy as np

from tests import _gate_ref as ref


def selection_values(scores: np.ndarray, e_bias=None) -> np.ndarray:
    """v = s + bias, one add in the scores' dtype."""
    s = np.asarray(scores)
    return s if e_bias is None else s + np.asarray(e_bias).astype(s.dtype)[None, :]


def group_scores(v: np.ndarray, n_group: int, group_top: int) -> np.ndarray:
    """[T, n_group]: a group's largest v, or the sum (one add) of its two largest."""
    T, E = v.shape
    g = -np.sort(-(v + v.dtype.type(0)).reshape(T, n_group, E // n_group), axis=2)
    return g[:, :, 0] if group_top == 1 else g[:, :, 0] + g[:, :, 1]


def kept_groups(v: np.ndarray, n_group: int, topk_group: int, group_top: int) -> np.ndarray:
    """bool [T, n_group]: the topk_group groups with the largest score, ties to the lower group."""
    gsc = group_scores(v, n_group, group_top)
    order = np.argsort(-(gsc + gsc.dtype.type(0)), axis=1, kind="stable")[:, :topk_group]
    keep = np.zeros(gsc.shape, dtype=bool)
    np.put_along_axis(keep, order, True, axis=1)
    return keep


def select(v: np.ndarray, topk: int, n_group: int = 1, topk_group: int = 1, group_top: int = 1) -> np.ndarray:
    """ids int32 [T, topk]: descending v among the kept groups' experts, ties by ascending index.
    Experts of dropped groups are never selected (the -inf fill)."""
    v = np.asarray(v)
    T, E = v.shape
    w = v + v.dtype.type(0)
    if n_group > 1:
        keep = np.repeat(kept_groups(v, n_group, topk_group, group_top), E // n_group, axis=1)
        w = np.where(keep, w, -np.inf).astype(v.dtype)
    return np.argsort(-w, axis=1, kind="stable")[:, :topk].astype(np.int32)


def sigmoid_weights(scores: np.ndarray, ids: np.ndarray, renormalize: bool, routed_scale: float) -> np.ndarray:
    """f64: the unbiased scores of the chosen experts, over their sum + 1e-20 with renormalize, times the
    scaling factor."""
    sel = np.take_along_axis(np.asarray(scores, dtype=np.float64), ids.astype(np.int64), axis=1)
    if renormalize:
        sel = sel / (sel.sum(axis=1, keepdims=True) + 1e-20)
    return sel * float(routed_scale)


def gate(hidden, w_gate, topk, *, scoring="softmax", e_bias=None, n_group=1, topk_group=1, group_top=None,
         renormalize=False, routed_scale=1.0, logits=None):
    """(ids int32 [T, topk], weights f64 [T, topk], scores f64 [T, E] or None, logits f64 [T, E]), all in f64;
    ``logits``: use these instead of the f64 GEMM."""
    x = ref.logits_f64(hidden, w_gate) if logits is None else np.asarray(logits, dtype=np.float64)
    if group_top is None:
        group_top = 2 if scoring == "sigmoid" and n_group > 1 else 1
    if scoring == "softmax":
        assert e_bias is None and group_top == 1
        ids = select(x, topk, n_group, topk_group, 1)
        return ids, ref.weights(x, ids, renormalize) * float(routed_scale), None, x
    s = ref.sigmoid(x)
    ids = select(selection_values(s, e_bias), topk, n_group, topk_group, group_top)
    return ids, sigmoid_weights(s, ids, renormalize, routed_scale), s, x


def decision_margins(v: np.ndarray, topk: int, n_group: int = 1, topk_group: int = 1, group_top: int = 1):
    """(expert margin [T], group margin [T]) of the routing of v: the smallest gap between adjacent v
    among the top-(topk + 1) experts of the kept groups (so the order of the chosen ones and the
    boundary to the first one left out), and the gap between the last kept and the first dropped
    group score (+inf when every group is kept)."""
    v = np.asarray(v, dtype=np.float64)
    T, E = v.shape
    w = v
    gm = np.full(T, np.inf)
    if n_group > 1:
        keep = np.repeat(kept_groups(v, n_group, topk_group, group_top), E // n_group, axis=1)
        w = np.where(keep, v, -np.inf)
        if topk_group < n_group:
            gsc = -np.sort(-group_scores(v, n_group, group_top), axis=1)
            gm = gsc[:, topk_group - 1] - gsc[:, topk_group]
    top = -np.sort(-w, axis=1)[:, :topk + 1]
    top = np.where(np.isfinite(top), top, np.nan)  # fewer than topk + 1 kept experts: no boundary
    em = np.nanmin(top[:, :-1] - top[:, 1:], axis=1)
    return em, gm


# a sigmoid score's absolute error bound against the f64 sigmoid of the same logit: the relative bound
# _gate_ref.SOFTMAX_RTOL derives for this arithmetic (exp2, rcp, the rounded argument) times s < 1,
# rounded up with the bias add's half ulp (6e-8)
SCORE_ABS_ERR = 1e-4
EXPERT_MARGIN = 2 * SCORE_ABS_ERR  # two neighbouring v, one such error each
GROUP_MARGIN = 4 * SCORE_ABS_ERR   # two top-2 sums, two such errors each


def onehot_data(T: int, E: int, seed: int, H: int = 64):
    """By-construction inputs: hidden = the first T rows of the H x H identity, so the logits table
    is w_gate[:, :T] transposed, exactly. Row t of the table is a permutation of linspace(-3, 3, E)
    rounded to fp16 (all T permutations are drawn first, then the bias); the bias is integers in
    [-64, 64] / 256. Returns (hidden fp16 [T, H], w_gate fp16 [E, H], e_bias f32 [E])."""
    assert T <= H
    rng = np.random.default_rng(seed)
    vals = np.linspace(-3.0, 3.0, E).astype(np.float16)
    table = np.stack([rng.permutation(vals) for _ in range(T)])
    w = np.zeros((E, H), dtype=np.float16)
    w[:, :T] = table.T
    hidden = np.eye(H, dtype=np.float16)[:T]
    return hidden, w, bias_data(E, rng)


def bias_data(E: int, rng) -> np.ndarray:
    """Integers in [-64, 64] / 256 as f32."""
    return (rng.integers(-64, 65, size=E) / 256.0).astype(np.float32)


# (T, E, topk, n_group, topk_group) of the by-construction cases, their seed, and the rows whose
# margins may fall short: at most 20 % (tests/test_gate_modes.py asserts it on the CPU)
ONEHOT_CASES = [(64, 256, 8, 8, 4), (48, 160, 6, 8, 3), (40, 64, 6, 1, 1)]
ONEHOT_SEED = 1
ONEHOT_MAX_DROPPED = 0.2


def onehot_rows(T, E, topk, n_group, topk_group, seed=ONEHOT_SEED):
    """The case's data, its f64 reference and the bool [T] mask of the rows whose margins suffice."""
    hidden, w, bias = onehot_data(T, E, seed)
    group_top = 2 if n_group > 1 else 1
    ids, wts, s, x = gate(hidden, w, topk, scoring="sigmoid", e_bias=bias, n_group=n_group, topk_group=topk_group,
                          group_top=group_top, renormalize=True, routed_scale=2.5)
    em, gm = decision_margins(selection_values(s, bias), topk, n_group, topk_group, group_top)
    return (hidden, w, bias), (ids, wts, s, x), (em >= EXPERT_MARGIN) & (gm >= GROUP_MARGIN)
