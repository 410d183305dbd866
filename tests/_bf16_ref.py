"""What the tests of the bf16 layers share (mxmoe_moe_gate_dt, mxmoe_moe_gather_quant, mxmoe_moe_combine_dt of
include/mxmoe_moe.h): bf16 <-> f32 in numpy, the data generators and the bf16 combine reference. The router's
references themselves are tests/_gate_ref.py and tests/_gate_modes_ref.py, unchanged: a bf16 value is an f32 value,
so they take the widened arrays as they are.

Every comparison built on this file is bit for bit. The one named tolerance is _gate_ref.SOFTMAX_RTOL for the
weights against the f64 softmax / sigmoid (its derivation does not depend on the operands' format: it covers the
arithmetic AFTER the logits, which the bf16 builds share with the fp16 ones).
"""
from __future__ import annotations

import numpy as np

from oracle import moe_ref
from tests import _gate_modes_ref as mref
from tests import _gate_ref as ref
from tests import _gate_wide_ref as wref


def bf16_bits(x: np.ndarray) -> np.ndarray:
    """f32 -> bf16 bit patterns (uint16), round to nearest even; NaN stays NaN (quiet)."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, ((b >> 16) | 0x40).astype(np.uint16), r)


def bf16_value(bits: np.ndarray) -> np.ndarray:
    """bf16 bit patterns (uint16) -> the f32 values they denote (exact)."""
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def is_bf16(x: np.ndarray) -> bool:
    """Every value of x survives f32 -> bf16 -> f32 unchanged (bits, so -0 counts)."""
    x32 = np.ascontiguousarray(x, dtype=np.float32)
    return bool((bf16_value(bf16_bits(x32)).view(np.uint32) == x32.view(np.uint32)).all())


def exact_data(T: int, H: int, E: int, seed: int = 0, shared: bool = False):
    """_gate_ref.exact_data widened to f32: integers in [-2, 2] and integers in [-2, 2] * 2^-6 have at most two
    significant bits, so they are bf16 values as they stand (tests/test_bf16_layer.py asserts it)."""
    hidden, w, sg = ref.exact_data(T, H, E, seed=seed, shared=shared)
    return hidden.astype(np.float32), w.astype(np.float32), None if sg is None else sg.astype(np.float32)


RANGE_HIDDEN_SCALE = 2.0 ** 17   # beyond fp16's largest finite value (65504): +-Inf as fp16
RANGE_WEIGHT_SCALE = 2.0 ** -30  # below fp16's smallest subnormal (2^-24): 0 as fp16


def range_data(T: int, H: int, E: int, seed: int = 0):
    """hidden: integers in [-2, 2] times 2^17; w_gate: integers in [-2, 2] times 2^-30 (f32 arrays of bf16 values).
    Every product is an integer in [-4, 4] times 2^-13 and a logit sums at most H <= 2048 of them: a multiple of
    2^-13 of magnitude <= 4 * 2048 * 2^-13 = 1, i.e. at most 14 significant bits — exact in f32 in any order. A
    router that rounded its operands to fp16 would compute Inf * 0."""
    assert H <= 2048
    rng = np.random.default_rng(seed)
    hidden = (rng.integers(-2, 3, size=(T, H)) * RANGE_HIDDEN_SCALE).astype(np.float32)
    w = (rng.integers(-2, 3, size=(E, H)) * RANGE_WEIGHT_SCALE).astype(np.float32)
    return hidden, w


def random_data(T: int, H: int, E: int, seed: int = 0):
    """_gate_ref.random_data's distributions rounded to bf16 (f32 arrays of bf16 values)."""
    rng = np.random.default_rng(seed)
    hidden = bf16_value(bf16_bits(rng.standard_normal((T, H)).astype(np.float32)))
    w = bf16_value(bf16_bits((rng.standard_normal((E, H)) * H ** -0.5).astype(np.float32)))
    return hidden, w


def gather_edge_rows(T: int, K: int, seed: int = 0) -> np.ndarray:
    """bf16 hidden states for the gather (f32 array of bf16 values, no NaN): normal rows, and
      row 0   all zero;
      row 1   -0 in every other column;
      row 2   the fp16-subnormal range: 2^-20 (an exact fp16 subnormal), 3 * 2^-26 (rounds up to 2^-24), 2^-25 (a
              tie: to even, 0), 3 * 2^-25 (a tie: to even, 2^-23), 2^-26 (rounds to 0), with both signs;
      row 3   1e5 (as bf16: 99840) and its negative: beyond fp16, +-Inf on both sides."""
    rng = np.random.default_rng(seed)
    x = bf16_value(bf16_bits(rng.standard_normal((T, K)).astype(np.float32)))
    x[0] = 0.0
    x[1, 0::2] = -0.0
    sub = np.array([2.0 ** -20, 3 * 2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26], dtype=np.float32)
    x[2, :10] = np.concatenate([sub, -sub])
    x[2, 64:74] = np.concatenate([-sub, sub])
    big = bf16_value(bf16_bits(np.array([1e5], dtype=np.float32)))[0]
    x[3, 5] = big
    x[3, K - 3] = -big
    assert is_bf16(x) and not np.isnan(x).any()
    return x


# The by-construction cases of the biased routing rules, (T, E, topk, n_group, topk_group, seed, H):
# _gate_modes_ref.ONEHOT_CASES[0] (DeepSeek-V3's rule: groups 8 / 4, on gate_modes_kernel) and
# _gate_wide_ref.WIDE_ONEHOT_CASES[0] (Kimi-K2's: 384 experts, on gate_wide_kernel), at the H of the parity table.
ONEHOT_CASES = [mref.ONEHOT_CASES[0] + (mref.ONEHOT_SEED, 256), wref.WIDE_ONEHOT_CASES[0] + (128,)]


def onehot_rows(T, E, topk, n_group, topk_group, seed, H):
    """_gate_modes_ref.onehot_rows with the logits table rounded to bf16 (linspace(-3, 3, E) as fp16 is no bf16 value;
    every bf16 value of that range is an fp16 value, so the rounded table is exact in both formats): the data as f32
    arrays of bf16 values, the f64 reference on the rounded table — sigmoid scores, e_bias, renormalised, factor 2.5 —
    and the bool [T] mask of the rows whose margins suffice, recomputed for the rounded table (rounding moves
    neighbouring values together, so the mask is not the fp16 table's). The cap on the rows left out stays
    _gate_modes_ref.ONEHOT_MAX_DROPPED; tests/test_bf16_layer.py asserts it."""
    hidden, w, bias = mref.onehot_data(T, E, seed, H)
    hidden = hidden.astype(np.float32)
    w = bf16_value(bf16_bits(w.astype(np.float32)))
    group_top = 2 if n_group > 1 else 1
    ids, wts, s, x = mref.gate(hidden, w, topk, scoring="sigmoid", e_bias=bias, n_group=n_group, topk_group=topk_group,
                               group_top=group_top, renormalize=True, routed_scale=2.5)
    em, gm = mref.decision_margins(mref.selection_values(s, bias), topk, n_group, topk_group, group_top)
    return (hidden, w, bias), (ids, wts, s, x), (em >= mref.EXPERT_MARGIN) & (gm >= mref.GROUP_MARGIN)


def combine_acc(y: np.ndarray, inv: np.ndarray, sorted_e, w: np.ndarray, topk: int, bias=None, E: int = 0, shared=None,
                shared_w=None, shared_bias=None) -> np.ndarray:
    """The combine's f32 accumulator (include/mxmoe_moe.h, mxmoe_moe_combine_bias): acc = +0, then for k in order
    acc = fma(w[t][k], f32(y[slot]) + f32(bias[e]), acc) (the add first; no bias, or an e outside [0, E): no add),
    then fma(ws, f32(shared) + f32(shared_bias), acc). oracle.moe_ref.fma_f32 asserts each fma is exactly one
    rounding."""
    T = w.shape[0]
    acc = np.zeros((T, y.shape[1]), np.float32)
    slots = inv.reshape(T, topk)
    for k in range(topk):
        slot = slots[:, k]
        term = y[slot].astype(np.float32)
        if bias is not None:
            e = sorted_e[slot]
            ok = (e >= 0) & (e < E)
            term = np.where(ok[:, None], term + bias[np.clip(e, 0, E - 1)].astype(np.float32), term)
        acc = moe_ref.fma_f32(w[:, k:k + 1].astype(np.float32), term, acc)
    if shared is not None:
        sw = np.ones((T, 1), np.float32) if shared_w is None else shared_w.reshape(T, 1).astype(np.float32)
        term = shared.astype(np.float32)
        if shared_bias is not None:
            term = term + shared_bias.astype(np.float32)[None, :]
        acc = moe_ref.fma_f32(sw, term, acc)
    return acc


def combine_bf16(*args, **kw) -> np.ndarray:
    """combine_acc rounded once to bf16, to nearest even: the bits (uint16) of mxmoe_moe_combine_dt's bf16 output."""
    return bf16_bits(combine_acc(*args, **kw))
