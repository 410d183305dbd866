"""CPU reference of the router (mxmoe_moe_gate, include/mxmoe_moe.h), numpy in f64, and the data
generators the router's tests share.

logits = hidden @ w_gate.T; selection = the topk largest logits, a stable sort on (-logit, index) so
the lower index wins among equal logits; weights = softmax over all E experts at the chosen ids, or
over the chosen ones (renormalize); shared gate = sigmoid(hidden @ w_shared_gate).
"""
from __future__ import annotations

import numpy as np

# |w - ref| <= SOFTMAX_RTOL * ref + 2^-126 for weights and shared_w against the f64 softmax / sigmoid
# of the same f32 logits. Derived, not measured: hardware exp2 and rcp about 1 ulp each (1.2e-7);
# the argument (x - m) * log2(e), rounded at magnitude up to 126 before the result flushes, moves the
# exponential by 126 * 2^-24 * ln 2 ~ 5e-6; a sum of up to 256 non-negative f32 terms in any order
# at most 256 * 2^-24 ~ 1.5e-5; doubled for numerator over denominator and rounded up. The absolute
# part covers a selected probability below the smallest normal f32, which flushes to zero.
SOFTMAX_RTOL = 4e-5
SOFTMAX_ATOL = 2.0 ** -126


def logits_f64(hidden: np.ndarray, w_gate: np.ndarray) -> np.ndarray:
    return hidden.astype(np.float64) @ w_gate.astype(np.float64).T


def select(logits: np.ndarray, topk: int) -> np.ndarray:
    """ids [T, topk] int32: descending logit, ties by ascending index (-0 == +0)."""
    x = np.asarray(logits, dtype=np.float64)
    order = np.argsort(-x, axis=1, kind="stable")  # stable: equal keys keep ascending index
    return order[:, :topk].astype(np.int32)


def weights(logits: np.ndarray, ids: np.ndarray, renormalize: bool) -> np.ndarray:
    x = np.asarray(logits, dtype=np.float64)
    p = np.exp(x - x.max(axis=1, keepdims=True))
    sel = np.take_along_axis(p, ids.astype(np.int64), axis=1)
    den = sel.sum(axis=1, keepdims=True) if renormalize else p.sum(axis=1, keepdims=True)
    return sel / den


def sigmoid(s: np.ndarray) -> np.ndarray:
    return 1.0 / (1.0 + np.exp(-np.asarray(s, dtype=np.float64)))


def gate(hidden: np.ndarray, w_gate: np.ndarray, topk: int, renormalize: bool = False, w_shared_gate=None,
         logits=None):
    """(ids int32 [T, topk], weights f64 [T, topk], shared_w f64 [T] or None, logits f64 [T, E]);
    ``logits``: use these (e.g. a kernel's own f32 logits) instead of the f64 GEMM."""
    x = logits_f64(hidden, w_gate) if logits is None else np.asarray(logits, dtype=np.float64)
    ids = select(x, topk)
    sw = None if w_shared_gate is None else sigmoid(hidden.astype(np.float64) @ w_shared_gate.astype(np.float64))
    return ids, weights(x, ids, renormalize), sw, x


def softmax_close(got: np.ndarray, ref: np.ndarray) -> tuple[bool, float]:
    """(all within the softmax tolerance, worst |got - ref| / ref over entries with ref above the
    absolute part) — the second for the message of a failing assertion."""
    got = np.asarray(got, dtype=np.float64)
    err = np.abs(got - ref)
    big = ref > 1e-30
    worst = float((err[big] / ref[big]).max()) if big.any() else 0.0
    return bool((err <= SOFTMAX_RTOL * ref + SOFTMAX_ATOL).all()), worst


def exact_data(T: int, H: int, E: int, seed: int = 0, shared: bool = False):
    """hidden: integers in [-2, 2]; w_gate (and the shared gate): integers in [-2, 2] times 2^-6, as
    fp16. Every product is a multiple of 2^-6 and every partial sum is at most H * 4 * 2^-6 <= 128
    (H <= 2048), so an f32 accumulation in any order is exact and equals the f64 logits bit for bit."""
    rng = np.random.default_rng(seed)
    hidden = rng.integers(-2, 3, size=(T, H)).astype(np.float16)
    w = (rng.integers(-2, 3, size=(E, H)) * 2.0 ** -6).astype(np.float16)
    sg = (rng.integers(-2, 3, size=(H,)) * 2.0 ** -6).astype(np.float16) if shared else None
    return hidden, w, sg


def random_data(T: int, H: int, E: int, seed: int = 0):
    """fp16 normal hidden, w_gate ~ N(0, 1/H)."""
    rng = np.random.default_rng(seed)
    hidden = rng.standard_normal((T, H)).astype(np.float16)
    w = (rng.standard_normal((E, H)) * H ** -0.5).astype(np.float16)
    return hidden, w
