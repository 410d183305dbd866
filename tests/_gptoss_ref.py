"""Numpy restatements of the gpt-oss layer arithmetic (include/mxmoe_moe.h: mxmoe_moe_glu_quant,
mxmoe_moe_combine_bias, mxmoe_moe_gate_ex2's logit bias) — TEST INFRASTRUCTURE ONLY.

Everything is f32 as the kernels compute it, with libm's exp where the GPU uses the hardware exp2 / reciprocal
(oracle/moe_ref.py's convention for the SiLU pass: at most 1 fp16 ulp / one code step apart after rounding). The
semantics are the public model code: transformers' GptOssExperts._apply_gate and GptOssTopKRouter
(tests/test_gptoss.py pins this file to them).
"""
from __future__ import annotations

import numpy as np

from oracle import moe_ref

ALPHA, LIMIT = 1.702, 7.0


def add_bias(x: np.ndarray, b) -> np.ndarray:
    """f32(x) + f32(b): one IEEE f32 add per element; b None: no add."""
    x = x.astype(np.float32)
    return x if b is None else x + np.asarray(b).astype(np.float32)


def silu_mul_f32(g: np.ndarray, u: np.ndarray) -> np.ndarray:
    """oracle/moe_ref.silu_mul's expression on f32 gate / up values."""
    with np.errstate(over="ignore"):
        s = g / (np.float32(1) + np.exp(-g, dtype=np.float32))
    return s * u


def swiglu_clamp_f32(g: np.ndarray, u: np.ndarray, alpha: float = ALPHA, limit: float = LIMIT) -> np.ndarray:
    """(clamp(u, -limit, limit) + 1) * gc * sigmoid(alpha * gc), gc = min(g, limit), in f32."""
    gc = np.minimum(g, np.float32(limit))
    uc = np.minimum(np.maximum(u, np.float32(-limit)), np.float32(limit))
    with np.errstate(over="ignore"):
        s = gc / (np.float32(1) + np.exp(-(np.float32(alpha) * gc), dtype=np.float32))
    return s * (uc + np.float32(1))


def glu(gu: np.ndarray, bias=None, act: str = "silu", alpha: float = ALPHA, limit: float = LIMIT) -> np.ndarray:
    """fp16 [R, 2N] ([gate | up]) + bias ([2N] or [R, 2N], fp16, [gate | up]; None: no add) -> act fp16 [R, N]."""
    N = gu.shape[1] // 2
    x = add_bias(gu, bias)
    g, u = x[:, :N], x[:, N:]
    a = silu_mul_f32(g, u) if act == "silu" else swiglu_clamp_f32(g, u, alpha, limit)
    return a.astype(np.float16)


def clamp_inputs(gu: np.ndarray, limit: float = LIMIT) -> np.ndarray:
    """The gate_up rows with the clamp already applied (gate from above, up from both sides), in fp16."""
    N = gu.shape[1] // 2
    out = gu.copy()
    out[:, :N] = np.minimum(gu[:, :N], np.float16(limit))
    out[:, N:] = np.clip(gu[:, N:], np.float16(-limit), np.float16(limit))
    return out


def fma_f32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf elementwise. moe_ref.fma_f32 wherever it applies (it asserts that the f64 sum of the exact product and c
    is exact). Here b is an f32 SUM of two fp16 values, up to 24 significant bits instead of 11, so that sum can be
    inexact; then: the product (48 bits) is still exact in f64, TwoSum gives the f64 sum s and its error, and the
    one f32 rounding of s + err differs from that of s only when s lies exactly on an f32 rounding midpoint, where
    the error's sign decides."""
    try:
        return moe_ref.fma_f32(a, b, c)
    except AssertionError:
        pass
    p = a.astype(np.float64) * b.astype(np.float64)
    o = np.broadcast_to(c.astype(np.float64), p.shape)
    s = p + o
    bp = s - o
    err = (p - bp) + (o - (s - bp))
    t = s.astype(np.float32)
    t64 = t.astype(np.float64)
    other = np.nextafter(t, np.where(s > t64, np.float32(np.inf), np.float32(-np.inf))).astype(np.float64)
    tie = (t64 != s) & ((t64 + other) / 2 == s) & (err != 0)
    toward_other = tie & (np.sign(err) == np.sign(other - t64))
    return np.where(toward_other, other, t64).astype(np.float32)


def combine_bias(y: np.ndarray, inv: np.ndarray, sorted_e: np.ndarray, w: np.ndarray, topk: int, bias, E: int,
                 shared=None, shared_w=None, shared_bias=None) -> np.ndarray:
    """acc = +0; acc = fma(w[t][k], f32(y[slot]) + f32(bias[e]), acc) for k in order (e = sorted_e[slot]; an e outside
    [0, E) or bias None: no add); then fma(ws, f32(shared) + f32(shared_bias), acc); fp16."""
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
        acc = fma_f32(w[:, k:k + 1].astype(np.float32), term, acc)
    if shared is not None:
        sw = np.ones((T, 1), np.float32) if shared_w is None else shared_w.reshape(T, 1).astype(np.float32)
        acc = fma_f32(sw, add_bias(shared, None if shared_bias is None else shared_bias[None, :]), acc)
    return acc.astype(np.float16)


def router(logits: np.ndarray, topk: int):
    """GptOssTopKRouter on (already biased) f32 logits: top-k on the logits (ties: lower index), softmax over the
    chosen ones. Returns (ids int32 [T, topk], weights f32 [T, topk])."""
    order = np.argsort(-logits.astype(np.float64), axis=1, kind="stable")[:, :topk]
    v = np.take_along_axis(logits, order, axis=1).astype(np.float32)
    p = np.exp(v - v[:, :1], dtype=np.float32)
    return order.astype(np.int32), p / p.sum(axis=1, keepdims=True, dtype=np.float32)


def layer(hidden: np.ndarray, w_gate: np.ndarray, logit_bias: np.ndarray, gate_up: np.ndarray, gate_up_bias: np.ndarray,
          down: np.ndarray, down_bias: np.ndarray, topk: int, alpha: float = ALPHA, limit: float = LIMIT) -> np.ndarray:
    """A whole gpt-oss MoE block in float64 (no intermediate rounding): hidden [T, H], w_gate [E, H], logit_bias [E],
    gate_up [E, 2N, H] with [gate; up] rows, gate_up_bias [E, 2N], down [E, H, N], down_bias [E, H] -> [T, H].
    The statement of what the layer computes, against which the staged GPU checks are read."""
    f = np.float64
    hidden = hidden.astype(f)
    logits = hidden @ w_gate.astype(f).T + logit_bias.astype(f)
    ids = np.argsort(-logits, axis=1, kind="stable")[:, :topk]
    v = np.take_along_axis(logits, ids, axis=1)
    p = np.exp(v - v[:, :1])
    wts = p / p.sum(axis=1, keepdims=True)
    N = gate_up.shape[1] // 2
    out = np.zeros_like(hidden)
    for t in range(hidden.shape[0]):
        for k in range(topk):
            e = ids[t, k]
            gu = gate_up[e].astype(f) @ hidden[t] + gate_up_bias[e].astype(f)
            g, u = np.minimum(gu[:N], limit), np.clip(gu[N:], -limit, limit)
            act = (u + 1) * g / (1 + np.exp(-alpha * g))
            out[t] += wts[t, k] * (down[e].astype(f) @ act + down_bias[e].astype(f))
    return out


def synthetic_checkpoint(E: int, N: int, H: int, seed: int, scale: float = 0.2):
    """A gpt-oss-shaped MoE checkpoint from random weights (torch, CPU): dict with gate_up_blocks uint8
    [E, 2N, H/32, 16], gate_up_scales uint8 [E, 2N, H/32], gate_up_bias f32 [E, 2N] (gate / up rows interleaved, as the
    model stores them), down_blocks [E, H, N/32, 16], down_scales [E, H, N/32], down_bias f32 [E, H]."""
    import torch

    from mxmoe_amd.quantize import quant_mxfp4

    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, rows, K in (("gate_up", 2 * N, H), ("down", H, N)):
        w = ((torch.rand(E * rows, K, generator=g) * 2 - 1) * scale).half()
        codes, scales = quant_mxfp4(w)
        out[f"{name}_blocks"] = codes.reshape(E, rows, K // 32, 16).contiguous()
        out[f"{name}_scales"] = scales.reshape(E, rows, K // 32).contiguous()
        out[f"{name}_bias"] = (torch.rand(E, rows, generator=g) * 2 - 1) * 0.5
    return out
