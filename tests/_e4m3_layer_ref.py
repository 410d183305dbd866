"""Reference of the per-token e4m3 activation tag (MXMOE_ACT_E4M3, include/mxmoe_moe.h) and the inputs of its tests
(tests/test_e4m3_layer.py on the CPU, tests/test_e4m3_layer_gpu.py on the GPU) — TEST INFRASTRUCTURE ONLY.

The quantiser is numpy written from the header's rule, not from the kernel's code and not through the oracle:
amax over the row's fp16 values as f32; s = fp16_rn(amax / 448) (the f32 quotient correctly rounded, then rounded to
fp16), 1.0 for a zero row, at least 0x0400; code = e4m3_rn_sat(f32(x) / f32(s)) with the correctly rounded f32
division (numpy's), one rounding to e4m3 to nearest even, saturation at +-448, the sign kept for zeros. A row holding
+-Inf or NaN: codes 0x00 and the scale 0x7E00. tests/test_e4m3_layer.py proves it equal to oracle.quant_e4m3 on the
finite edge rows below before anything on the GPU is compared with it."""
from __future__ import annotations

import numpy as np

from tests._gptoss_ref import fma_f32  # fmaf on f32 arrays (exact f64 product, TwoSum, one rounding)

E4M3_MAX = np.float32(448.0)
NAN_SCALE = 0x7E00


def e4m3_rn_sat(q: np.ndarray) -> np.ndarray:
    """finite f32 -> OCP e4m3 codes (uint8): saturated at +-448, rounded once to nearest even, zeros keep their sign.
    The e4m3 grid: steps of 2^(e - 3) in the binade [2^e, 2^(e + 1)) for e >= -6, steps of 2^-9 below 2^-6."""
    q = np.asarray(q, np.float32)
    assert np.isfinite(q).all()
    sign = np.signbit(q).astype(np.uint8) << 7
    v = np.minimum(np.abs(q).astype(np.float64), 448.0)
    e = np.floor(np.log2(np.where(v > 0, v, 1.0)))  # (exact at powers of two: log2 of a power of two is exact)
    e = np.maximum(e, -6.0)
    step = np.exp2(e - 3)
    n = np.rint(v / step)  # v / step is exact (a power of two); rint: half to even
    val = n * step  # (n == 16 carries into the next binade: still a grid value)
    m, ex = np.frexp(val)  # val = m 2^ex, m in [0.5, 1)
    eb = ex - 1
    sub = eb < -6
    code = np.where(val == 0, 0, np.where(sub, val * 512, ((eb + 7) * 8) + (val / np.exp2(eb - 3.0) - 8)))
    return code.astype(np.uint8) | sign


def quant(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fp16 [rows, K] -> (codes uint8 [rows, K] in logical K order, scale bit patterns uint16 [rows])."""
    x = np.ascontiguousarray(x, np.float16)
    xf = x.astype(np.float32)
    bad = ~np.isfinite(xf).all(axis=1)
    xf = np.where(bad[:, None], np.float32(0), xf)
    amax = np.abs(xf).max(axis=1) if x.shape[1] else np.zeros(x.shape[0], np.float32)
    s = (amax / E4M3_MAX).astype(np.float16)  # f32 division, then one rounding to fp16
    s = np.maximum(s, np.float16(2.0 ** -14))
    s = np.where(amax == 0, np.float16(1), s).astype(np.float16)
    codes = e4m3_rn_sat(xf / s.astype(np.float32)[:, None])
    codes = np.where(bad[:, None], np.uint8(0), codes)
    sbits = np.where(bad, np.uint16(NAN_SCALE), s.view(np.uint16)).astype(np.uint16)
    return codes, sbits


def pack(codes: np.ndarray) -> np.ndarray:
    """logical codes [rows, K] -> pack_wxax's 8-bit byte order (element 2j in the high byte of its 16-bit word)."""
    r, K = codes.shape
    return np.ascontiguousarray(codes.reshape(r, K // 2, 2)[:, :, ::-1]).reshape(r, K)


# ---------------------------------------------------------------------------------------------- the division
def kernel_quotient(x: np.ndarray, s: np.ndarray) -> np.ndarray:
    """The kernel's sequence in place of the f32 division (moe_ops.hip, codes_e4m3): r = the correctly rounded 1 / s,
    q = x r, q' = fma(fma(-q, s, x), r, q), the sign copied from x. f32 arrays in, f32 out."""
    x, s = np.asarray(x, np.float32), np.asarray(s, np.float32)
    r = (np.float32(1) / s).astype(np.float32)
    q = (x * r).astype(np.float32)
    return np.copysign(fma_f32(fma_f32(-q, s, x), r, q), x)


# ---------------------------------------------------------------------------------------------- inputs
def scale_rounding_amax(down: bool) -> np.float16:
    """The first fp16 a in [1024, 2048) whose scale s = fp16(a / 448) was rounded down (a / s > 448: the row's largest
    elements saturate) or up (a / s < 448: they do not)."""
    a = np.arange(0x6400, 0x6800, dtype=np.uint16).view(np.float16)
    s = (a.astype(np.float32) / E4M3_MAX).astype(np.float16)
    d = a.astype(np.float64) / s.astype(np.float64)
    return a[np.nonzero(d > 448 if down else d < 448)[0][0]]


EDGE_KINDS = ("zero", "lone_tiny", "amax_max", "ties", "scale_down", "scale_up")


def edge_rows(W: int, seed: int = 0, n_random: int = 3, tail: bool = False) -> np.ndarray:
    """fp16 [6 + n_random, W]: one row per EDGE_KINDS, then random rows over 30 binades.
      zero ........ all +0: scale 1, codes 0
      lone_tiny ... a lone 2^-24: amax / 448 underflows in fp16, the scale is the clamp 2^-14 and 2^-24 / 2^-14 = 2^-10
                    is the tie between 0 and the smallest e4m3 subnormal
      amax_max .... amax 65504 at both signs over uniform values
      ties ........ amax 448 (scale exactly 1): 17, 19, -17 (ties of the binade of 16), -0, 2^-10 and 3 * 2^-10 (ties
                    of the subnormal grid), 447, over small multiples of 2^-9
      scale_down .. amax = scale_rounding_amax(True): the scale was rounded down, amax / s > 448 saturates
      scale_up .... amax = scale_rounding_amax(False): rounded up, amax / s < 448
    tail: every row's largest elements lie in its last 8 columns only (a split row's last quarter)."""
    rng = np.random.default_rng(977 * seed + W)
    c0 = W - 8 if tail else 0  # where the elements that set the scale go
    rows = [np.zeros(W)]
    x = np.zeros(W)
    x[W - 3] = 2.0 ** -24
    rows.append(x)
    x = rng.uniform(-1, 1, W) * 60000
    x[c0], x[c0 + 1] = 65504, -65504
    rows.append(x)
    x = rng.integers(-40, 41, W) * 2.0 ** -9
    x[c0:c0 + 8] = [448, 17, 19, -17, -0.0, 2.0 ** -10, 3 * 2.0 ** -10, 447]
    rows.append(x)
    for down in (True, False):
        a = float(scale_rounding_amax(down))
        x = rng.uniform(-0.97, 0.97, W) * a
        prev = float(np.nextafter(np.float16(a), np.float16(0)))
        x[c0:c0 + 4] = [a, -a, prev, -prev]
        rows.append(x)
    for i in range(n_random):
        x = rng.standard_normal(W) * 2.0 ** rng.integers(-15, 15, W) * 0.5
        if tail:
            x[:c0] *= 2.0 ** -16
            x[c0] = 300.0 * (i + 1)
        rows.append(np.clip(x, -65504, 65504))
    return np.stack(rows).astype(np.float16)
