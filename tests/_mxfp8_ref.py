"""numpy f64 restatement of OCP MXFP8 with e4m3 elements (the A operand of w4a8_g32_sym_MXFP8) for the
tests: the e4m3 decode, the RTN quantiser of include/mxmoe_moe.h (written independently of
mxmoe_amd.quantize: nearest representable value by search over the 127 finite magnitudes, ties to the
even code) and the GroupGEMM reference against an MXFP4 B operand (tests/_mxfp4_ref.py)

    C[m][n] = sum_b 2^(sa[m][b] - 127) 2^(sb[n][b] - 127) sum_{k in b} e4m3(a[m][k]) e2m1(b[n][k])   (f64)

Canonical A format: codes uint8 [rows][K] (one OCP e4m3 code per element: bit 7 sign, bits 6..3
exponent with bias 7, bits 2..0 mantissa; exponent 0 subnormal, 0x7F / 0xFF NaN, no infinities),
scales uint8 e8m0 [rows][K/32].
"""
from __future__ import annotations

import numpy as np

from tests import _mxfp4_ref as fp4

BLOCK = 32
E4M3_MAX = 448.0


def _magnitude(c: int) -> float:
    ex, man = (c >> 3) & 0xF, c & 7
    if ex == 15 and man == 7:
        return float("nan")
    return man * 2.0 ** -9 if ex == 0 else (8 + man) * 2.0 ** (ex - 10)


# the 128 magnitudes by the low 7 code bits (index 127 is NaN), and all 256 code values
MAGNITUDES = np.array([_magnitude(c) for c in range(128)])
CODE_VALUES = np.concatenate([MAGNITUDES, -MAGNITUDES])


def e4m3(codes: np.ndarray) -> np.ndarray:
    """uint8 e4m3 codes -> f64 values (0x7F and 0xFF -> NaN)."""
    return CODE_VALUES[np.asarray(codes, np.uint8)]


def dequant(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    v = e4m3(codes)
    rows, K = v.shape
    return (v.reshape(rows, K // BLOCK, BLOCK) * fp4.e8m0(scales)[..., None]).reshape(rows, K)


def quant(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fp16 [rows, K] -> (codes [rows, K], scales [rows, K/32]), the quantiser the header defines."""
    x = np.asarray(x, np.float16)
    rows, K = x.shape
    assert K % BLOCK == 0
    xb = x.astype(np.float64).reshape(rows, K // BLOCK, BLOCK)
    codes = np.zeros(xb.shape, np.uint8)
    sc = np.zeros(xb.shape[:2], np.uint8)
    grid = MAGNITUDES[:127]  # finite magnitudes, ascending with the code
    for r in range(rows):
        for b in range(K // BLOCK):
            blk = xb[r, b]
            if not np.isfinite(blk).all():
                sc[r, b] = 255
                continue
            amax = np.abs(blk).max()
            # frexp: amax = m 2^ex, m in [0.5, 1) -> floor(log2(amax)) = ex - 1, exactly
            e = -127 if amax == 0 else int(np.clip(np.frexp(amax)[1] - 1 - 8, -127, 127))
            sc[r, b] = e + 127
            y = np.minimum(np.abs(np.ldexp(blk, -e)), E4M3_MAX)
            d = np.abs(y[:, None] - grid[None, :])
            best = d.min(axis=1, keepdims=True)
            cand = d == best  # one value, or two neighbours at a tie: the even code
            idx = np.array([next(i for i in np.flatnonzero(c) if cand[j].sum() == 1 or i % 2 == 0)
                            for j, c in enumerate(cand)], np.uint8)
            codes[r, b] = idx | (np.signbit(blk).astype(np.uint8) << 7)
    return codes.reshape(rows, K), sc


def gemm(a_codes, a_scales, b_codes, b_scales) -> np.ndarray:
    """f64 reference of the w4a8_g32_sym_MXFP8 problem (canonical operands: A MXFP8, B MXFP4)."""
    return dequant(a_codes, a_scales) @ fp4.dequant(b_codes, b_scales).T


def gemm_f32_blockwise(a_codes, a_scales, b_codes, b_scales) -> np.ndarray:
    """Emulation of the kernel's arithmetic: per block an exact dot product times the two scales,
    added block by block into an f32 accumulator."""
    a, b = e4m3(a_codes), fp4.elements(b_codes)
    M, K = a.shape
    N = b.shape[0]
    sa, sb = fp4.e8m0(a_scales), fp4.e8m0(b_scales)
    acc = np.zeros((M, N), np.float32)
    for k in range(K // BLOCK):
        sl = slice(k * BLOCK, (k + 1) * BLOCK)
        part = (a[:, sl] @ b[:, sl].T) * sa[:, k][:, None] * sb[:, k][None, :]
        acc = (acc.astype(np.float64) + part).astype(np.float32)  # one f32 rounding per block
    return acc
