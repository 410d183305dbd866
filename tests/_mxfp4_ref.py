"""numpy f64 restatement of OCP MXFP4 (w4a4_g32_sym_MXFP4) for the tests: the e2m1 / e8m0 decode, the
RTN quantiser of include/mxmoe_gg.h (written independently of mxmoe_amd.quantize: nearest grid point by
search, ties to the even code), the scale-layout transpose and the GroupGEMM reference

    C[m][n] = sum_b 2^(sa[m][b] - 127) 2^(sb[n][b] - 127) sum_{k in b} a[m][k] b[n][k]     (f64)

Canonical operand format: codes uint8 [rows][K/2] (element 2i in the low nibble of byte i), scales
uint8 e8m0 [rows][K/32].
"""
from __future__ import annotations

import numpy as np

BLOCK = 32
GRID = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])
# the 16 e2m1 codes: bit 3 sign, bits 2..0 index into GRID
CODE_VALUES = np.concatenate([GRID, -GRID])


def e8m0(codes: np.ndarray) -> np.ndarray:
    """uint8 e8m0 -> f64 2^(code - 127); 255 -> NaN."""
    c = np.asarray(codes).astype(np.int64)
    return np.where(c == 255, np.nan, np.ldexp(1.0, np.minimum(c, 254) - 127))


def nibbles(codes: np.ndarray) -> np.ndarray:
    """codes uint8 [rows, K/2] -> nibble codes uint8 [rows, K] in element order."""
    c = np.asarray(codes, np.uint8)
    return np.stack([c & 0xF, c >> 4], axis=-1).reshape(c.shape[0], 2 * c.shape[1])


def pack_nibbles(nib: np.ndarray) -> np.ndarray:
    n = np.asarray(nib, np.uint8).reshape(nib.shape[0], nib.shape[1] // 2, 2)
    return (n[..., 0] | (n[..., 1] << 4)).astype(np.uint8)


def elements(codes: np.ndarray) -> np.ndarray:
    """codes -> the unscaled e2m1 values f64 [rows, K]."""
    return CODE_VALUES[nibbles(codes)]


def dequant(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    v = elements(codes)
    rows, K = v.shape
    return (v.reshape(rows, K // BLOCK, BLOCK) * e8m0(scales)[..., None]).reshape(rows, K)


def quant(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fp16 [rows, K] -> (codes, scales), the quantiser the header defines, block by block."""
    x = np.asarray(x, np.float16)
    rows, K = x.shape
    assert K % BLOCK == 0
    xb = x.astype(np.float64).reshape(rows, K // BLOCK, BLOCK)
    nib = np.zeros(xb.shape, np.uint8)
    sc = np.zeros(xb.shape[:2], np.uint8)
    for r in range(rows):
        for b in range(K // BLOCK):
            blk = xb[r, b]
            if not np.isfinite(blk).all():
                sc[r, b] = 255
                continue
            amax = np.abs(blk).max()
            # frexp: amax = m 2^ex, m in [0.5, 1) -> floor(log2(amax)) = ex - 1, exactly
            e = -127 if amax == 0 else int(np.clip(np.frexp(amax)[1] - 1 - 2, -127, 127))
            sc[r, b] = e + 127
            y = np.minimum(np.abs(np.ldexp(blk, -e)), 6.0)
            d = np.abs(y[:, None] - GRID[None, :])
            best = d.min(axis=1, keepdims=True)
            cand = d == best  # one grid point, or two neighbours at a tie: take the even code
            idx = np.array([next(i for i in np.flatnonzero(c) if cand[j].sum() == 1 or i % 2 == 0)
                            for j, c in enumerate(cand)], np.uint8)
            nib[r, b] = idx | (np.signbit(blk).astype(np.uint8) << 3)
    return pack_nibbles(nib.reshape(rows, K)), sc


def pack_scales(scales: np.ndarray) -> np.ndarray:
    """canonical [rows, K/32] -> device layout [rows, 16 G]: dev[16 t + 4 g + i] = canon[16 t + 4 i + g], pads 127."""
    s = np.asarray(scales, np.uint8)
    rows, nb = s.shape
    G = (nb + 15) // 16
    dev = np.full((rows, 16 * G), 127, np.uint8)
    for c in range(nb):
        t, i, g = c // 16, (c % 16) // 4, c % 4
        dev[:, 16 * t + 4 * g + i] = s[:, c]
    return dev


def gemm(a_codes, a_scales, b_codes, b_scales) -> np.ndarray:
    """f64 reference of the MXFP4 GroupGEMM problem (canonical operands)."""
    return dequant(a_codes, a_scales) @ dequant(b_codes, b_scales).T


def gemm_f32_blockwise(a_codes, a_scales, b_codes, b_scales) -> np.ndarray:
    """Emulation of the kernel's arithmetic: per block an exact dot product times the two scales,
    added block by block into an f32 accumulator."""
    a, b = elements(a_codes), elements(b_codes)
    M, K = a.shape
    N = b.shape[0]
    sa, sb = e8m0(a_scales), e8m0(b_scales)
    acc = np.zeros((M, N), np.float32)
    for k in range(K // BLOCK):
        sl = slice(k * BLOCK, (k + 1) * BLOCK)
        part = (a[:, sl] @ b[:, sl].T) * sa[:, k][:, None] * sb[:, k][None, :]
        acc = (acc.astype(np.float64) + part).astype(np.float32)  # one f32 rounding per block
    return acc
