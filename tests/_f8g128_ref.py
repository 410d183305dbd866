"""numpy restatement of w8a8_g128_sym_E4M3 for the tests, independent of mxmoe_amd.quantize: the per-group
quantiser (nearest e4m3 value by search, ties to the even code), the weight block scales, the f64 GroupGEMM
C[m][n] = sum_g sa[m][g] sb[n / 128][g] sum_{k in g} a[m][k] b[n][k] and the contract's f32 fold (include/mxmoe_gg.h).
Operands: codes uint8 [rows][K], sa f32 [M][K/128], sb f32 [ceil(N/128)][K/128] (the GroupGEMM takes both transposed)."""
from __future__ import annotations

import numpy as np

from tests._mxfp8_ref import MAGNITUDES, e4m3

G = 128
E4M3_MAX = np.float32(448.0)


def quant(x: np.ndarray) -> tuple[np.ndarray, np.ndarray]:
    """fp16 [rows, K] -> (codes [rows, K], f32 scales [rows, K/128])."""
    x = np.asarray(x, np.float16)
    rows, K = x.shape
    xg = x.astype(np.float32).reshape(rows, K // G, G)
    codes = np.zeros(xg.shape, np.uint8)
    sc = np.ones(xg.shape[:2], np.float32)
    grid = MAGNITUDES[:127]  # finite magnitudes, ascending with the code
    for r in range(rows):
        for g in range(K // G):
            blk = xg[r, g]
            if not np.isfinite(blk).all():
                sc[r, g] = np.nan
                continue
            amax = np.abs(blk).max()
            if amax > 0:
                sc[r, g] = amax / E4M3_MAX  # f32 division
            y = np.minimum(np.abs(blk / sc[r, g]), E4M3_MAX).astype(np.float64)  # f32 quotient, then exact
            d = np.abs(y[:, None] - grid[None, :])
            lo = d.argmin(axis=1)  # first of two neighbours at a tie
            tie = (lo < 126) & (d[np.arange(G), lo] == d[np.arange(G), np.minimum(lo + 1, 126)])
            idx = np.where(tie & (lo % 2 == 1), lo + 1, lo).astype(np.uint8)
            codes[r, g] = idx | (np.signbit(blk).astype(np.uint8) << 7)
    return codes.reshape(rows, K), sc


def weight_scales(w: np.ndarray) -> np.ndarray:
    """fp16 [N, K] -> f32 [ceil(N/128), K/128]: amax / 448 per 128 x 128 block (1 for an all-zero block)."""
    N, K = w.shape
    a = np.abs(np.asarray(w, np.float16).astype(np.float32))
    amax = np.array([[a[i:i + G, j:j + G].max() for j in range(0, K, G)] for i in range(0, N, G)], np.float32)
    return np.where(amax == 0, np.float32(1), amax / E4M3_MAX).astype(np.float32)


def operands(M: int, N: int, K: int, exact: bool, seed: int):
    """(a_codes, sa, b_codes, sb). Scales carry a power-of-two pattern that changes by at least 2x from a group or a
    block to its neighbour (sa 2^{0,1}, sb 2^{-1,-3,-5,-7}: no step of one cancels the other's). exact: integer codes
    in [-4, 4] and the bare pattern — group sums below 2^11, scales in 2^[-7, 0], 9 groups: every fold fits 22 bits."""
    rng = np.random.default_rng(seed)
    g, nb = np.arange(K // G), np.arange((N + G - 1) // G)
    sa = np.exp2((np.arange(M)[:, None] + g[None, :]) % 2).astype(np.float32)
    sb = np.exp2(-2.0 * ((nb[:, None] + g[None, :]) % 4) - 1).astype(np.float32)
    if exact:
        ints = np.array([0x00, 0x38, 0x40, 0x44, 0x48], np.uint8)  # e4m3 codes of 0, 1, 2, 3, 4

        def draw_int(rows):
            return ints[rng.integers(0, 5, (rows, K))] | (rng.integers(0, 2, (rows, K)).astype(np.uint8) << 7)
        return draw_int(M), sa, draw_int(N), sb

    def draw(rows):  # every finite code
        c = rng.integers(0, 256, (rows, K)).astype(np.uint8)
        return np.where((c & 0x7F) == 0x7F, np.uint8(0x3A), c)
    return (draw(M), sa * rng.uniform(0.5, 1.0, sa.shape).astype(np.float32) * np.float32(2.0 ** -8),
            draw(N), sb * rng.uniform(0.5, 1.0, sb.shape).astype(np.float32) * np.float32(2.0 ** -8))


def _group_sums(a_codes, b_codes):
    a, b = e4m3(a_codes), e4m3(b_codes)
    return [a[:, k:k + G] @ b[:, k:k + G].T for k in range(0, a.shape[1], G)]  # exact in f64 for e4m3 products


def gemm(a_codes, sa, b_codes, sb) -> np.ndarray:
    sbn = np.repeat(sb, G, axis=0)[: b_codes.shape[0]].astype(np.float64)
    return sum(p * sa[:, g].astype(np.float64)[:, None] * sbn[:, g][None, :] for g, p in enumerate(_group_sums(a_codes, b_codes)))


def fma32(a: np.ndarray, b: np.ndarray, c: np.ndarray) -> np.ndarray:
    """fmaf on f32 arrays, one rounding. The product of two f32 is exact in f64; the f64 sum with c is rounded to odd
    (the error of the sum from TwoSum; an inexact sum whose last bit is even moves to its odd neighbour on the side of
    the error), and a value rounded to odd at 53 bits rounds to 24 bits as the exact one does. NaN and Inf pass through
    (0 * Inf is NaN, as in the instruction)."""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, np.float32).astype(np.float64) * np.asarray(b, np.float32).astype(np.float64)
        c = np.asarray(c, np.float32).astype(np.float64)
        p, c = np.broadcast_arrays(p, c)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def scale_products(sa, sb, rows):
    """f32_rn(sa[m][g] * sb[n / 128][g]) per group: [G] arrays of [M, N]."""
    sbn = np.repeat(np.asarray(sb, np.float32), G, axis=0)[:rows]
    with np.errstate(invalid="ignore", over="ignore"):
        return [np.asarray(sa, np.float32)[:, g][:, None] * sbn[:, g][None, :] for g in range(sa.shape[1])]


def fold_f32(accs, scales, order=None) -> np.ndarray:
    """out = 0; out = fmaf(f32(acc_g), s_g, out) over the groups of ``order`` (default: ascending): the f32 sum."""
    out = np.zeros(accs[0].shape, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for g in (range(len(accs)) if order is None else order):
            out = fma32(accs[g].astype(np.float32), scales[g], out)
    return out


def to_f16(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(x).astype(np.float16)


def gemm_fold_f32(a_codes, sa, b_codes, sb) -> np.ndarray:
    """The contract: out = fmaf(f32(acc_g), f32_rn(sa sb), out) group by group, C = fp16_rn(out). Scales may be NaN,
    Inf, zero or negative; a NaN code makes its group's acc_g NaN for the whole row (column)."""
    with np.errstate(invalid="ignore"):
        accs = _group_sums(a_codes, b_codes)
    return to_f16(fold_f32(accs, scale_products(sa, sb, b_codes.shape[0])))


def slice_bounds(groups: int, ks: int, split=lambda g, ks: -(-g // ks)) -> list[tuple[int, int]]:
    """[g0, g1) of each K slice of the decode kernel: ceil(G / ks) contiguous groups each, the last what remains
    (mxmoe_amd/csrc/moe_decode_f8g.h, DESIGN.md §4 "Decode forward: block-scaled FP8", "Waves and K slices")."""
    per = split(groups, ks)
    return [(min(s * per, groups), min(s * per + per, groups) if s < ks - 1 else groups) for s in range(ks)]


def gemm_fold_f32_sliced(a_codes, sa, b_codes, sb, ks: int, split=lambda g, ks: -(-g // ks)) -> np.ndarray:
    """The decode kernel's order with ks K slices: every slice folds its own groups from zero as the contract does, the
    slices' f32 sums are added to slice 0's in slice order (one f32 addition each), then fp16_rn. ks = 1 is
    gemm_fold_f32. ``split``: the groups per slice (the kernel's: ceil)."""
    with np.errstate(invalid="ignore"):
        accs = _group_sums(a_codes, b_codes)
    scales = scale_products(sa, sb, b_codes.shape[0])
    parts = [fold_f32(accs, scales, range(g0, g1)) for g0, g1 in slice_bounds(len(accs), ks, split)]
    out = parts[0]
    with np.errstate(invalid="ignore", over="ignore"):
        for p in parts[1:]:
            out = out + p  # f32 + f32 -> f32
    return to_f16(out)
