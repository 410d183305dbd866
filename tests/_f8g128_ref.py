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


def gemm_fold_f32(a_codes, sa, b_codes, sb) -> np.ndarray:
    """The contract: out = fmaf(f32(acc_g), f32_rn(sa sb), out) group by group, C = fp16_rn(out)."""
    sbn = np.repeat(sb, G, axis=0)[: b_codes.shape[0]]
    out = np.zeros((a_codes.shape[0], b_codes.shape[0]), np.float32)
    for g, p in enumerate(_group_sums(a_codes, b_codes)):
        s = sa[:, g][:, None] * sbn[:, g][None, :]  # f32 x f32 -> f32, one rounding
        out = (p.astype(np.float32).astype(np.float64) * s.astype(np.float64) + out.astype(np.float64)).astype(np.float32)
    return out.astype(np.float16)
