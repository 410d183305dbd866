"""Edge-value operands for the w8a8_g128_sym_E4M3 bodies (gg_tile_f8g128 exact and fallback builds, gg_tile_f8g128s on
wo3, decode_f8g_kernel): tests/test_f8g128_edges.py on the CPU, tests/test_f8g128_edges_gpu.py on the GPU.

Every generator is pure numpy and seeded; both files call the same ones, so what the CPU file proves about a family
holds for what the GPU file runs. A problem is a ``Prob``: shape, operands in tests/_f8g128_ref.py's layout
(a_codes [M, K], sa f32 [M, K/128], b_codes [N, K], sb f32 [ceil(N/128), K/128]) and an ``info`` dict.

The comparison rule is bit for bit against ``_f8g128_ref.gemm_fold_f32`` (NaN by isnan), with no tolerance. The
contract fixes the fold (out = fmaf(acc_g, f32_rn(sa sb), out), groups ascending, C = fp16_rn(out)) but not the order
in which the MFMA sums a group's 128 products, so the operands make that order irrelevant PER GROUP: within a group all
products are multiples of a granule ga gb, for every (row, column, group) sum |a b| / (ga gb) < 2^24 (``info['bound']``),
and the largest single product stays below 2^14 granules (``info['span']``, the exact_span rule of
tests/_decode_lp_edges.py: sums with one product far above the granule came back inexact from the scaled MFMA once,
DESIGN.md §4 "Decode forward on MFMA"). Then acc_g is exact in f32 in any order and the ordered fold is the one right
answer for ANY f32 scales. Only family F-x breaks the span rule, on purpose.

Where the contract is silent no case is built: no scale product f32_rn(sa sb) is an f32 subnormal (``scale_classes``
asserts it). A zero output is compared by bits like any other: the contract's own words (`out = 0`, then fmas) give +0
whenever every product is zero - also under a negative scale or -0 codes, since x + (+0) is +0 for x = +-0 - and -0
only where a negative f32 sum underflows in fp16_rn, and the reference follows them.
"""
from __future__ import annotations

import dataclasses

import numpy as np

from tests import _f8g128_ref as ref
from tests import _fp8_bf16_edges as E
from tests._fp8_bf16_edges import E4M3, window_codes, window_granule
from tests._util import permuted_identity

G = 128
ONE = 0x38  # e4m3 code of 1.0
SPAN = 2.0 ** 14
F32_MIN_NORMAL = 2.0 ** -126


@dataclasses.dataclass
class Prob:
    M: int
    N: int
    K: int
    ops: tuple  # (a_codes, sa, b_codes, sb)
    info: dict

    @property
    def shape(self):
        return self.M, self.N, self.K


# the GPU file's shapes. v2x (exact build and fallback): one tile of one group | a partial scale block, odd group
# count | the 128-row class, 9 groups | a 256-row tile + tail tile, a guarded N tail crossing a block boundary.
# wo3: one row | a row block boundary | a second tile of one row, 9 groups | three tiles with a 2-row tail.
SHAPES_V2X = [(1, 128, 128), (17, 200, 384), (129, 384, 1152), (300, 264, 256)]
SHAPES_WO3 = [(1, 128, 128), (17, 200, 384), (65, 384, 1152), (130, 200, 256)]
SHAPES = {"v2x": SHAPES_V2X, "wo3": SHAPES_WO3}

# Exponent-field windows of tests/_fp8_bf16_edges.py. A window [lo, hi] has max |v| / granule = 15 * 2^(hi - max(lo, 1));
# with spans sA + sB <= 6 the largest product is 225 * 2^6 = 14400 < 2^14 granules and a group's sum of magnitudes at most
# 128 * 14400 < 2^21. The six pairs hold every window on each side: all 254 finite codes.
W_LOW, W_MID_LO, W_MID_HI, W_TOP = E.W_LOW, E.W_MID_LO, E.W_MID_HI, E.W_TOP
FA_WINDOWS = [(W_LOW, W_LOW), (W_TOP, W_TOP), (W_LOW, W_TOP), (W_TOP, W_LOW), (W_MID_LO, W_MID_HI), (W_MID_HI, W_MID_LO)]
W_SMALL = ((5, 8), (5, 8))  # |v| in [0.25, 3.75], granule 2^-5


def values(codes) -> np.ndarray:
    return E4M3[np.asarray(codes, np.uint8)]


def group_accs(p: Prob) -> np.ndarray:
    """acc_g [G, M, N] in f64 (exact: e4m3 products are multiples of 2^-18 below 2^18)."""
    a, b = values(p.ops[0]), values(p.ops[2])
    with np.errstate(invalid="ignore"):
        return np.stack([a[:, k:k + G] @ b[:, k:k + G].T for k in range(0, p.K, G)])


def bounds(p: Prob) -> tuple[float, float]:
    """(bound, span) from the operands in f64: max over (row, column, group) of sum |a b| / (ga gb), and max over all
    products of |a b| / (ga gb); asserts every finite operand is a multiple of its granule. NaN codes count as 448."""
    ga, gb = p.info["ga"], p.info["gb"]
    a, b = np.abs(np.nan_to_num(values(p.ops[0]), nan=448.0)) / ga, np.abs(np.nan_to_num(values(p.ops[2]), nan=448.0)) / gb
    assert (a == np.rint(a)).all() and (b == np.rint(b)).all(), "an operand is off its granule"
    bound = max(float((a[:, k:k + G] @ b[:, k:k + G].T).max()) for k in range(0, p.K, G))
    span = max(float((a[:, k:k + G].max(axis=0) * b[:, k:k + G].max(axis=0)).max()) for k in range(0, p.K, G))
    return bound, span


def _finish(M, N, K, ops, **info) -> Prob:
    p = Prob(M, N, K, tuple(np.ascontiguousarray(o) for o in ops), info)
    p.info["bound"], p.info["span"] = bounds(p)
    return p


def expected(p: Prob) -> np.ndarray:
    return ref.gemm_fold_f32(*p.ops)


def mismatch(out: np.ndarray, want: np.ndarray) -> np.ndarray:
    """Where out differs from want: bit for bit, a zero's sign included; NaN by isnan (E.mismatch)."""
    return E.mismatch(out, want)


def full_f32(rng, shape, lo_exp: float, hi_exp: float) -> np.ndarray:
    """f32 drawn log-uniformly in [2^lo_exp, 2^hi_exp) with random low significand bits (the last one set: 24 bits)."""
    x = np.exp2(rng.uniform(lo_exp, hi_exp, shape)).astype(np.float32)
    return ((x.view(np.uint32) & ~np.uint32(0xFFF)) | rng.integers(0, 1 << 12, shape).astype(np.uint32) | np.uint32(1)).view(np.float32)


def _window_rows(rng, rows, K, win):
    """Bytes drawn from a window's codes, the whole code list at the start of row 0 and at the end of the last row."""
    return E.window_rows(rng, rows, K, win)


# ------------------------------------------------------------------ F-a: windows, the fold contract
def gen_window(M, N, K, wa, wb, seed) -> Prob:
    """F-a: A bytes from window wa, B bytes from wb, every code of each window present; sa and sb with full 24-bit
    significands, drawn log-uniformly over two octaves around a base that brings a group's contribution to order 1 -
    so outputs stay finite (and, but for rare cancellations, normal) in fp16, every f32_rn(sa sb) rounds, and with
    more than one group every fold step rounds."""
    rng = np.random.default_rng(seed)
    A, B = _window_rows(rng, M, K, wa), _window_rows(rng, N, K, wb)
    rms = np.sqrt(G * np.mean(values(A) ** 2) * np.mean(values(B) ** 2))
    base = -np.log2(rms) / 2
    sa = full_f32(rng, (M, K // G), base - 1, base + 1)
    sb = full_f32(rng, ((N + G - 1) // G, K // G), base - 1, base + 1)
    return _finish(M, N, K, (A, sa, B, sb), family="a", wa=wa, wb=wb, ga=window_granule(wa[0]), gb=window_granule(wb[0]))


def window_problems(path: str) -> list[Prob]:
    """F-a for a path's shapes ("v2x" / "wo3"): the six window pairs over the four shapes (the two largest twice)."""
    shapes = SHAPES[path]
    order = [0, 1, 2, 3, 2, 3]
    return [gen_window(*shapes[order[i]], wa, wb, seed=2000 + 10 * i + (path == "wo3"))
            for i, (wa, wb) in enumerate(FA_WINDOWS)]


# ------------------------------------------------------------------ F-b: readout
READ_K, READ_ROWS = 256, 264
NAN_ROW_STEP = E.NAN_ROW_STEP


def gen_readout(side: str, seed: int) -> Prob:
    """F-b, K = 256. side "B" (256, 264, 256): A is a permuted identity of code 0x38 and row n of B holds code
    (k + n) % 256 at byte k - over the rows every code stands at every byte position of a group, in both groups:
    C[m, n] = fp16_rn(value(B[n, pi[m]]) * sa[m][g] sb[n / 128][g]), g = pi[m] / 128. side "A" (264, 256, 256): the
    mirror, A cycling and B the permuted identity. The scales are powers of two that differ per group and per block
    (and per row parity): the output also tells whose scale was applied. The NaN codes stay only in the rows
    r % 15 == 5 of the cycling side (there they poison their whole output column / row through 0 * NaN); elsewhere
    they are replaced by +-448. Every (row, column, group) has at most one nonzero product (info['one_product']):
    exact whatever its size, and nothing stands beside it for the span rule to speak of."""
    rng = np.random.default_rng(seed)
    K, rows = READ_K, READ_ROWS
    codes = ((np.arange(K)[None, :] + np.arange(rows)[:, None]) % 256).astype(np.uint8)
    nan_rows = np.arange(rows) % NAN_ROW_STEP == 5
    swap = ((codes & 0x7F) == 0x7F) & ~nan_rows[:, None]
    codes[swap] -= 1
    ident, pi = permuted_identity(K, rng)
    ident = np.where(ident != 0, np.uint8(ONE), np.uint8(0)).astype(np.uint8)
    M, N = (K, rows) if side == "B" else (rows, K)
    A, B = (ident, codes) if side == "B" else (codes, ident)
    g, nb = np.arange(K // G), np.arange((N + G - 1) // G)
    sa = np.exp2((np.arange(M)[:, None] + g[None, :]) % 2).astype(np.float32)
    sb = np.exp2(-2.0 * ((nb[:, None] + 2 * g[None, :]) % 4) - 1).astype(np.float32)
    return _finish(M, N, K, (A, sa, B, sb), family="b", side=side, pi=pi, nan_rows=nan_rows, one_product=True,
                   ga=1.0 if side == "B" else 2.0 ** -9, gb=2.0 ** -9 if side == "B" else 1.0)


def readout_problems() -> list[Prob]:
    return [gen_readout("B", 2100), gen_readout("A", 2101)]


# ------------------------------------------------------------------ F-c: scale ladder
INTS = np.array([0x00, 0x38, 0x40, 0x44, 0x48], np.uint8)  # 0, 1, 2, 3, 4
LADDER_KINDS = ("zero", "negative", "sub_exact", "sub_tie", "overflow", "nan_sa", "nan_inf_sb", "inf_sa")
LADDER_SHAPES = {"v2x": [(17, 200, 384), (300, 264, 256)], "wo3": [(17, 200, 384), (130, 200, 256)]}


def gen_ladder(M, N, K, kind: str, seed: int) -> Prob:
    """F-c: integer codes 0, +-1 .. +-4 (a group's sum is an integer of at most 2048) on the power-of-two scale pattern
    of _f8g128_ref.operands (exact) - every fold exact - with one class of scale edge planted:
      zero ......... sa entries 0 and -0 (single (row, group) pairs and a whole row) and an sb block entry 0 and -0
      negative ..... every third sa row negative, sb negative in the odd blocks
      sub_exact .... sa sb scaled by 2^-24: outputs are integers on fp16's subnormal grid, met exactly
      sub_tie ...... by 2^-25: every odd sum is a tie on that grid (to even); 2^-25 is a normal f32
      overflow ..... by 2^+11 in the even groups: sums beyond 65504 / 2^11 leave fp16 for +-inf, the others stay finite
      nan_sa ....... NaN sa for single (row, group) pairs whose A codes are zero - what the quantiser emits for a group
                     with Inf / NaN: rows 0, M - 1 and the first row of the last (partial) 16-row block, exactly
                     those rows NaN (info['rows'])
      nan_inf_sb ... one NaN and one Inf sb entry, one of them in the last, partial block (N % 128 != 0): the NaN
                     block's columns NaN for every row, the Inf block's +-inf (NaN where the group sum is 0)
      inf_sa ....... an Inf sa on a (row, group) with zero A codes: 0 * Inf = NaN, that row alone
    info['classes'] names the scale classes the problem holds."""
    assert kind in LADDER_KINDS and N % G and M >= 17
    rng = np.random.default_rng(seed)
    NB, Gk = (N + G - 1) // G, K // G
    draw = lambda rows: INTS[rng.integers(0, 5, (rows, K))] | (rng.integers(0, 2, (rows, K)).astype(np.uint8) << 7)
    A, B = draw(M), draw(N)
    _, sa, _, sb = ref.operands(M, N, K, True, seed)
    last_block_row = 16 * ((M - 1) // 16)
    rows, classes = [], {kind}
    if kind == "zero":
        sa[1, 0], sa[M - 1, Gk - 1], sa[5, :] = 0.0, -0.0, -0.0
        sb[0, Gk - 1], sb[NB - 1, 0] = 0.0, -0.0
        classes |= {"sa_zero", "sa_negzero", "sb_zero", "sb_negzero"}
    elif kind == "negative":
        sa[::3] *= -1
        sb[1::2] *= -1
    elif kind in ("sub_exact", "sub_tie"):
        sa *= np.float32(2.0 ** -12)
        sb *= np.float32(2.0 ** (-12 if kind == "sub_exact" else -13))
    elif kind == "overflow":
        sa[:, ::2] *= np.float32(2.0 ** 7)
        sb[:, ::2] *= np.float32(2.0 ** 4)
    elif kind in ("nan_sa", "inf_sa"):
        rows = sorted({0, last_block_row, M - 1}) if kind == "nan_sa" else [last_block_row + (M - 1 > last_block_row)]
        for i, r in enumerate(rows):
            g = (Gk - 1 - i) % Gk
            A[r, g * G:(g + 1) * G] = 0
            sa[r, g] = np.nan if kind == "nan_sa" else np.inf
    else:
        flip = (seed // 16) % 2 == 1  # (the second shape of a path: the other way round)
        sb[(NB - 1, 0)[flip], 0] = np.nan
        sb[(0, NB - 1)[flip], Gk - 1] = np.inf
        classes |= {"nan_sb", "inf_sb", "partial_block_" + ("nan", "inf")[flip]}
    return _finish(M, N, K, (A, sa, B, sb), family="c", kind=kind, classes=classes, rows=rows, ga=1.0, gb=1.0)


def ladder_problems(path: str) -> list[Prob]:
    return [gen_ladder(*s, kind, seed=2200 + 16 * j + i) for j, s in enumerate(LADDER_SHAPES[path])
            for i, kind in enumerate(LADDER_KINDS)]


def scale_classes(p: Prob) -> set:
    """The classes of f32_rn(sa sb) a problem holds, recomputed from its operands; asserts that no product is an f32
    subnormal (the contract is silent there)."""
    sa, sb = p.ops[1], p.ops[3]
    with np.errstate(invalid="ignore", over="ignore"):
        prod = (sa[:, None, :] * sb[None, :, :]).astype(np.float32)
    fin = np.isfinite(prod) & (prod != 0)
    assert (np.abs(prod[fin]) >= F32_MIN_NORMAL).all(), "an f32-subnormal scale product"
    out = set()
    for name, s in (("sa", sa), ("sb", sb)):
        if ((s == 0) & ~np.signbit(s)).any():
            out.add(name + "_zero")
        if ((s == 0) & np.signbit(s)).any():
            out.add(name + "_negzero")
        if (s < 0).any():
            out.add(name + "_negative")
        if np.isnan(s).any():
            out.add("nan_" + name)
        if np.isinf(s).any():
            out.add("inf_" + name)
    return out


# ------------------------------------------------------------------ F-d: cancellation across groups
FD_SHAPES = {"v2x": [(129, 384, 1152), (300, 264, 1152)], "wo3": [(65, 384, 1152), (130, 200, 1152)]}


def gen_cancel(M, N, K, seed) -> Prob:
    """F-d, K = 1152 (9 groups): groups g and g + 4 (g = 0 .. 3) hold the same codes on both sides, so their group sums
    are equal for every (row, column), and their scales nearly cancel: sa[m][g + 4] = -sa[m][g] (1 + da[m][g]),
    sb[j][g + 4] = sb[j][g] (1 + db[j][g]) with da, db in 2^-20 .. 2^-10. A pair leaves (da + db) of one contribution;
    the pairs' magnitudes step by 2^3, the ninth group is of the remainder's order. The partial sums stand 2^10 .. 2^20
    above the final value, so every rounding of the f32 fold is worth many fp16 ulps of the output: any other order,
    an unfused multiply-add or another rounding of the scale product moves many outputs."""
    assert K == 9 * G
    rng = np.random.default_rng(seed)
    wa, wb = W_SMALL
    A, B = _window_rows(rng, M, K, wa), _window_rows(rng, N, K, wb)
    NB = (N + G - 1) // G
    for g in range(4):
        A[:, (g + 4) * G:(g + 5) * G] = A[:, g * G:(g + 1) * G]
        B[:, (g + 4) * G:(g + 5) * G] = B[:, g * G:(g + 1) * G]
    sa, sb = np.empty((M, 9), np.float32), np.empty((NB, 9), np.float32)
    for g in range(4):
        sa[:, g] = full_f32(rng, M, 1.5 * g, 1.5 * g + 1)
        sb[:, g] = full_f32(rng, NB, 1.5 * g, 1.5 * g + 1)
        sa[:, g + 4] = -(sa[:, g] * (np.float32(1) + full_f32(rng, M, -20, -10)))
        sb[:, g + 4] = sb[:, g] * (np.float32(1) + full_f32(rng, NB, -20, -10))
    sa[:, 8], sb[:, 8] = full_f32(rng, M, -5, -4), full_f32(rng, NB, -5, -4)
    return _finish(M, N, K, (A, sa, B, sb), family="d", ga=window_granule(wa[0]), gb=window_granule(wb[0]))


def cancel_problems(path: str) -> list[Prob]:
    return [gen_cancel(*s, seed=2300 + 2 * i + (path == "wo3")) for i, s in enumerate(FD_SHAPES[path])]


# ------------------------------------------------------------------ F-x: the 448 question (breaks the span rule)
FX_SHAPES = {"v2x": [(129, 384, 1152), (300, 264, 256)], "wo3": [(65, 384, 1152), (130, 200, 256)]}


def gen_span(M, N, K, seed) -> Prob:
    """F-x: both sides from window (5, 8) (|v| in 0.25 .. 3.75, granule 2^-5), and in every A group one +-448 code: it
    meets a weight code of 0.25 .. 3.75 beside products down to 2^-4. Every product is a multiple of 2^-10, the
    largest is 448 * 3.75 = 2^20.7 granules, and a group's sum of magnitudes stays below 2^22 granules: exact in f32
    in any order, but not under the 2^14 span rule. Scales: F-a's. These are the operands of the DESIGN.md note;
    nothing is asserted about bits on them."""
    rng = np.random.default_rng(seed)
    wa, wb = (5, 8), (5, 8)
    A, B = _window_rows(rng, M, K, wa), _window_rows(rng, N, K, wb)
    hot = G * np.arange(K // G) + (7 * np.arange(K // G) + 3) % G
    A[:, hot] = np.where(rng.integers(0, 2, (M, K // G)) == 1, np.uint8(0x7E), np.uint8(0xFE))
    B[:, hot] = np.where(B[:, hot] & 0x7F == 0, np.uint8(0x30), B[:, hot])
    rms = np.sqrt(G * np.mean(values(A) ** 2) * np.mean(values(B) ** 2))
    base = -np.log2(rms) / 2
    sa = full_f32(rng, (M, K // G), base - 1, base + 1)
    sb = full_f32(rng, ((N + G - 1) // G, K // G), base - 1, base + 1)
    return _finish(M, N, K, (A, sa, B, sb), family="x", ga=2.0 ** -5, gb=2.0 ** -5)


def span_problems(path: str) -> list[Prob]:
    return [gen_span(*s, seed=2400 + 2 * i + (path == "wo3")) for i, s in enumerate(FX_SHAPES[path])]


# ------------------------------------------------------------------ F-q: quantiser rows for the decode kernel
def special_groups() -> np.ndarray:
    """The first group of every row of tests/test_f8g128.py::_special_groups, [6, 128]: zero with a -0 | a single
    65504 | code ties | fp16 subnormals | random, and rows 4 / 5 with the Inf / NaN that the original keeps in its
    second group planted here."""
    from tests.test_f8g128 import _special_groups
    x = _special_groups()[:, :G].copy()
    x[4, 9] = np.inf
    x[5, 2] = np.nan
    return x


def quant_rows(n: int, K: int, seed: int) -> np.ndarray:
    """F-q: fp16 [n, K]. Every group is random (an amax that is not 448 * 2^e: the f32 division and the f32 quotients
    round) at a magnitude of 2^-6 .. 2^6 of its own; row r < 6 * (K / 128) carries special group r % 6 at group
    position r // 6 - every special at every 128-column position, the row's last group included, as far as n reaches
    (n < 6 K / 128: position by position from the LAST group down, so the last group is always covered)."""
    rng = np.random.default_rng(seed)
    Gk = K // G
    x = (rng.standard_normal((n, K)) * np.exp2(rng.integers(-6, 7, (n, Gk))).repeat(G, axis=1)).astype(np.float16)
    sp = special_groups()
    for r in range(min(n, 6 * Gk)):
        g = Gk - 1 - r // 6
        x[r, g * G:(g + 1) * G] = sp[r % 6]
    return x


def readout_weight(H: int, K: int, seed: int):
    """[H, K] codes: row h < K one-hot of 0x38 at column pi[h], rows past K zero; sb = 1: y[p, h] = fp16_rn(value(code
    [p, pi[h]]) * sa[p][pi[h] / 128])."""
    ident, pi = permuted_identity(K, np.random.default_rng(seed))
    W = np.zeros((H, K), np.uint8)
    W[:K] = np.where(ident != 0, np.uint8(ONE), np.uint8(0))
    return W, np.ones(((H + G - 1) // G, K // G), np.float32), pi


# ------------------------------------------------------------------ decode fold operands
def decode_operands(rows: int, E_: int, C: int, K: int, seed: int, wa=W_MID_LO, wb=W_MID_HI, span_break: bool = False,
                    e_span: int = 6, gain: float = 1.0):
    """fp16 A rows [rows, K] whose in-kernel quantisation is known, and per expert weight codes [C, K] with block
    scales [ceil(C / 128), K / 128]. In every group of a row one element is 448 * 2^e (e per (row, group) in -6 .. 6)
    at a column where every weight code is zero; the other elements are window-wa values times 2^e: the quantiser's
    amax is 448 * 2^e, its scale 2^e exactly, its quotients the window's values, its codes the window's. Weight codes
    come from window wb, the block scales are f32 with 24-bit significands at a base that brings a group's contribution
    to order ``gain`` (times the row's 2^e), so every fold step rounds. span_break (F-x): the hot column's weight codes
    are not zeroed. e_span: e in -e_span .. e_span (gate_up takes 1 and gain 1/8: g and u stay below 64 and their gated
    product inside fp16). Returns (x, a_codes, sa, [(b_codes, sb)] * E_)."""
    rng = np.random.default_rng(seed)
    Gk = K // G
    pool = window_codes(*wa)
    a_codes = pool[rng.integers(0, len(pool), (rows, K))]
    hot = G * np.arange(Gk) + (7 * np.arange(Gk) + 3) % G
    a_codes[:, hot] = 0x7E
    sa = np.exp2(rng.integers(-e_span, e_span + 1, (rows, Gk))).astype(np.float32)
    x = (values(a_codes) * np.repeat(sa, G, axis=1)).astype(np.float16)
    assert (x.astype(np.float64) == values(a_codes) * np.repeat(sa, G, axis=1)).all()  # exact fp16 values
    wpool = window_codes(*wb)
    rms = np.sqrt(G * np.mean(values(pool) ** 2) * np.mean(values(wpool) ** 2)) / gain
    ws = []
    for _ in range(E_):
        b = wpool[rng.integers(0, len(wpool), (C, K))]
        b[:, hot] = np.where(b[:, hot] & 0x7F == 0, np.uint8(0x30), b[:, hot]) if span_break else 0
        ws.append((b, full_f32(rng, ((C + G - 1) // G, Gk), -np.log2(rms) - 1, -np.log2(rms) + 1)))
    return x, a_codes, sa, ws


def decode_cancel_operands(rows: int, E_: int, C: int, K: int, seed: int):
    """F-d for the decode kernel. With np = (G - 1) / 2 pairs, groups g and g + np (g < np) of an act row are the same
    fp16 values, so they quantise to the same codes and the same scale, and hold the same weight codes; the groups
    past 2 np are free. The act scale of a (row, pair) is j 2^e with j odd in 65 .. 127: the hot element is
    448 j 2^e (an fp16 value: 7 j < 2048), the others window-(5, 8) values times j 2^e (4 + 7 significant bits: fp16
    values), so the in-kernel amax / 448 and every quotient are exact and the codes known - but sa is no power of two:
    f32_rn(acc sa) rounds, and (acc sa) sb differs from acc f32_rn(sa sb). sb[g + np] = -sb[g] (1 + d), d in
    2^-20 .. 2^-10, the pairs' magnitudes stepping by 2^3, the free groups of the remainder's order: the partial sums
    stand 2^10 .. 2^20 above the result, within a K slice or across the two. Returns decode_operands' tuple."""
    rng = np.random.default_rng(seed)
    Gk = K // G
    npair = (Gk - 1) // 2
    base = np.array([g - npair if npair <= g < 2 * npair else g for g in range(Gk)])
    wa, wb = W_SMALL
    pool, wpool = window_codes(*wa), window_codes(*wb)
    hot = G * np.arange(Gk) + (7 * base + 3) % G

    def dup(c):
        for g in range(npair):
            c[:, (g + npair) * G:(g + npair + 1) * G] = c[:, g * G:(g + 1) * G]
        return c
    a_codes = pool[rng.integers(0, len(pool), (rows, K))]
    a_codes[:, hot] = 0x7E
    a_codes = dup(a_codes)
    sa = ((2 * rng.integers(32, 64, (rows, Gk)) + 1) * np.exp2(rng.integers(-8, -5, (rows, Gk)))).astype(np.float32)
    sa[:, npair:2 * npair] = sa[:, :npair]
    x = (values(a_codes) * np.repeat(sa, G, axis=1)).astype(np.float16)
    assert (x.astype(np.float64) == values(a_codes) * np.repeat(sa, G, axis=1)).all()  # exact fp16 values
    ws = []
    NB = (C + G - 1) // G
    for _ in range(E_):
        b = wpool[rng.integers(0, len(wpool), (C, K))]
        b[:, hot] = 0
        b = dup(b)
        sb = full_f32(rng, (NB, Gk), -5, -4)
        for g in range(npair):
            sb[:, g] = full_f32(rng, NB, 3.0 * g, 3.0 * g + 1)
            sb[:, g + npair] = -(sb[:, g] * (np.float32(1) + full_f32(rng, NB, -20, -10)))
        ws.append((b, sb))
    return x, a_codes, sa, ws


# The decode tests' cases, shared by the CPU and the GPU file: (E, topk, T, K, C, ks, kind). K is the folded width (down:
# N; gate_up: H), C the output columns of the entry (down: H; gate_up: N, the weight holding 2 C rows), ks the K slices
# of the tile width geometry() picks (ct = 32: 2; ct = 64 and 128: 1). kind: "" windows (decode_operands), "scales"
# the same with a NaN and a zero sb entry, "cancel" decode_cancel_operands, "span" F-x.
DOWN_CASES = [(4, 2, 16, 640, 256, 2, ""), (4, 2, 16, 1152, 256, 2, ""), (4, 2, 16, 640, 256, 2, "scales"),
              (64, 4, 16, 128, 1024, 1, ""), (64, 4, 16, 384, 2048, 1, ""),
              (4, 2, 16, 640, 256, 2, "cancel"), (4, 2, 16, 1152, 256, 2, "cancel"),
              (64, 4, 16, 640, 1024, 1, "cancel"), (64, 4, 16, 640, 2048, 1, "cancel")]
GATE_UP_CASES = [(4, 2, 16, 640, 256, 2, ""), (4, 2, 16, 1152, 256, 2, ""), (4, 2, 16, 640, 256, 2, "zero_sb"),
                 (64, 4, 16, 128, 1024, 1, ""), (64, 4, 16, 384, 2048, 1, "")]
SPAN_CASE = (4, 2, 16, 640, 256, 2, "span")


def decode_case(case, gate_up: bool = False):
    """The operands of one decode case: (x, a_codes, sa, ws, flat) - fp16 rows (down: one per pair; gate_up: one per
    token), their known codes and scales, per expert (codes, sb) of [C or 2 C, K], and the expert of every pair
    (pair p goes to expert p % E). gate_up keeps |g|, |u| small (e in -1 .. 1, gain 1/8) so the gated product stays
    inside fp16."""
    E_, topk, T, K, C, ks, kind = case
    rows, cols = (T, 2 * C) if gate_up else (T * topk, C)
    seed = (2700 if gate_up else 2600) + K + C + 7 * len(kind)
    if kind == "cancel":
        x, a_codes, sa, ws = decode_cancel_operands(rows, E_, cols, K, seed)
    elif kind == "span":
        x, a_codes, sa, ws = decode_operands(rows, E_, cols, K, seed, wa=(5, 8), wb=(5, 8), span_break=True)
    else:
        kw = dict(e_span=1, gain=0.125) if gate_up else {}
        x, a_codes, sa, ws = decode_operands(rows, E_, cols, K, seed, **kw)
    if kind == "scales":  # F-c: a NaN sb entry on expert 0 (block 0), a zero one on expert 1 (the last block)
        ws[0][1][0, 1] = np.nan
        ws[1][1][-1, 0] = 0.0
    if kind == "zero_sb":
        ws[1][1][-1, 0] = ws[0][1][0, 1] = 0.0
    flat = [p % E_ for p in range(T * topk)]
    return x, a_codes, sa, ws, flat


def decode_probs(case, gate_up: bool = False) -> list[Prob]:
    """A decode case as one Prob per expert that has rows (its rows in pair order), info['rows'] the pairs."""
    E_, topk, T, K, C, ks, kind = case
    x, a_codes, sa, ws, flat = decode_case(case, gate_up)
    g = 2.0 ** -5 if kind in ("cancel", "span") else None
    out = []
    for e in sorted(set(flat)):
        ps = [p for p, f in enumerate(flat) if f == e]
        src = [p // topk for p in ps] if gate_up else ps
        out.append(_finish(len(ps), ws[e][0].shape[0], K, (a_codes[src], sa[src], *ws[e]), family="decode", kind=kind,
                           ga=g or window_granule(W_MID_LO[0]), gb=g or window_granule(W_MID_HI[0]), rows=ps, x=x[src], ks=ks))
    return out


# ------------------------------------------------------------------ wrong arithmetic, restated in numpy
MUTANTS = ("descending", "split_scale", "unfused", "one_sum", "sb_neighbour", "sa_neighbour")


def applies(name: str, p: Prob) -> bool:
    """Whether a mutant can differ on a problem at all: the fold mutants need two groups, a neighbouring block two
    blocks, a neighbouring row two rows, the wrong split point of two slices an odd group count of at least 3."""
    Gk, NB = p.K // G, (p.N + G - 1) // G
    return {"descending": Gk >= 2, "unfused": Gk >= 2, "one_sum": Gk >= 2, "split_scale": True, "sb_neighbour": NB >= 2,
            "sa_neighbour": p.M >= 2, "floor_split": Gk >= 3 and Gk % 2 == 1}[name]


def mutant(p: Prob, name: str, ks: int = 1) -> np.ndarray:
    """fp16 [M, N] of a body that gets the contract wrong in one way (ks > 1: inside every K slice of the decode
    kernel's order, the slices' sums then added as the kernel adds them):
      descending ..... the groups (of a slice) folded last to first
      split_scale .... out = fmaf(f32_rn(acc_g sa), sb, out) instead of fmaf(acc_g, f32_rn(sa sb), out)
      unfused ........ out = f32_rn(out + f32_rn(acc_g s)): the product rounded on its own
      one_sum ........ one f32 sum over all of K times the first group's scale product (accumulating in the MFMA)
      sb_neighbour ... sb read from the next block (cyclically)
      sa_neighbour ... sa read from the next row (cyclically)
      floor_split .... two K slices split at floor(G / 2) instead of ceil(G / 2) (against gemm_fold_f32_sliced)"""
    a, sa, b, sb = p.ops
    if name == "sb_neighbour":
        return ref.gemm_fold_f32_sliced(a, sa, b, np.roll(sb, -1, axis=0), ks)
    if name == "sa_neighbour":
        return ref.gemm_fold_f32_sliced(a, np.roll(sa, -1, axis=0), b, sb, ks)
    if name == "floor_split":
        return ref.gemm_fold_f32_sliced(a, sa, b, sb, 2, split=lambda g, ks: g // ks)
    accs = [x.astype(np.float32) for x in group_accs(p)]
    scales = ref.scale_products(sa, sb, p.N)
    sbn = np.repeat(sb, G, axis=0)[:p.N]
    if name == "one_sum":
        with np.errstate(invalid="ignore", over="ignore"):
            return ref.to_f16(sum(accs[1:], accs[0]) * scales[0])
    parts = []
    with np.errstate(invalid="ignore", over="ignore"):
        for g0, g1 in ref.slice_bounds(len(accs), ks):
            out = np.zeros((p.M, p.N), np.float32)
            if name == "descending":
                out = ref.fold_f32(accs, scales, range(g1 - 1, g0 - 1, -1))
            elif name == "split_scale":
                for g in range(g0, g1):
                    out = ref.fma32(accs[g] * sa[:, g][:, None], np.broadcast_to(sbn[:, g][None, :], out.shape), out)
            else:
                assert name == "unfused"
                for g in range(g0, g1):
                    out = out + accs[g] * scales[g]
            parts.append(out)
        out = parts[0]
        for q in parts[1:]:
            out = out + q
    return ref.to_f16(out)
