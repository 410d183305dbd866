"""Edge-value operands for the w8a8_g-1_sym_E4M3 (QT_F8) and bf16 (QT_BF16) GroupGEMM bodies
(tests/test_fp8_bf16_edges.py on the CPU, tests/test_fp8_bf16_edges_gpu.py on the GPU).

Every generator is pure numpy and seeded and returns a ``tests._util.Raw``; both files call the same
ones, so what the CPU file proves about a family holds for what the GPU file runs.

The comparison rule is bit for bit against the f64 oracle, with no tolerance. Both bodies sum f32
products in an unspecified order, so the inputs are built to make the order irrelevant: all products
of a problem are multiples of a granule g, and for every (row, column) pair sum |a_k b_k| / g < 2^24.
Then every partial sum, in any order and any grouping, is a multiple of g below 2^24 g: exact in f32.
``Raw.info`` carries the granules (``ga``, ``gb``) and the bound (``bound`` = max over pairs of
sum |a_k b_k| / (ga gb)); ``exact_bound`` recomputes it from the operands. The readout and
non-finite problems have at most one (two, where said) nonzero product per pair instead
(``info['one_product']``), which a normal f32 holds exactly (8 x 8 significand bits).

E4M3 operands are bytes in the kernel's order: byte k of an A row meets byte k of a B row (pack_wxax
swaps the two bytes of each 16-bit word on both sides alike, oracle/gg_oracle.c oracle_gg_e4m3), so
the generators place codes by byte position and the readouts name byte positions.
"""
from __future__ import annotations

import numpy as np

from mxmoe_amd.groupgemm import BF16, W8A8_E4M3
from tests._util import LADDER_A, LADDER_B, Raw, p2

# ------------------------------------------------------------------ E4M3 codes
E4M3_NAN = (0x7F, 0xFF)


def e4m3_values() -> np.ndarray:
    """f64 value of each of the 256 OCP e4m3 codes (S.EEEE.MMM, bias 7, no infinities; S.1111.111 is
    NaN): m 2^-9 for exponent field 0, (8 + m) 2^(e - 10) otherwise. Every finite one is a multiple of
    2^-9, at most 448, and an fp16 value."""
    c = np.arange(256)
    e, m = (c >> 3) & 15, c & 7
    mag = np.where(e == 0, m * 2.0 ** -9, (8 + m) * 2.0 ** (e - 10.0))
    v = np.where(c & 0x80, -mag, mag)
    v[list(E4M3_NAN)] = np.nan
    return v


E4M3 = e4m3_values()


def window_codes(lo: int, hi: int) -> np.ndarray:
    """Every finite code, both signs, whose exponent field lies in [lo, hi]."""
    c = np.arange(256)
    e = (c >> 3) & 15
    return c[(e >= lo) & (e <= hi) & ((c & 0x7F) != 0x7F)].astype(np.uint8)


def window_granule(lo: int) -> float:
    """The common granule of a window starting at exponent field lo (fields 0 and 1 share 2^-9)."""
    return 2.0 ** (max(lo, 1) - 10)


# Exponent-field windows: |v| <= 15 * 2^-7 (subnormal and low-normal codes, granule 2^-9),
# two middle windows, and the top one (|v| in [32, 448], granule 4). A window [lo, hi] has
# max |v| / granule <= 15 * 2^(hi - max(lo, 1)); a pair of windows with spans sA + sB <= 7 keeps
# K * 225 * 2^(sA + sB) < 2^24 up to K = 582 (K = 256 and 432 here), sA + sB <= 3 up to K = 9320.
W_LOW, W_MID_LO, W_MID_HI, W_TOP = (0, 3), (4, 7), (8, 11), (12, 15)
EA_WINDOWS = [(W_LOW, W_LOW), (W_TOP, W_TOP), (W_LOW, W_TOP), (W_TOP, W_LOW), (W_MID_LO, W_MID_HI), (W_MID_HI, W_MID_LO)]
EA_SHAPES = [(300, 264, 256), (130, 136, 432)]  # a 256-row tile + tail-class tile + N tail | 3 stages + 48 B
W_SPLITK = ((6, 7), (6, 8))  # spans 1 + 2: the bound holds at K = 8192
W_LADDER = ((5, 8), (5, 8))  # |v| in [0.25, 3.75], granule 2^-5


def _window_rows(rng, rows: int, K: int, win) -> np.ndarray:
    """Bytes drawn uniformly from a window's codes; the window's whole code list stands at the start
    of row 0 and at the end of the last row (inside the K tail when there is one)."""
    codes = window_codes(*win)
    assert len(codes) <= K
    x = codes[rng.integers(0, len(codes), (rows, K))]
    x[0, :len(codes)] = codes
    x[rows - 1, K - len(codes):] = codes
    return x


def exact_bound(raw: Raw) -> float:
    """max over (row, column) pairs of sum_k |a_k b_k| / (ga gb), from the operands in f64; asserts that
    every operand is a multiple of its granule. Below 2^24 every partial sum is exact in f32."""
    a, b = operand_values(raw)
    ga, gb = raw.info["ga"], raw.info["gb"]
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert (a / ga == np.rint(a / ga)).all() and (b / gb == np.rint(b / gb)).all(), "an operand is off its granule"
    return float((np.abs(a / ga) @ np.abs(b / gb).T).max()) if a.size and b.size else 0.0


def operand_values(raw: Raw) -> tuple[np.ndarray, np.ndarray]:
    """f64 values of A [M, K] and B [N, K] (E4M3: by byte position)."""
    if raw.q.is_fp8:
        return E4M3[raw.A], E4M3[raw.B]
    return bf16_f64(raw.A), bf16_f64(raw.B)


def _pow2_scales(acc_max: float, M: int, N: int) -> tuple[np.ndarray, np.ndarray]:
    """sa = sb = 1 unless the largest |sum| would pass 2^15: then powers of two with sa sb = 2^-k, the
    smallest k that brings it to 2^15 or less (a power-of-two product rescales exactly)."""
    k = 0 if acc_max <= 2.0 ** 15 else int(np.ceil(np.log2(acc_max / 2.0 ** 15)))
    return np.full(M, p2(-(k // 2)), np.float16), np.full(N, p2(-(k - k // 2)), np.float16)


def gen_e4m3_window(M: int, N: int, K: int, wa, wb, seed: int) -> Raw:
    """E-a / E-d: A bytes from window wa, B bytes from window wb, every code of each window present."""
    rng = np.random.default_rng(seed)
    A, B = _window_rows(rng, M, K, wa), _window_rows(rng, N, K, wb)
    acc = E4M3[A] @ E4M3[B].T
    sa, sb = _pow2_scales(float(np.abs(acc).max()), M, N)
    raw = Raw(M, N, K, W8A8_E4M3, A, B, sa, sb, info=dict(wa=wa, wb=wb, ga=window_granule(wa[0]), gb=window_granule(wb[0])))
    raw.info["bound"] = exact_bound(raw)
    return raw


def e4m3_window_problems() -> list[Raw]:
    """E-a: the ladder of window pairs, each at both shapes."""
    return [gen_e4m3_window(M, N, K, wa, wb, seed=800 + 2 * i + j)
            for i, (wa, wb) in enumerate(EA_WINDOWS) for j, (M, N, K) in enumerate(EA_SHAPES)]


def e4m3_splitk_problems() -> list[Raw]:
    """E-d: the two shapes of test_low_fill_split_k (K = 8192) on exact data."""
    return [gen_e4m3_window(M, 256, 8192, *W_SPLITK, seed=830 + i) for i, M in enumerate((256, 96))]


READOUT_K, READOUT_N = 256, 264
NAN_ROW_STEP = 15  # rows r % 15 == 5 keep their NaN codes: r % 16 walks through all 16 byte positions


def gen_e4m3_readout(side: str, seed: int, ea: int = 0, eb: int = 0) -> Raw:
    """E-b: M = K = 256, N = 264. side "B": A is a permuted identity of code 0x38 (1.0) and row n of B
    holds code (k + n) % 256 at byte k, so over the rows every code stands at every byte position of
    the row (every byte of a 16-B chunk, every chunk of a 128-B stage): C[m, n] = value(B[n, pi[m]]).
    side "A": the mirror, B[n] one-hot at pi[n % 256], C[m, n] = value(A[m, pi[n % 256]]).
    A dot product runs over the whole row, and 0 * NaN is NaN, so the NaN codes 0x7F / 0xFF stay only
    in the rows r % 15 == 5 of the cycling operand (there they poison the whole output column / row);
    in the other rows they are replaced by +-448 (0x7E / 0xFE). sa = 2^-ea, sb = 2^-eb."""
    rng = np.random.default_rng(seed)
    K, N = READOUT_K, READOUT_N
    rows = N if side == "B" else K
    codes = ((np.arange(K)[None, :] + np.arange(rows)[:, None]) % 256).astype(np.uint8)
    nan_rows = np.arange(rows) % NAN_ROW_STEP == 5
    swap = ((codes & 0x7F) == 0x7F) & ~nan_rows[:, None]
    codes[swap] -= 1
    pi = rng.permutation(K)
    if side == "B":
        A = np.zeros((K, K), np.uint8)
        A[np.arange(K), pi] = 0x38
        B = codes
        src = codes[:, pi].T  # code read by C[m, n]
    else:
        A = codes
        B = np.zeros((N, K), np.uint8)
        B[np.arange(N), pi[np.arange(N) % K]] = 0x38
        src = codes[:, pi[np.arange(N) % K]]
    return Raw(K, N, K, W8A8_E4M3, A, B, np.full(K, p2(-ea), np.float16), np.full(N, p2(-eb), np.float16),
               info=dict(side=side, pi=pi, src=np.ascontiguousarray(src), nan_rows=nan_rows, scale=2.0 ** -(ea + eb),
                         one_product=True))


def e4m3_readout_problems() -> list[Raw]:
    """E-b: B and A readouts at unit scales, then the B readout at sa sb = 2^-15 (itself a subnormal
    fp16 product; the values m 2^-9 become m 2^-24: fp16's subnormal grid, met exactly) and at 2^-16
    (m 2^-25: every odd m is a tie on that grid, and 2^-16 is a subnormal product too)."""
    return [gen_e4m3_readout("B", 840), gen_e4m3_readout("A", 841), gen_e4m3_readout("B", 842, 7, 8),
            gen_e4m3_readout("B", 843, 8, 8), gen_e4m3_readout("A", 844, 8, 8)]


def gen_e4m3_ladder(M: int, N: int, K: int, seed: int) -> Raw:
    """E-c: the LADDER_A / LADDER_B scales of tests/_util.py on codes of one exact window. A rows
    m % 5 == 0 are all code 0x00, m % 5 == 1 hold one nonzero code, and of the rest m % 7 == 3 are all -0 (0x80)."""
    assert M >= 30 and N >= 7
    rng = np.random.default_rng(seed)
    wa, wb = W_LADDER
    A, B = _window_rows(rng, M, K, wa), _window_rows(rng, N, K, wb)
    ca = window_codes(*wa)
    for m in range(M):
        if m % 5 == 0:
            A[m] = 0x00
        elif m % 5 == 1:
            A[m] = 0x00
            A[m, (7 * m) % K] = ca[m % len(ca)]
        elif m % 7 == 3:
            A[m] = 0x80
    raw = Raw(M, N, K, W8A8_E4M3, A, B, LADDER_A[np.arange(M) % 6].copy(), LADDER_B[np.arange(N) % 7].copy(),
              info=dict(wa=wa, wb=wb, ga=window_granule(wa[0]), gb=window_granule(wb[0])))
    raw.info["bound"] = exact_bound(raw)
    return raw


def e4m3_ladder_problems() -> list[Raw]:
    """E-c in the shapes ladder_problems uses for w8a8: one tile with tails, several tiles."""
    return [gen_e4m3_ladder(M, N, K, seed=850 + i) for i, (M, N, K) in enumerate([(37, 136, 256), (130, 264, 512)])]


# ------------------------------------------------------------------ bf16
def bf16_bits(x) -> np.ndarray:
    """bf16 bit patterns of f32-representable values that are exact in bf16 (asserted)."""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    assert ((u & 0xFFFF) == 0).all(), "a value is not a bf16 value"
    return (u >> 16).astype(np.uint16)


def bf16_f64(bits) -> np.ndarray:
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


BA_SHAPES = [(300, 264, 256), (130, 264, 216), (17, 264, 256), (300, 264, 216), (130, 264, 256), (17, 264, 216)]


def gen_bf16_exact(M: int, N: int, K: int, kind: str, seed: int) -> Raw:
    """B-a: "eighths": multiples of 1/8 with |v| <= 8 (7 significant bits: exact in bf16), products
    multiples of 2^-6 up to 64; "ints": integers in [-128, 128], products up to 2^14 (K < 1024). Row 0
    starts with the extreme pair at both signs and a -0."""
    rng = np.random.default_rng(seed)
    top, g = (64, 0.125) if kind == "eighths" else (128, 1.0)
    a = rng.integers(-top, top + 1, (M, K)).astype(np.float64) * g
    b = rng.integers(-top, top + 1, (N, K)).astype(np.float64) * g
    a[0, :3] = top * g, -top * g, -0.0
    b[0, :3] = top * g, top * g, 1.0
    raw = Raw(M, N, K, BF16, bf16_bits(a), bf16_bits(b), info=dict(kind=kind, ga=g, gb=g))
    raw.info["bound"] = exact_bound(raw)
    return raw


def bf16_exact_problems() -> list[Raw]:
    """B-a: M = 300 / 130 / 17 (the 256-, 128- and 64-row classes), N = 264, K = 256 and 216 (3 stages
    + 48 bytes) on eighths; the integers at the first three shapes."""
    return [gen_bf16_exact(M, N, K, "eighths", seed=860 + i) for i, (M, N, K) in enumerate(BA_SHAPES)] + \
           [gen_bf16_exact(M, N, K, "ints", seed=870 + i) for i, (M, N, K) in enumerate(BA_SHAPES[:3])]


def bf16_splitk_problems() -> list[Raw]:
    """B-a through the split-K shapes of test_low_fill_split_k (K = 4096)."""
    return [gen_bf16_exact(M, 256, 4096, "eighths", seed=880 + i) for i, M in enumerate((256, 96))]


BF16_KINDS = ("unit", "tie", "scaled", "subnormal")
# planted in row 1 of the "unit" patterns: 65280 (the last bf16 below fp16's 65504 / 65520 boundary) and
# 65536 (the first above: +-inf), both signs; 2^-25 and 1.5 * 2^-24 (ties on fp16's subnormal grid, to
# even: 0 and 2^-23), 1.75 * 2^-24 (nearest 2^-23, truncated 2^-24), 1.25 * 2^-25 (above the tie: 2^-24),
# 2^-26 (underflow to 0), and negatives of the ties
UNIT_PLANTED = (0x477F, 0x4780, 0xC77F, 0xC780, 0x3300, 0x33C0, 0x33E0, 0x3320, 0x3280, 0xB300, 0xB3C0, 0xB280)
SCALED_FIELDS = (1, 2, 5, 30, 60, 90, 100, 160, 180, 200, 230, 250, 254)  # B exponent fields far outside fp16's range


def gen_bf16_readout(side: str, kind: str, seed: int) -> Raw:
    """B-b: M = K = 256, N = 264, one operand one-hot per row (side "B": A row m holds h(pi[m]) at column
    pi[m], C[m, n] = fp16_rn(h(pi[m]) * B[n, pi[m]]); side "A": the mirror with B row n one-hot at
    pi[n % 256]). The other operand holds finite bf16 patterns P[r, k]:
      unit ....... h = 1.0; every exponent field 1..254 (row 0 holds each once), both signs, random mantissas,
                   and UNIT_PLANTED in row 1. A bf16 value has 8 significant bits and fp16 has 11, so one bf16
                   value never ties on fp16's NORMAL grid; it does on the subnormal grid.
      tie ........ h = 1 + 2^-7; exponents inside fp16's normal range, every second mantissa with low bits
                   1000: the 15-bit product's four dropped bits are 1000, a tie on the normal grid.
      scaled ..... column k holds exponent field SCALED_FIELDS[k % 13] and h(k) = 2^s(k) brings the product's
                   exponent to d(k) in [-26, 16]: values far outside fp16's range come back into it (and to its
                   subnormal grid, its overflow and its underflow). Every product is a normal f32.
      subnormal .. even columns hold f32-subnormal patterns (exponent field 0, mantissa 1..127: m 2^-133) and
                   h = 2^127 (products m 2^-6, exact fp16 values); odd columns normal values with h = 1.
                   info['sub'] marks the outputs that read a subnormal input."""
    assert kind in BF16_KINDS
    rng = np.random.default_rng(seed)
    K, N = READOUT_K, READOUT_N
    rows = N if side == "B" else K
    sign = rng.integers(0, 2, (rows, K)) << 15
    mant = rng.integers(0, 128, (rows, K))
    hot = np.full(K, 0x3F80)  # 1.0
    sub = np.zeros((rows, K), bool)
    if kind == "unit":
        e = rng.integers(1, 255, (rows, K))
        e[0, 1:255] = np.arange(1, 255)
        P = sign | (e << 7) | mant
        P[1, :len(UNIT_PLANTED)] = UNIT_PLANTED
    elif kind == "tie":
        e = rng.integers(127 - 10, 127 + 14, (rows, K))
        mant[:, ::2] = (mant[:, ::2] & 0x70) | 8
        P = sign | (e << 7) | mant
        hot[:] = 0x3F81
    elif kind == "scaled":
        eb = np.array(SCALED_FIELDS)[np.arange(K) % len(SCALED_FIELDS)]
        d = rng.integers(-26, 17, K)
        d[3:7] = 15, 16, -25, -24  # (fields 30 .. 100: 2^s stays inside bf16's range, d is met)
        s = np.clip(d - (eb - 127), -126, 127)
        mant[1, 3:7] = 0x7F, 0, 0, 0x40  # 65280 | 65536 | the ties 2^-25 and 1.5 * 2^-24
        P = sign | (eb[None, :] << 7) | mant
        hot = (s + 127) << 7
    else:
        sub[:, 0::2] = True
        msub = rng.integers(1, 128, (rows, K))
        msub[2, 0], msub[2, 2], msub[3, 0], msub[3, 2] = 1, 127, 1, 127
        sign[2, 0], sign[2, 2], sign[3, 0], sign[3, 2] = 0, 0, 1 << 15, 1 << 15
        e = rng.integers(127 - 8, 127 + 8, (rows, K))
        P = np.where(sub, sign | msub, sign | (e << 7) | mant)
        hot = np.where(np.arange(K) % 2 == 0, 254 << 7, 0x3F80)
    P = P.astype(np.uint16)
    pi = rng.permutation(K)
    if side == "B":
        A = np.zeros((K, K), np.uint16)
        A[np.arange(K), pi] = hot[pi]
        B = P
        col = pi[:, None] + np.zeros((1, N), np.int64)  # the K column read by C[m, n]
        src, submask = P[:, pi].T, sub[:, pi].T
    else:
        A = P
        B = np.zeros((N, K), np.uint16)
        pn = pi[np.arange(N) % K]
        B[np.arange(N), pn] = hot[pn]
        col = pn[None, :] + np.zeros((K, 1), np.int64)
        src, submask = P[:, pn], sub[:, pn]
    return Raw(K, N, K, BF16, A, B, info=dict(side=side, kind=kind, pi=pi, src=np.ascontiguousarray(src),
                                              hot=hot[col].astype(np.uint16), sub=np.ascontiguousarray(submask),
                                              one_product=True))


def bf16_readout_problems(kind: str) -> list[Raw]:
    """B-b: the B readout and its mirror for one kind."""
    i = BF16_KINDS.index(kind)
    return [gen_bf16_readout("B", kind, seed=890 + 2 * i), gen_bf16_readout("A", kind, seed=891 + 2 * i)]


BF16_INF, BF16_NINF, BF16_NAN, BF16_NAN2, BF16_2P100 = 0x7F80, 0xFF80, 0x7FC0, 0xFFC1, (100 + 127) << 7


def gen_bf16_nonfinite(kind: str, seed: int) -> Raw:
    """B-c: M = 130, N = 136, K = 216 of eighths, with
      "inf" / "inf_flipped": one infinity in A row r1 (column k1) and one of the other sign in B row c1
          (column k2), one NaN pattern in A row r2 and one in B row c2. The columns k1 of B and k2 of A
          hold no zero (no 0 x inf anywhere), and at (r1, c1) both infinite products are of one sign, so no
          output sums infinities of opposite sign: rows r1 / columns c1 are +-inf by the sign of the
          finite factor, rows r2 / columns c2 NaN, every other output an exact sum.
      "overflow": A[r3, k5] = B[c3, k5] = 2^100: one product overflows f32 to +inf; the rest of row r3
          and column c3 is +-2^100 b, beyond fp16 (or an exact sum where b = 0).
    info['rows'] / info['cols'] list the affected rows and columns."""
    rng = np.random.default_rng(seed)
    M, N, K = 130, 136, 216
    a = rng.integers(-64, 65, (M, K)).astype(np.float64) / 8
    b = rng.integers(-64, 65, (N, K)).astype(np.float64) / 8
    flip = kind == "inf_flipped"
    r1, r2, r3, c1, c2, c3 = (7, 64, 129, 135, 3, 70) if not flip else (129, 0, 5, 0, 131, 9)
    k1, k2, k3, k4, k5 = (5, 100, 37, 150, 77) if not flip else (200, 215, 193, 208, 77)  # flipped: inside the K tail
    for x, k in ((b, k1), (a, k2)):
        x[:, k] = np.where(x[:, k] == 0, 0.125, x[:, k])
    A, B = bf16_bits(a), bf16_bits(b)
    if kind == "overflow":
        A[r3, k5] = B[c3, k5] = BF16_2P100
        rows, cols = [r3], [c3]
    else:
        A[r1, k1], B[c1, k2] = (BF16_NINF, BF16_INF) if flip else (BF16_INF, BF16_NINF)
        # (r1, c1): inf * B[c1, k1] and A[r1, k2] * (-+inf) must agree in sign
        B[c1, k1], A[r1, k2] = 0xBF80, 0x3F80  # -1.0, 1.0
        A[r2, k3], B[c2, k4] = (BF16_NAN2, BF16_NAN) if flip else (BF16_NAN, BF16_NAN2)
        rows, cols = [r1, r2], [c1, c2]
    return Raw(M, N, K, BF16, A, B, info=dict(kind=kind, rows=rows, cols=cols, ga=0.125, gb=0.125))


def bf16_nonfinite_problems() -> list[Raw]:
    return [gen_bf16_nonfinite(kind, seed=900 + i) for i, kind in enumerate(("inf", "inf_flipped", "overflow"))]


# ------------------------------------------------------------------ numpy restatements (true and wrong)
def f16_bits(x) -> np.ndarray:
    return np.ascontiguousarray(x, np.float16).view(np.uint16)


def to_f16(x: np.ndarray, mode: str = "rn") -> np.ndarray:
    """f32 / f64 -> fp16: "rn" nearest even with overflow to +-inf (the definition), "sat" the same but
    +-65504 where rn overflows, "trunc" towards zero (finite inputs beyond 65504 stay 65504)."""
    with np.errstate(over="ignore"):
        r = np.asarray(x).astype(np.float16)
    if mode == "rn":
        return r
    fin = np.isfinite(x)
    if mode == "sat":
        return np.where(fin & np.isinf(r), np.copysign(np.float16(65504), r), r).astype(np.float16)
    assert mode == "trunc"
    over = np.abs(r.astype(np.float64)) > np.abs(x)  # rounded away from zero: step back
    back = np.nextafter(r, np.float16(0)).astype(np.float16)
    out = np.where(fin & over, back, r).astype(np.float16)
    return np.where((out == 0) & fin, np.copysign(np.float16(0), x), out).astype(np.float16)


def _subnormal16(x) -> np.ndarray:
    b = f16_bits(x) & 0x7FFF
    return (b > 0) & (b < 0x0400)


def np_gg_e4m3(raw: Raw, flush: bool = False, mode: str = "rn") -> np.ndarray:
    """oracle_gg_e4m3 in numpy: fp16(0 + f32(exact sum) * f32(fp16_rn(sa sb))). flush: a subnormal
    scale product becomes 0; mode: the output conversion (to_f16)."""
    a, b = operand_values(raw)
    with np.errstate(invalid="ignore"):
        acc = (np.nan_to_num(a) @ np.nan_to_num(b).T)
    acc = np.where(np.isnan(a).any(axis=1)[:, None] | np.isnan(b).any(axis=1)[None, :], np.nan, acc)
    s16 = (raw.sa.astype(np.float64)[:, None] * raw.sb.astype(np.float64)[None, :]).astype(np.float16)
    if flush:
        s16 = np.where(_subnormal16(s16), np.float16(0), s16)
    with np.errstate(over="ignore", invalid="ignore"):
        v = np.float32(0) + acc.astype(np.float32) * s16.astype(np.float32)
    return to_f16(v, mode)


def np_gg_bf16(raw: Raw, mode: str = "rn") -> np.ndarray:
    """oracle_gg_bf16 in numpy for FINITE operands: fp16(f32(exact f64 sum))."""
    a, b = operand_values(raw)
    with np.errstate(over="ignore"):
        return to_f16((a @ b.T).astype(np.float32), mode)


def mismatch(out: np.ndarray, ref: np.ndarray) -> np.ndarray:
    """Where out differs from ref: NaN compares by isnan (not by payload), everything else bit for bit."""
    no, nr = np.isnan(out), np.isnan(ref)
    return (no != nr) | (~no & ~nr & (f16_bits(out) != f16_bits(ref)))
