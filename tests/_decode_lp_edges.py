"""Edge-value operands for the decode forward's MFMA tile (mxmoe_amd/csrc/moe_decode_mfma.h; the _lp entries
mxmoe_moe_decode_gate_up_lp / mxmoe_moe_decode_down_lp): tests/test_decode_lp_edges.py on the CPU,
tests/test_decode_lp_edges_gpu.py on the GPU.

Every generator is numpy and seeded; both files call the same ones, so what the CPU file proves about a family holds
for what the GPU file runs. Operands are canonical: fp16 A rows (the kernel quantises them itself), E4M3 weights as
uint8 codes [rows, K] in logical K order with fp16 row scales, MX weights as e2m1 nibbles [rows, K] (one per byte) with
e8m0 bytes [rows, K / 32].

The comparison rule is tests/_fp8_bf16_edges.py's: bit for bit against float64 arithmetic on the operands the contract
defines (quantize.quant_e4m3 / quant_mxfp8 / quant_mxfp4 of the A rows, the weights' values), one rounding to fp16, no
tolerance. The MFMA sums f32 products in an order of its own, so the inputs make the order irrelevant: with ga[r] and
gb[c] the largest powers of two that divide every value of A row r and of weight row c (for the block-scaled kinds
after the e8m0 scales are applied), every product of the pair is a multiple of ga[r] gb[c], and the generators keep
max over pairs of sum_k |a_k b_k| / (ga gb) (``exact_bound``) below BOUND: 2^24 for E4M3 (tests/_fp8_bf16_edges.py,
module docstring), 2^23 for the block-scaled kinds (tests/test_mxfp8_a8_gpu.py line 7: "23 bits, exact in f32 in any
order"). The readout family has one nonzero product per output instead.
"""
from __future__ import annotations

import dataclasses
import functools

import numpy as np
import torch

from mxmoe_amd import quantize as qz
from tests._fp8_bf16_edges import E4M3, to_f16, window_codes

KINDS = ("e4m3", "mxfp8", "mxfp4")
# the two kinds of expert_tile (VALU dot products: integer sums, resp. f32 sums in the kernel's order) that stand
# beside the three in the wide-tile family
# ("w4a16": w4a16_g-1_asym weights that are integers in [-8, 7] times a power of two with both ends in every row, so
# that quant_weightonly returns them unchanged; to the reference an fp16 weight)
OTHER_KINDS = ("w8a8", "fp16", "w4a16")
BOUND = {"e4m3": 2.0 ** 24, "mxfp8": 2.0 ** 23, "mxfp4": 2.0 ** 23, "w8a8": 2.0 ** 24, "fp16": 2.0 ** 24, "w4a16": 2.0 ** 24}
E2M1 = np.array(list(qz.E2M1_VALUES) + [-v for v in qz.E2M1_VALUES])  # value of a nibble
E2M1_TIES = (0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0)
E4M3_POS = np.sort(E4M3[:0x7F])  # the 127 finite non-negative values
E4M3_TIES = (E4M3_POS[:-1] + E4M3_POS[1:]) / 2  # 126 midpoints: 5 significant bits, fp16 values at any scale used here
ONE8, TOP8, TOP8_MX, ONE4, TOP4 = 0x38, 0x7E, 0x78, 2, 6  # e4m3 1.0, 448, 256; e2m1 1.0, 4.0


# ------------------------------------------------------------------ operands
@dataclasses.dataclass
class Weight:
    """One linear's weight, canonical. e4m3: codes uint8 [rows, K], scales fp16 [rows]; MX: nibbles uint8 [rows, K],
    scales uint8 e8m0 [rows, K / 32]; w8a8: integers [rows, K] in +-127 with 127 in every row and power-of-two fp16
    scales [rows] (quant_rtn_sym of fp16() returns them); fp16: the values themselves, no scales."""

    kind: str
    codes: np.ndarray
    scales: np.ndarray

    @property
    def mx(self) -> bool:
        return self.kind == "mxfp4"

    def fp16(self) -> np.ndarray:
        """w8a8 / fp16: the fp16 tensor the layer is built from"""
        if self.kind in ("fp16", "w4a16"):
            return self.codes
        v = self.codes.astype(np.float64) * self.scales.astype(np.float64)[:, None]
        assert self.kind == "w8a8" and np.array_equal(v.astype(np.float16).astype(np.float64), v)
        return v.astype(np.float16)

    def values(self) -> np.ndarray:
        """f64 [rows, K]: E4M3 the code values (the row scale stays apart), MX the scaled values."""
        if self.kind in OTHER_KINDS:
            return self.codes.astype(np.float64)
        if not self.mx:
            return E4M3[self.codes]
        s = np.exp2(self.scales.astype(np.float64) - 127)
        return E2M1[self.codes] * np.repeat(s, 32, axis=1)

    def packed(self) -> np.ndarray:
        """MX: uint8 [rows, K / 2], the low nibble the even element."""
        return (self.codes[:, 0::2] | (self.codes[:, 1::2] << 4)).astype(np.uint8)


def quant_a(kind: str, x: np.ndarray):
    """fp16 rows through the kind's activation quantiser (mxmoe_amd.quantize): (codes, scales) as numpy."""
    fn = {"e4m3": qz.quant_e4m3, "mxfp8": qz.quant_mxfp8, "mxfp4": qz.quant_mxfp4}[kind]
    c, s = fn(torch.from_numpy(np.ascontiguousarray(x, np.float16)))
    return c.numpy(), s.numpy()


def a_values(kind: str, x: np.ndarray):
    """The A operand of fp16 rows: (f64 [R, K], fp16 row scales or None). E4M3: the code values, a row holding an Inf
    or a NaN all NaN (zero codes and a NaN scale: 0 * NaN); MX: the scaled values, NaN in a block whose byte is 255."""
    if kind in ("fp16", "w4a16"):
        return x.astype(np.float64), None
    if kind == "w8a8":
        c, s = qz.quant_rtn_sym(torch.from_numpy(np.ascontiguousarray(x, np.float16)), 8)
        return c.numpy().astype(np.float64), s.numpy()
    c, s = quant_a(kind, x)
    if kind == "e4m3":
        v = E4M3[c].copy()
        v[~np.isfinite(x.astype(np.float64)).all(axis=1)] = np.nan
        return v, s
    t = lambda a: torch.from_numpy(a)
    return (qz.dequant_mxfp8 if kind == "mxfp8" else qz.dequant_mxfp4)(t(c), t(s)).numpy(), None


def ref_linear(kind: str, x: np.ndarray, w: Weight, wrong: str = "") -> np.ndarray:
    """fp16 [R, rows]: the contract of one linear of the kind on fp16 A rows. MX: fp16_rn(f64 sum). E4M3:
    fp16_rn(f32(sum) * f32(fp16_rn(sa * sb))), the sum exact by the bound (a NaN scale: NaN). ``wrong`` names a
    deliberately wrong variant (the CPU file's sensitivity checks):
      "scale_once"  E4M3: acc * sa * sb with one rounding at the end
      "tie_away"    the output conversion rounds ties away from zero"""
    a, sa = a_values(kind, x)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = a @ w.values().T
        if kind == "w8a8":  # acc * fp16_rn(sa * sb); exact whatever the epilogue's order where both are powers of two
            s16 = (sa.astype(np.float64)[:, None] * w.scales.astype(np.float64)[None, :]).astype(np.float16)
            return _f16(acc * s16.astype(np.float64), wrong)
        if kind != "e4m3":
            return _f16(acc, wrong)
        if wrong == "scale_once":
            return _f16(acc * sa.astype(np.float64)[:, None] * w.scales.astype(np.float64)[None, :], "")
        s16 = (sa.astype(np.float64)[:, None] * w.scales.astype(np.float64)[None, :]).astype(np.float16)
        return _f16((np.float32(0) + acc.astype(np.float32) * s16.astype(np.float32)).astype(np.float64), wrong)


def _f16(v: np.ndarray, wrong: str) -> np.ndarray:
    r = to_f16(v)
    if wrong != "tie_away":
        return r
    # a tie: v exactly between r and its neighbour away from zero (r was the even one and lies nearer zero)
    away = np.nextafter(r, np.copysign(np.float16(np.inf), r)).astype(np.float16)
    with np.errstate(invalid="ignore", over="ignore"):
        tie = np.isfinite(v) & np.isfinite(away) & (np.abs(v) > np.abs(r.astype(np.float64))) & \
            (v - r.astype(np.float64) == away.astype(np.float64) - v)
    return np.where(tie, away, r).astype(np.float16)


def row_granule(v: np.ndarray) -> np.ndarray:
    """Per row, the largest power of two that divides every nonzero value (1 for an all-zero row)."""
    m, e = np.frexp(np.where(np.isfinite(v), v, 0.0))
    mi = np.abs(m * 2.0 ** 53).astype(np.int64)
    low = np.where(mi == 0, 1, mi & -mi).astype(np.float64)
    ge = np.where(mi == 0, 4096, e - 53 + np.log2(low).astype(np.int64))
    ge = ge.min(axis=1)
    return np.exp2(np.where(ge == 4096, 0, ge).astype(np.float64))


def exact_bound(kind: str, x: np.ndarray, w: Weight) -> float:
    """max over (row, weight row) of sum_k |a_k b_k| / (ga gb) of the operands the kernel multiplies; rows holding a
    non-finite value are left out (their outputs are compared by class)."""
    a, _ = a_values(kind, x)
    a = a[np.isfinite(a).all(axis=1)]
    b = w.values()
    if not a.size:
        return 0.0
    return float(((np.abs(a) / row_granule(a)[:, None]) @ (np.abs(b) / row_granule(b)[:, None]).T).max())


SPAN = 2.0 ** 14


def exact_span(kind: str, x: np.ndarray, w: Weight) -> float:
    """max over (row, weight row, k) of |a_k b_k| / (ga gb): how far the largest product of a sum stands above the
    sum's granule. Sums with one product 2^20.7 granules large came back inexact from the tile although exact in f32
    in any order (DESIGN.md §4 "Decode forward on MFMA": supposed to be the scaled MFMA dropping low bits of small
    products beside a much larger one; not separated from the kernel), so the dense families stay below SPAN = 2^14,
    about what the GroupGEMM's exact suites reach per product (tests/_fp8_bf16_edges.py, W_TOP x W_TOP: 448 * 448 / 16 =
    12544; tests/test_mxfp8_a8_gpu.py: 64 * 12 * 16 = 12288)."""
    if kind in OTHER_KINDS:  # (no MFMA)
        return 0.0
    a, _ = a_values(kind, x)
    a = a[np.isfinite(a).all(axis=1)]
    b = w.values()
    if not a.size:
        return 0.0
    a, b = np.abs(a) / row_granule(a)[:, None], np.abs(b) / row_granule(b)[:, None]
    return float(max((a[r][None, :] * b).max() for r in range(a.shape[0])))


# ------------------------------------------------------------------ exact A rows and weights
def rows_e4m3(rng, R: int, K: int, win, ks, top: int = 0, sign=None):
    """fp16 [R, K]: row r is 2^ks[r] times e4m3 values of window ``win`` with 448 * 2^ks[r] at column ``top``, so
    quant_e4m3 gives the scale 2^ks[r] and exactly these codes (returned). sign [K] of +-1: the columns' signs."""
    pool = window_codes(*win)
    c = pool[rng.integers(0, len(pool), (R, K))]
    c[:, top] = TOP8
    if sign is not None:
        c = ((c & 0x7F) | np.where(sign < 0, 0x80, 0)[None, :]).astype(np.uint8)
    x = E4M3[c] * np.exp2(np.asarray(ks, np.float64))[:, None]
    x16 = x.astype(np.float16)
    assert np.array_equal(x16.astype(np.float64), x)
    return x16, c


def rows_mx(kind: str, rng, R: int, K: int, win, bytes_, top: int = 0, sign=None):
    """fp16 [R, K]: block b of row r is 2^(bytes_[r, b] - 127) times code values (mxfp8: e4m3 window ``win``; mxfp4:
    any nibble) with the power of two that selects the byte (256, resp. 4, times the scale) at in-block position
    ``top``: quant_mxfp8 / quant_mxfp4 give these bytes and codes (returned)."""
    if kind == "mxfp8":
        pool = window_codes(*win)
        c = pool[rng.integers(0, len(pool), (R, K))]
        c[:, top::32] = TOP8_MX
        neg, val = 0x80, E4M3
    else:
        c = rng.integers(0, 16, (R, K)).astype(np.uint8)
        c[:, top::32] = TOP4
        neg, val = 8, E2M1
    if sign is not None:
        c = ((c & (neg - 1)) | np.where(sign < 0, neg, 0)[None, :]).astype(np.uint8)
    x = val[c] * np.repeat(np.exp2(bytes_.astype(np.float64) - 127), 32, axis=1)
    x16 = x.astype(np.float16)
    assert np.array_equal(x16.astype(np.float64), x)
    return x16, c


def exact_rows(kind: str, rng, R: int, K: int, win, lo: int, hi: int, top: int = 0, sign=None):
    """Exact A rows of a kind with scales drawn from [lo, hi]: E4M3 the row's exponent k (scale 2^k), MX the e8m0 byte
    of every block, independently. Returns (fp16 rows, codes, scales as the quantiser must report them)."""
    if kind == "fp16":  # the MXFP4 kind's rows: multiples of 2^-4 up to 6
        return exact_rows("mxfp4", rng, R, K, None, 124, 127, top, sign)
    if kind == "w8a8":  # integers in +-127 times 2^k, 127 at ``top``: quant_rtn_sym gives the scale 2^k and the integers
        ks = rng.integers(-5, -3, R)
        c = rng.integers(-127, 128, (R, K))
        c[:, top] = 127
        x = c * np.exp2(ks.astype(np.float64))[:, None]
        return x.astype(np.float16), c, np.exp2(ks.astype(np.float64)).astype(np.float16)
    if kind == "e4m3":
        ks = rng.integers(lo, hi + 1, R)
        x, c = rows_e4m3(rng, R, K, win, ks, top, sign)
        return x, c, np.exp2(ks.astype(np.float64)).astype(np.float16)
    b = rng.integers(lo, hi + 1, (R, K // 32)).astype(np.uint8)
    x, c = rows_mx(kind, rng, R, K, win, b, top % 32, sign)
    return x, c, b


def assert_quantises_to(kind: str, x: np.ndarray, codes: np.ndarray, scales: np.ndarray) -> None:
    """The quantiser of mxmoe_amd.quantize returns the codes and scales the generator intended."""
    c, s = quant_a(kind, x)
    if kind == "mxfp4":
        c = np.stack([c & 0xF, c >> 4], axis=-1).reshape(c.shape[0], -1)
    assert np.array_equal(c, codes), "A codes differ from the intended ones"
    assert np.array_equal(s.view(np.uint16) if kind == "e4m3" else s, scales.view(np.uint16) if kind == "e4m3" else scales)


def weight_e4m3(rng, rows: int, K: int, win, scales, sign=None, fixed=None) -> Weight:
    """Window codes with fp16 row scales; sign [rows, K] of +-1 fixes the signs; fixed (column, code): one column
    holds that code's magnitude in every row."""
    pool = window_codes(*win)
    c = pool[rng.integers(0, len(pool), (rows, K))]
    if fixed is not None:
        c[:, fixed[0]] = fixed[1]
    if sign is not None:
        c = ((c & 0x7F) | np.where(sign < 0, 0x80, 0)).astype(np.uint8)
    return Weight("e4m3", c, np.broadcast_to(np.asarray(scales, np.float16), (rows,)).copy())


def weight_mx(rng, rows: int, K: int, lo: int, hi: int, sign=None, fixed=None, anchor: bool = False) -> Weight:
    """Random nibbles with per-block bytes drawn independently from [lo, hi]. fixed (in-block position, nibble): that
    position of every block holds the nibble's magnitude; anchor: in-block position 31 holds +-4 or +-6, so that
    quantising the dequantised block again (MoEFFN on fp16 tensors) returns the same byte."""
    c = rng.integers(0, 16, (rows, K)).astype(np.uint8)
    if anchor:
        c[:, 31::32] = (c[:, 31::32] & 8) | 6 | (c[:, 31::32] & 1)
    if fixed is not None:
        c[:, fixed[0]::32] = fixed[1]
    if sign is not None:
        c = ((c & 7) | np.where(sign < 0, 8, 0)).astype(np.uint8)
    return Weight("mxfp4", c, rng.integers(lo, hi + 1, (rows, K // 32)).astype(np.uint8))


def weight_kind(kind: str) -> str:
    """the weight format a kind's activations meet"""
    return kind if kind in ("e4m3",) + OTHER_KINDS else "mxfp4"


# ------------------------------------------------------------------ the down entry alone
@dataclasses.dataclass
class DownProblem:
    """One call of mxmoe_moe_decode_down_lp on raw expert records: expert e of kinds[e] (the shared one last) with
    weights[e] [H, K_e]; act [T * topk, N] and act_shared [T, Ns] fp16; ids [T, topk]."""

    name: str
    kinds: list
    weights: list
    ids: np.ndarray
    act: np.ndarray
    act_shared: np.ndarray
    H: int
    info: dict = dataclasses.field(default_factory=dict)

    @property
    def E(self) -> int:
        return len(self.kinds) - 1

    @functools.cached_property
    def expected(self):
        """(y [T * topk, H], ys [T, H]) fp16"""
        flat = self.ids.reshape(-1)
        y = np.stack([ref_linear(self.kinds[e], self.act[p:p + 1], self.weights[e])[0] for p, e in enumerate(flat)])
        return y, ref_linear(self.kinds[-1], self.act_shared, self.weights[-1])

    def wrong(self, variant: str, **kw):
        """``expected`` under a deliberately wrong kernel (see WRONG)"""
        flat = self.ids.reshape(-1)
        y = np.stack([wrong_linear(variant, self.kinds[e], self.act[p:p + 1], self.weights[e], **kw)[0]
                      for p, e in enumerate(flat)])
        return y, wrong_linear(variant, self.kinds[-1], self.act_shared, self.weights[-1], **kw)

    @functools.cached_property
    def bound(self) -> float:
        flat = self.ids.reshape(-1)
        b = [exact_bound(self.kinds[e], self.act[flat == e], self.weights[e]) for e in range(self.E) if (flat == e).any()]
        return max(b + [exact_bound(self.kinds[-1], self.act_shared, self.weights[-1])])

    @functools.cached_property
    def span(self) -> float:
        flat = self.ids.reshape(-1)
        b = [exact_span(self.kinds[e], self.act[flat == e], self.weights[e]) for e in range(self.E) if (flat == e).any()]
        return max(b + [exact_span(self.kinds[-1], self.act_shared, self.weights[-1])])

    def assert_exact(self) -> None:
        if self.info.get("one_product"):
            return
        lim = min(BOUND[k] for k in self.kinds)
        assert self.bound < lim, f"{self.name}: bound {self.bound:.3g} >= {lim:.3g}"
        assert self.span < SPAN, f"{self.name}: span {self.span:.3g} >= {SPAN:.3g}"


# ---- wrong kernels: what a mis-addressed or mis-rounded tile would compute
def _swap_bytes(sc: np.ndarray, how: str) -> np.ndarray:
    """e8m0 bytes [rows, K / 32] as a wrong kernel would pair them with the blocks. A K = 128 step u holds blocks
    4 u .. 4 u + 3 (K group g = block & 3); a dword of the device layout holds one K group's bytes of four steps.
      "neighbour"  block b reads the byte of block b ^ 1 (the next K group's dword)
      "step"       step u reads the byte of step u ^ 1 of its dword
      "group"      steps s0 > 0 of the second trip (s >= kSteps = 8) read the 16-byte group of s0 == 0"""
    nb = sc.shape[1]
    b = np.arange(nb)
    if how == "neighbour":
        src = b ^ 1
    elif how == "step":
        src = ((b >> 2) ^ 1) * 4 + (b & 3)
    else:
        src = np.where(b >= 32, b - 32, b)
    src = np.where(src < nb, src, b)
    return sc[:, src]


def wrong_linear(variant: str, kind: str, x: np.ndarray, w: Weight, side: str = "b") -> np.ndarray:
    """ref_linear as a kernel wrong in one way would give it:
      neighbour / step / group   MX: the weight's (side "b") or the A row's (side "a") e8m0 bytes mis-paired (_swap_bytes)
      halves       fp8 A: the two 64-byte halves of every K = 128 step of the A codes swapped
      scale_once / tie_away      ref_linear's
      no_floor     E4M3: the row scale without its 2^-14 floor
      quant_tie_away             the A quantiser rounds ties away from zero
      inf_kept     an Inf / NaN row (E4M3) or block (MX) quantised as if the value were 0 instead of zeroed with a NaN scale"""
    if variant in ("scale_once", "tie_away"):
        return ref_linear(kind, x, w, wrong=variant)
    if variant in ("neighbour", "step", "group"):
        if side == "b":
            return ref_linear(kind, x, Weight(w.kind, w.codes, _swap_bytes(w.scales, variant)))
        c, s = quant_a(kind, x)
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        a = (qz.dequant_mxfp8 if kind == "mxfp8" else qz.dequant_mxfp4)(t(c), t(_swap_bytes(s, variant))).numpy()
        with np.errstate(invalid="ignore", over="ignore"):
            return to_f16(a @ w.values().T)
    if variant == "halves":
        K = x.shape[1]
        idx = np.arange(K)
        idx = (idx & ~127) | ((idx & 127) ^ 64)
        a, sa = a_values(kind, x)
        a = a[:, idx]
        with np.errstate(invalid="ignore", over="ignore"):
            acc = a @ w.values().T
            if kind != "e4m3":
                return to_f16(acc)
            s16 = (sa.astype(np.float64)[:, None] * w.scales.astype(np.float64)[None, :]).astype(np.float16)
            return to_f16(np.float32(0) + acc.astype(np.float32) * s16.astype(np.float32))
    if variant == "no_floor":
        xf = x.astype(np.float32)
        amax = np.abs(xf).max(axis=1)
        s = np.where(amax == 0, np.float16(1), (amax / np.float32(448)).astype(np.float16))
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            q = np.clip(xf / s.astype(np.float32)[:, None], -448, 448)
            c = torch.from_numpy(np.nan_to_num(q)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
            acc = E4M3[c] @ w.values().T
            s16 = (s.astype(np.float64)[:, None] * w.scales.astype(np.float64)[None, :]).astype(np.float16)
            return to_f16(np.float32(0) + acc.astype(np.float32) * s16.astype(np.float32))
    if variant == "quant_tie_away":
        a, sa = _a_tie_away(kind, x)
        with np.errstate(invalid="ignore", over="ignore"):
            acc = a @ w.values().T
            if kind != "e4m3":
                return to_f16(acc)
            s16 = (sa.astype(np.float64)[:, None] * w.scales.astype(np.float64)[None, :]).astype(np.float16)
            return to_f16(np.float32(0) + acc.astype(np.float32) * s16.astype(np.float32))
    assert variant == "inf_kept"
    return ref_linear(kind, np.where(np.isfinite(x), x, np.float16(0)).astype(np.float16), w)


def _a_tie_away(kind: str, x: np.ndarray):
    """a_values with a quantiser that rounds ties away from zero: the scales are the true quantiser's, every scaled
    element goes to the nearest value of the code grid, the larger magnitude on a tie."""
    c, s = quant_a(kind, x)
    grid = E4M3_POS if kind != "mxfp4" else np.array(qz.E2M1_VALUES)
    xf = np.nan_to_num(x.astype(np.float64), nan=0.0, posinf=0.0, neginf=0.0)
    if kind == "e4m3":
        scale = s.astype(np.float64)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            y = (x.astype(np.float32) / s.astype(np.float32)[:, None]).astype(np.float64)
        y = np.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0)
    else:
        scale = np.repeat(np.exp2(np.where(s == 255, 127, s).astype(np.float64) - 127), 32, axis=1)
        y = xf / scale
    m = np.minimum(np.abs(y), grid[-1])
    i = np.clip(np.searchsorted(grid, m), 1, len(grid) - 1)
    lo, hi = grid[i - 1], grid[i]
    q = np.where(m - lo < hi - m, lo, hi) * np.sign(y)
    if kind == "e4m3":
        q[~np.isfinite(x.astype(np.float64)).all(axis=1)] = np.nan
        return q, s
    q = q * scale
    q[np.repeat(s == 255, 32, axis=1)] = np.nan
    return q, None


WRONG = ("quant_tie_away", "neighbour", "step", "group", "halves", "scale_once", "tie_away", "no_floor", "inf_kept")


def _ids_all(T: int, topk: int, e) -> np.ndarray:
    return np.full((T, topk), e, np.int32) if np.isscalar(e) else np.asarray(e, np.int32).reshape(T, topk)


def _routing(rng, T: int, E: int, topk: int) -> np.ndarray:
    return np.stack([rng.permutation(E)[:topk] for _ in range(T)]).astype(np.int32)


# ---- L-a: the A quantiser read out
LA_ROWS = ("zero", "neg_zero", "subnormal", "amax_65504", "below_floor", "ties", "ties_small", "ladder_lo", "ladder_hi",
           "inf", "nan", "exact", "exact_small", "randn", "randn_small", "randn_large")


def la_rows(kind: str, K: int, seed: int) -> np.ndarray:
    """The 16 fp16 rows of LA_ROWS for a kind.
      ties / ties_small   E4M3: 448 * 2^k first (k = 0, -5), then every midpoint of two adjacent e4m3 values times 2^k
                          at both signs. MX: per block of scale 2^e (e cycling) the byte-selecting power of two, the
                          e2m1 ties (resp. e4m3 midpoints of the block's range) and values above saturation (mxfp4:
                          5, 7, 7.5; mxfp8: 449 .. 511 with the tie 464), both signs
      ladder_lo / _hi     32-blocks whose amax climbs from 2^-24 to 2^15, every other block zero (E4M3: the same rows;
                          the row amax decides)
      below_floor         every |x| < 448 * 2^-14, the E4M3 scale floor
      inf / nan           one +Inf, one NaN, in block 3 only"""
    rng = np.random.default_rng(seed)
    mx = kind != "e4m3"
    rows = {}
    rows["zero"] = np.zeros(K)
    rows["neg_zero"] = -np.zeros(K)
    rows["subnormal"] = rng.integers(-1023, 1024, K) * 2.0 ** -24
    r = rng.standard_normal(K) * 2e4
    r[K // 2 + 5] = 65504.0
    rows["amax_65504"] = np.clip(r, -65504, 65504)
    rows["below_floor"] = rng.uniform(-1, 1, K) * 0.027
    for name, k in (("ties", 0), ("ties_small", -5)):
        v = rng.standard_normal(K)
        if kind == "e4m3":
            t = np.concatenate([[448.0], E4M3_TIES, -E4M3_TIES]) * 2.0 ** k
            v = v * 2.0 ** k
            v[:len(t)] = t
        else:
            top, pool = (256.0, np.concatenate([E4M3_TIES[E4M3_TIES > 8], [449, 463, 464, 465, 480, 496, 511]])) \
                if kind == "mxfp8" else (4.0, np.array(E2M1_TIES + (5.0, 7.0, 7.5, 0.125, 0.375)))
            for b in range(K // 32):
                e = k - (b % 7)
                blk = pool[rng.integers(0, len(pool), 32)] * rng.choice([-1.0, 1.0], 32)
                if b < 8 and kind == "mxfp4":  # every tie and the values above saturation, both signs, once in order
                    blk[1:1 + 2 * len(pool)] = np.concatenate([pool, -pool])
                blk[0] = top
                v[32 * b:32 * b + 32] = blk * 2.0 ** e
        rows[name] = v
    exps = np.rint(np.linspace(-24, 15, 2 * (K // 64))).astype(int)
    for name, ex in (("ladder_lo", exps[:K // 64]), ("ladder_hi", exps[K // 64:])):
        v = np.zeros(K)
        for i, e in enumerate(ex):
            m = rng.integers(8, 16, 32) / 8.0 * rng.choice([-1.0, 1.0], 32) * rng.integers(0, 2, 32)
            m[i % 32] = 1.0 + (i % 3) / 4.0
            v[64 * i:64 * i + 32] = np.minimum(m * 2.0 ** e, 65504)
        rows[name] = v
    for name, bad in (("inf", np.inf), ("nan", np.nan)):
        v = rng.standard_normal(K)
        v[3 * 32 + 7] = bad
        rows[name] = v
    for name, k in (("exact", 0), ("exact_small", -6)):
        lo, hi = (k, k) if kind == "e4m3" else (127 + k - 3, 127 + k)
        rows[name] = exact_rows(kind, rng, 1, K, (0, 15) if kind != "mxfp4" else None, lo, hi)[0][0].astype(np.float64)
    rows["randn"] = rng.standard_normal(K)
    rows["randn_small"] = rng.standard_normal(K) * 1e-3
    rows["randn_large"] = rng.standard_normal(K) * 1e3
    with np.errstate(over="ignore"):
        return np.stack([rows[n] for n in LA_ROWS]).astype(np.float16)


def _onehot(kind: str, rng, K: int, pi: np.ndarray) -> Weight:
    """Weight row n one-hot at column pi[n]. E4M3: code 0x38, scale 1. MX: nibble 1.0 in a block of byte 127, the
    row's other bytes random in 1..254 (their codes are zero)."""
    n = np.arange(K)
    if kind == "e4m3":
        c = np.zeros((K, K), np.uint8)
        c[n, pi] = ONE8
        return Weight("e4m3", c, np.ones(K, np.float16))
    c = np.zeros((K, K), np.uint8)
    c[n, pi] = ONE4
    sc = rng.integers(1, 255, (K, K // 32)).astype(np.uint8)
    sc[n, pi // 32] = 127
    return Weight("mxfp4", c, sc)


@functools.lru_cache(maxsize=None)
def la_problem(kind: str, K: int) -> DownProblem:
    """L-a: H = N = Ns = K; 16 rows (LA_ROWS) on routed expert 1 and, in another order, on the shared expert; weight
    row n is one-hot at pi[n], so y[p, n] = fp16(dequant(quant(act[p]))[pi[n]]) (E4M3: times fp16(scale_a))."""
    rng = np.random.default_rng(1000 + K + KINDS.index(kind))
    rows = la_rows(kind, K, 1100 + K + KINDS.index(kind))
    ws = [_onehot(kind, rng, K, rng.permutation(K)) for _ in range(3)]
    order = rng.permutation(16)
    return DownProblem(f"L-a {kind} K={K}", [kind] * 3, ws, _ids_all(16, 1, 1), rows, rows[order], K,
                       dict(one_product=True, rows=rows, order=order))


# ---- L-c: the E4M3 scale ladder
# scale_b of the weight rows; with scale_a = 2^k, k in LC_KS, the product scale_a * scale_b is ordinary (1 * 0.0123),
# a rounding tie on fp16's subnormal grid (2^-1 * (1 + 2^-10) 2^-14 and 2^-1 * (1 + 3 * 2^-10) 2^-14: half a step above
# an even and an odd neighbour), subnormal (2^-10 * 2^-10), zero by underflow (2^-14 * 2^-14, 2^-10 * 2^-24) and
# large (2^7 * 200 = 25600: any |acc| >= 3 overflows the output)
LC_SB = np.array([1.0, 0.0123, (1 + 2.0 ** -10) * 2.0 ** -14, (1 + 3 * 2.0 ** -10) * 2.0 ** -14, 2.0 ** -10, 2.0 ** -14,
                  2.0 ** -24, 200.0, 1.5]).astype(np.float16)
LC_KS = (0, -1, -10, -14, 7)
W_LADDER_A, W_LADDER_B = (5, 8), (5, 8)  # tests/_fp8_bf16_edges.W_LADDER


@functools.lru_cache(maxsize=None)
def lc_problem(T: int) -> DownProblem:
    """L-c: E = 4, topk = 2, H = 128, N = 384, Ns = 640; A rows with scales 2^k, k cycling through LC_KS; weight row n
    of expert e carries LC_SB[(n + e) % 9]. A rows p % 5 == 1 hold 448 * 2^k and one more code (a small sum)."""
    rng = np.random.default_rng(1200 + T)
    E, topk, H, N, Ns = 4, 2, 128, 384, 640
    ws = [weight_e4m3(rng, H, K, W_LADDER_B, LC_SB[(np.arange(H) + e) % len(LC_SB)], fixed=(5, 0))  # (exact_span)
          for e, K in enumerate([N] * E + [Ns])]
    def rows(R, K, off):
        ks = np.array(LC_KS)[(np.arange(R) + off) % len(LC_KS)]
        x, _ = rows_e4m3(rng, R, K, W_LADDER_A, ks, top=5)
        for p in range(R):
            if p % 5 == 1:
                keep = x[p, [5, 40, 41]].copy()
                x[p] = 0
                x[p, [5, 40, 41]] = keep
        return x
    return DownProblem(f"L-c T={T}", ["e4m3"] * (E + 1), ws, _routing(rng, T, E, topk), rows(T * topk, N, 0), rows(T, Ns, 2), H)


# ---- L-d: the MX scale range
@functools.lru_cache(maxsize=None)
def ld_problem(kind: str, T: int) -> DownProblem:
    """L-d: test_mx_down_scale_ladder's scheme. Weight row n of expert e has the byte 99 + (n + 5 e) % 57 in every block
    (99 .. 155), A row p the byte 115 + p % 17 (mxfp8: 115 + p % 13) in every block: sa + sb - 254 spans [-40, 17 + ...]
    (mxfp8 codes reach 448 = 2^8.8, mxfp4 codes 6), both ends of fp16."""
    rng = np.random.default_rng(1300 + T + KINDS.index(kind))
    E, topk, H, N, Ns = 4, 2, 128, 384, 640
    ws = []
    for e, K in enumerate([N] * E + [Ns]):
        w = weight_mx(rng, H, K, 127, 127, fixed=(3, 0) if kind == "mxfp8" else None)
        w.scales[:] = (99 + (np.arange(H) + 5 * e) % 57).astype(np.uint8)[:, None]
        ws.append(w)
    def rows(R, K):
        b = np.repeat((115 + np.arange(R) % (13 if kind == "mxfp8" else 17)).astype(np.uint8)[:, None], K // 32, 1)
        return rows_mx(kind, rng, R, K, (6, 9), b, top=3)[0]
    return DownProblem(f"L-d {kind} T={T}", [kind] * (E + 1), ws, _routing(rng, T, E, topk), rows(T * topk, N), rows(T, Ns), H)


# ---- L-e: geometry
def decode_ct(E: int, T: int, topk: int, C: int, C_shared: int = 0) -> int:
    """geometry() of mxmoe_amd/csrc/moe_decode.h restated, the lines from "columns of the experts that can have rows" to
    "a.ct = ct" (npairs = T * topk; cols = min(E, npairs) * C + (with_shared ? C_shared : 0); ct = 128;
    while (ct > 32 && cols / ct < 1024) ct >>= 1): cols = min(E, T * topk) * C + C_shared (the columns of the
    experts that can have rows); ct starts at 128 and is halved while ct > 32 and cols / ct < 1024."""
    cols = min(E, T * topk) * C + C_shared
    ct = 128
    while ct > 32 and cols // ct < 1024:
        ct >>= 1
    return ct


def lp_rb(kinds, K: int, T: int = 16) -> int:
    """lp_lds() of moe_decode.h restated: the rows of a batch for the widest A row of the call's lp kinds."""
    row = max(K // 2 if k == "mxfp4" else K for k in kinds) + 16
    srow = ((K // 32 + 15) // 16) * 16 + 4
    return min(max((60 * 1024 - 32) // (row + srow), 1), 16, T)


# A windows per kind for dense sums: (code window, scale lo, hi). The K = 4096 family narrows the scales
# (tests/_fp8_bf16_edges.W_SPLITK's spans) so that the bound holds at that width.
A_WIN = {"e4m3": ((6, 7), -3, 0), "mxfp8": ((7, 7), 124, 127), "mxfp4": (None, 124, 127), "w8a8": (None, 0, 0),
         "fp16": (None, 0, 0)}
A_WIN_4096 = {"e4m3": ((6, 7), -3, 0), "mxfp8": ((7, 7), 126, 127), "mxfp4": (None, 126, 127)}


def dense_weight(kind: str, rng, rows: int, K: int, narrow: bool = False, sb_exp=(-4, -1), anchor: bool = False,
                 zero_col=None, col_code: int = 0, win=(6, 8)) -> Weight:
    """A dense weight for exact sums: E4M3 codes of window (6, 8) with power-of-two row scales 2^sb_exp[0] ..
    2^sb_exp[1]; MX random nibbles with bytes 123 .. 126 (narrow: 125, 126). zero_col: the column (E4M3) or in-block
    position (MX) that meets the scale-selecting element of exact fp8 A rows holds code 0, which keeps that element's
    product (448 or 256 code units) out of the sums (exact_span); col_code: a small code there instead (the K = 4096
    family, whose narrow scales leave room for it). w8a8: integers with 127 in column 1 and scales 2^-7, 2^-6 (scale
    products stay normal fp16 numbers); fp16:
    multiples of 1 / 64 in [-1 / 8, 1 / 8]."""
    if kind == "w8a8":
        c = rng.integers(-127, 128, (rows, K))
        c[:, 1] = 127
        return Weight("w8a8", c, np.exp2(rng.integers(-7, -5, rows).astype(np.float64)).astype(np.float16))
    if kind == "fp16":
        return Weight("fp16", (rng.integers(-8, 9, (rows, K)) / 64.0).astype(np.float16), None)
    if kind == "e4m3":
        return weight_e4m3(rng, rows, K, win, np.exp2(rng.integers(sb_exp[0], sb_exp[1] + 1, rows).astype(np.float64)),
                           fixed=None if zero_col is None else (zero_col, col_code))
    return weight_mx(rng, rows, K, 125 if narrow else 123, 126, anchor=anchor,
                     fixed=None if zero_col is None else (zero_col % 32, col_code))


@functools.lru_cache(maxsize=None)
def le_cut_problem(kind: str) -> DownProblem:
    """L-e (ii): K = N = Ns = 4096, H = 128, E = 4, topk = 4, T = 16, every id 2: 64 rows on one expert, and 16 on the
    shared one, in batches of lp_rb() rows (E4M3 and MXFP8: 14, so 14 + 2 rows for the shared expert and 14 * 4 + 8 for
    the routed one)."""
    rng = np.random.default_rng(1400 + KINDS.index(kind))
    E, topk, T, H, K = 4, 4, 16, 128, 4096
    win, lo, hi = A_WIN_4096[kind]
    # the column that meets the rows' scale-selecting element (448, resp. 256 code units) holds a small nonzero code
    # (E4M3 0x20 = 2^-3, e2m1 0.5), so that element's product is part of every sum, inside exact_span
    ws = [dense_weight(weight_kind(kind), rng, H, K, narrow=True, sb_exp=(-8, -6), zero_col=None if kind == "mxfp4" else 77,
                       col_code=0x20 if kind == "e4m3" else 1) for _ in range(E + 1)]
    act = exact_rows(kind, rng, T * topk, K, win, lo, hi, top=77)[0]
    act_s = exact_rows(kind, rng, T, K, win, lo, hi, top=77)[0]
    return DownProblem(f"L-e cut {kind}", [kind] * (E + 1), ws, _ids_all(T, topk, 2), act, act_s, H, dict(rb=lp_rb([kind], K)))


WIDE_KINDS = KINDS + ("w8a8", "fp16")  # lp_tile and expert_tile in one launch
LE_WIDE_C = {64: 1024, 128: 2048}  # the smallest of the candidates 512 / 1024 / 2048 / 4096 that reaches each ct


@functools.lru_cache(maxsize=None)
def le_wide_down_problem(ct: int) -> DownProblem:
    """L-e (i), down: E = 64, T = 16, topk = 4 with every token's ids distinct, K = N = 128, C = H = LE_WIDE_C[ct], no
    shared expert's width in the column count but one present (Ns = 128); expert e of kind WIDE_KINDS[e % 5]."""
    rng = np.random.default_rng(1500 + ct)
    E, topk, T, K, H = 64, 4, 16, 128, LE_WIDE_C[ct]
    kinds = [WIDE_KINDS[e % 5] for e in range(E)] + ["mxfp8"]
    ws = [dense_weight(weight_kind(k), rng, H, K, zero_col=9 if k in ("e4m3", "mxfp8") else None) for k in kinds]
    ids = _routing(rng, T, E, topk)
    act = np.zeros((T * topk, K), np.float16)
    for p, e in enumerate(ids.reshape(-1)):
        win, lo, hi = A_WIN[kinds[e]]
        act[p] = exact_rows(kinds[e], rng, 1, K, win, lo, hi, top=9)[0][0]
    win, lo, hi = A_WIN["mxfp8"]
    act_s = exact_rows("mxfp8", rng, T, K, win, lo, hi, top=9)[0]
    return DownProblem(f"L-e wide ct={ct}", kinds, ws, ids, act, act_s, H, dict(ct=ct))


# ------------------------------------------------------------------ L-b: both entries, a whole layer
LB_SHAPES = {"a": (128, 1152, 512), "b": (1152, 512, 128), "c": (640, 1024, 640), "d": (1024, 640, 1024),
             "e": (512, 128, 1152)}  # (H, N, Ns): every width of 128 / 512 / 640 / 1024 / 1152 as H and as N once
# "cross": the three cross-kind pairs of tests/test_decode_lp_gpu.MIXED cycling over the five experts; "mixed": that
# whole list, one pair per expert, the shared expert last
LB_PAIRS = {"e4m3": [("e4m3", "e4m3")], "mxfp8": [("mxfp8", "mxfp8")], "mxfp4": [("mxfp4", "mxfp4")],
            "cross": [("e4m3", "mxfp8"), ("mxfp8", "mxfp4"), ("mxfp4", "e4m3")],
            "mixed": [("e4m3", "mxfp8"), ("mxfp8", "mxfp4"), ("mxfp4", "e4m3"), ("w8a8", "w4a16"), ("w4a16", "w8a8")]}
LB_CASES = [(name, shape, T) for name in LB_PAIRS for shape, T in (("a", 1), ("b", 16), ("c", 5), ("d", 16), ("e", 5))]


@dataclasses.dataclass
class LayerCase:
    """A layer of E routed experts and a shared one on exact data: pairs[e] = (gate_up kind, down kind), w1[e]
    [2 N_e, H] in [gate; up] order, w2[e] [H, N_e]; hidden [T, H] fp16 (or bf16-exact values); ids [T, topk]."""

    name: str
    pairs: list
    w1: list
    w2: list
    hidden: np.ndarray
    ids: np.ndarray
    H: int
    N: int
    Ns: int
    info: dict = dataclasses.field(default_factory=dict)

    @property
    def E(self) -> int:
        return len(self.pairs) - 1

    def gu_ref(self, e: int, rows: np.ndarray) -> np.ndarray:
        """fp16 [R, 2 N_e]: the gate_up linear of expert e on hidden rows, [gate | up]"""
        return ref_linear(self.pairs[e][0], rows, self.w1[e])

    def y_ref(self, e: int, act: np.ndarray) -> np.ndarray:
        return ref_linear(self.pairs[e][1], act, self.w2[e])

    @functools.cached_property
    def bound1(self) -> float:
        flat = self.ids.reshape(-1)
        topk = self.ids.shape[1]
        b = [exact_bound(self.pairs[e][0], self.hidden[np.unique(np.nonzero(flat == e)[0] // topk)], self.w1[e])
             for e in range(self.E) if (flat == e).any()]
        return max(b + [exact_bound(self.pairs[-1][0], self.hidden, self.w1[-1])])

    def bound2(self, act: np.ndarray, act_shared: np.ndarray) -> float:
        """the down stage's bound on given act rows (pair order) — the CPU restatement's or the device's own"""
        flat = self.ids.reshape(-1)
        b = [exact_bound(self.pairs[e][1], act[flat == e], self.w2[e]) for e in self.exact_down(flat)]
        return max(b + ([exact_bound(self.pairs[-1][1], act_shared, self.w2[-1])] if self.pairs[-1][1] in KINDS else [0.0]))

    @functools.cached_property
    def span1(self) -> float:
        return max(exact_span(p[0], self.hidden, w) for p, w in zip(self.pairs, self.w1))

    def span2(self, act: np.ndarray, act_shared: np.ndarray) -> float:
        flat = self.ids.reshape(-1)
        b = [exact_span(self.pairs[e][1], act[flat == e], self.w2[e]) for e in self.exact_down(flat)]
        return max(b + ([exact_span(self.pairs[-1][1], act_shared, self.w2[-1])] if self.pairs[-1][1] in KINDS else [0.0]))

    def exact_down(self, flat) -> list:
        """the routed experts with rows whose down linear is one of the three kinds: the sums held exact on the device's
        own act (a w8a8 down is integer arithmetic; a w4a16 down sums fp16 act values of 11 significant bits in f32)"""
        return [e for e in range(self.E) if (flat == e).any() and self.pairs[e][1] in KINDS]

    def limit(self, stage: int) -> float:
        return min(BOUND[p[stage]] for p in self.pairs if stage == 0 or p[1] in KINDS)


def _gate_up_weight(kind: str, rng, N: int, H: int, sign_k: np.ndarray, top: int, up_sign: np.ndarray, anchor: bool,
                    fp8_a: bool, win=(6, 8)) -> Weight:
    """[gate; up] rows whose element signs follow the A rows' column signs: every product of a gate row is positive
    and every product of up row n has the sign up_sign[n], so g and |u| are sums without cancellation — a narrow
    range of magnitudes, which the gated activation keeps (see layer_case). The column(s) that meet the A rows'
    scale-selecting element hold magnitude 1 (MXFP4 rows) or 0 (fp8 rows: exact_span)."""
    rsign = np.concatenate([np.ones(N), up_sign])[:, None] * sign_k[None, :]
    if kind == "w8a8":  # magnitudes 1 .. 15 and one 127 (the row's scale is then its power of two)
        c = rng.integers(1, 16, (2 * N, H))
        c[:, top] = 127
        return Weight("w8a8", (c * rsign).astype(np.int64), np.ones(2 * N, np.float16))
    if kind == "w4a16":  # magnitudes 0 .. 7, with -8 at one negative and 7 at one positive position of every row
        c = rng.integers(0, 8, (2 * N, H)) * rsign
        for r in range(2 * N):
            c[r, np.nonzero(rsign[r] < 0)[0][0]] = -8
            c[r, np.nonzero(rsign[r] > 0)[0][0]] = 7
        return Weight("w4a16", c.astype(np.float16), None)
    if kind == "e4m3":
        return weight_e4m3(rng, 2 * N, H, win, 1.0, sign=rsign, fixed=(top, 0))
    return weight_mx(rng, 2 * N, H, 123, 126, sign=rsign, fixed=(top % 32, 0 if fp8_a else ONE4), anchor=anchor)


def _rescale(w: Weight, acc_max: float, target: float) -> None:
    """Scales a weight by the power of two that brings acc_max to target or less (E4M3: the row scales; MX: the bytes)."""
    k = int(np.ceil(np.log2(acc_max / target)))
    if w.kind == "w4a16":
        w.codes = (w.codes.astype(np.float64) * 2.0 ** -k).astype(np.float16)
    elif w.mx:
        w.scales[:] = (w.scales.astype(np.int64) - k).astype(np.uint8)
    else:
        w.scales[:] = (w.scales.astype(np.float64) * 2.0 ** -k).astype(np.float16)


@functools.lru_cache(maxsize=None)
def layer_case(name: str, shape: str, T: int, clamp: bool = False, anchor: bool = False) -> LayerCase:
    """L-b: E = 4, topk = 2 and the shared expert (Ns != N) at LB_SHAPES[shape], the kinds LB_PAIRS[name].

    hidden: exact rows (exact_rows) of A_WIN's windows — E4M3 row scales 2^-3 .. 2^0, MX per-block bytes 124 .. 127 —
    with one column sign pattern for all tokens. The gate_up weights follow it (_gate_up_weight), so g > 0 and u has
    its row's sign with |g|, |u| within a small factor of each other over a row; their scales bring max g and max |u|
    to 2^7 or less (clamp: 7 or less, the limit, and up rows positive, so the clamp acts on a few values only and
    u + 1 >= 1). act = g sigmoid(g) u then spans few binades per row (and per 32-block), which keeps the granule of
    its E4M3 / MXFP8 / MXFP4 codes, and with it the down stage's bound, where the kernel's f32 sums are exact. The
    down weights are dense with random signs (dense_weight): y has cancellation."""
    H, N, Ns = LB_SHAPES[shape]
    pairs = [LB_PAIRS[name][e % len(LB_PAIRS[name])] for e in range(5)]
    rng = np.random.default_rng(1600 + 7 * list(LB_SHAPES).index(shape) + 100 * list(LB_PAIRS).index(name) + T + 50 * clamp)
    E, topk = 4, 2
    sign_k = rng.choice([-1.0, 1.0], H)
    top = int(rng.integers(0, 31))  # (in-block position 31 is the anchor's)
    # one hidden row feeds experts of several gate_up kinds in the cross and mixed layers: its rows are the MXFP4 kind's
    # exact rows (multiples of 2^-4 up to 6), which MXFP8 quantises exactly too, fp16 weights take as they are, E4M3
    # rounds to codes whose 448 then meets window (7, 7) weight codes (exact_span), and w8a8 to integers
    many = name in ("cross", "mixed")
    hid_kind = "mxfp4" if many else pairs[0][0]
    win, lo, hi = A_WIN[hid_kind]
    if clamp and hid_kind == "e4m3":
        lo = hi
    hidden, hcodes, hscales = exact_rows(hid_kind, rng, T, H, win, lo, hi, top=top, sign=sign_k)
    ids = _routing(rng, T, E, topk)
    w1, w2 = [], []
    target = 6.5 if clamp else 2.0 ** 7
    for e, (k1, k2) in enumerate(pairs):
        n = Ns if e == E else N
        up_sign = np.ones(n) if clamp else rng.choice([-1.0, 1.0], n)
        w = _gate_up_weight(weight_kind(k1), rng, n, H, sign_k, top, up_sign, anchor, hid_kind != "mxfp4",
                            win=(7, 7) if many else (6, 8))
        a, sa = a_values(k1, hidden)
        acc = np.abs(a @ w.values().T).max(axis=1) * (1.0 if sa is None else sa.astype(np.float64))
        _rescale(w, float(acc.max()), target)
        w1.append(w)
        # (MX down weights: bytes of two values — act's own block maxima reach 448 code units, and exact_span must hold)
        if k2 == "w4a16":  # integers in [-8, 7] times 2^-12, both ends in every row
            c = rng.integers(-8, 8, (H, n))
            c[:, 0], c[:, 1] = -8, 7
            w2.append(Weight("w4a16", (c * 2.0 ** -12).astype(np.float16), None))
            continue
        w2.append(dense_weight(weight_kind(k2), rng, H, n, narrow=True, sb_exp=(-14, -12), anchor=anchor))
        if w2[-1].mx:
            w2[-1].scales -= 10
        elif k2 == "w8a8":
            w2[-1].scales = (w2[-1].scales.astype(np.float64) * 2.0 ** -8).astype(np.float16)
    return LayerCase(f"L-b {name} {shape} T={T}" + (" clamp" if clamp else ""), pairs, w1, w2, hidden, ids, H, N, Ns,
                     dict(hid_kind=hid_kind, hcodes=hcodes, hscales=hscales, clamp=clamp))


# ------------------------------------------------------------------ L-f: dense sums, the down entry alone
@functools.lru_cache(maxsize=None)
def dense_down_problem(kind: str) -> DownProblem:
    """L-f: what L-b's down stage cannot carry (its A rows are the device's own act, which forces narrow weight scales
    and gate_up signs without cancellation): dense exact sums on raw records with random signs on both sides, MX weight
    bytes drawn per block from four values (123 .. 126) and A scales per row / block from four (A_WIN). E = 4, topk = 2,
    T = 16, H = 128, N = 1152 (S = 9: the second K trip of fp4 weights, a third scale group), Ns = 640."""
    rng = np.random.default_rng(1900 + KINDS.index(kind))
    E, topk, T, H, N, Ns = 4, 2, 16, 128, 1152, 640
    win, lo, hi = A_WIN[kind]
    top = 45
    ws = [dense_weight(weight_kind(kind), rng, H, K, zero_col=None if kind == "mxfp4" else top) for K in [N] * E + [Ns]]
    act = exact_rows(kind, rng, T * topk, N, win, lo, hi, top=top)[0]
    act_s = exact_rows(kind, rng, T, Ns, win, lo, hi, top=top)[0]
    return DownProblem(f"L-f {kind}", [kind] * (E + 1), ws, _routing(rng, T, E, topk), act, act_s, H)


# ------------------------------------------------------------------ L-e (i), gate_up: a layer of 64 experts
@functools.lru_cache(maxsize=None)
def wide_layer_case(ct: int) -> LayerCase:
    """L-e (i), gate_up: E = 64 experts of kinds WIDE_KINDS[e % 5] and a shared MXFP4 one, H = 128, N = Ns =
    LE_WIDE_C[ct], T = 16, topk = 4 with distinct ids. One hidden row feeds experts of every kind, so the rows are the
    MXFP4 kind's exact rows (multiples of 2^-4 up to 6): MXFP4 and MXFP8 quantise them exactly, E4M3 to rounded codes
    (its weights are window (7, 7) codes, which keeps exact_span), fp16 takes them as they are, and w8a8 is integer
    arithmetic whatever the codes. Only the gate_up stage is built to be exact."""
    rng = np.random.default_rng(1800 + ct)
    E, T, topk, H, N = 64, 16, 4, 128, LE_WIDE_C[ct]
    kinds = [WIDE_KINDS[e % 5] for e in range(E)] + ["mxfp4"]

    def wt(k, rows, K):
        if k in OTHER_KINDS:
            return dense_weight(k, rng, rows, K)
        w = dense_weight(weight_kind(k), rng, rows, K, sb_exp=(-9, -8), win=(7, 7))
        if w.mx:
            w.scales -= 8
        return w

    w1, w2 = [wt(k, 2 * N, H) for k in kinds], [wt(k, H, N) for k in kinds]
    hidden, hc, hs = exact_rows("mxfp4", rng, T, H, None, 124, 127)
    return LayerCase(f"L-e wide gate_up ct={ct}", [(k, k) for k in kinds], w1, w2, hidden, _routing(rng, T, E, topk), H, N, N,
                     dict(hid_kind="mxfp4", hcodes=hc, hscales=hs, clamp=False, ct=ct))
