"""Shared helpers for tests: seeded problem construction + oracle expectations."""
from __future__ import annotations

import dataclasses

import numpy as np
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd.groupgemm import BF16, FP16, W4A4, W4A4_G128, W8A8, W8A8_E4M3, Problem, QParams
from mxmoe_amd.quantize import pack_e4m3, pack_wxax, quant_e4m3, quant_rtn_sym
from oracle import oracle, weightonly

QCFGS = {"fp16": FP16, "w8a8_g-1_sym": W8A8, "w4a4_g-1_sym": W4A4, "w4a4_g128_sym": W4A4_G128,
         "w8a8_g-1_sym_E4M3": W8A8_E4M3, "bf16": BF16}


FULL_SIZE_CFGS = ("fp16", "w8a8", "w4a4", "mixed", "ds2_mixed")  # BASELINE configs[1]-[4] at bs=8192


def full_size_variants() -> list:
    """Variants the full-size (bs=8192) parity tests run: EVERY production variant, so the kernel
    AUTO hands a benched config to (the kernel of record) is always among them
    (tests/test_abi.py::test_full_size_parity_covers_auto_choices guards this)."""
    return list(nat.production_variants())


def full_size_layer(cfg: str) -> dict:
    """{"gate_up": [QShape], "down": [QShape]} of one BASELINE full-size config."""
    from mxmoe_amd.workload import (ds2_mixed_qconfig, ds2_workload, load_workload, mixed_qconfig_lp1,
                                    qwen2_layer11_workload)

    if cfg == "ds2_mixed":
        return load_workload(ds2_workload(8192, qconfig=ds2_mixed_qconfig()))["layer-1"]
    kw = {"fp16": {}, "w8a8": dict(qstr="w8a8_g-1_sym"), "w4a4": dict(qstr="w4a4_g-1_sym"),
          "mixed": dict(qconfig=mixed_qconfig_lp1())}[cfg]
    return load_workload(qwen2_layer11_workload(8192, **kw))["layer-11"]


def exact_compare(q: QParams) -> bool:
    """Integer-accumulating quant types are checked bit for bit; fp16 / bf16 / weight-only / E4M3
    (f32 sums in an unspecified order) within the fp16 tolerance."""
    return q.is_quant and not q.is_weight_only and not q.is_fp8


class HostProblem:
    """Host copies of one problem's inputs (numpy) + the device Problem."""

    def __init__(self, M, N, K, q: QParams, seed: int, device: str, ldc: int = 0, C: torch.Tensor | None = None,
                 c_col0: int = 0, ref_format: bool = False):
        g = torch.Generator().manual_seed(seed)
        self.M, self.N, self.K, self.q = M, N, K, q
        a = (torch.rand(M, K, generator=g, dtype=torch.float32) * 2 - 1).to(torch.float16)
        b = (torch.rand(N, K, generator=g, dtype=torch.float32) * 2 - 1).to(torch.float16)
        if q.is_fp8:
            qa, sa = quant_e4m3(a)
            qb, sb = quant_e4m3(b)
            self.qa, self.qb = qa.numpy(), qb.numpy()
            self.A, self.B = pack_e4m3(qa).numpy(), pack_e4m3(qb).numpy()
            self.sa, self.sb = sa.numpy(), sb.numpy()
        elif q.fmt == "bf16":
            self.A = a.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            self.B = b.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
            self.sa = self.sb = None
        elif q.is_weight_only:
            # oracle quantisation; B either packed straight into the kernel layout or built in the
            # reference's packed format and converted by the library (the drop-in route)
            qv, sz = weightonly.quant_wo(b.numpy(), q.w_bits, q.gsize, q.sym)
            self.sb = weightonly.permute_scale(sz, N, K, q.gsize, q.sym)
            self.qb = qv
            if ref_format:
                self.B = nat.repack_weightonly(weightonly.ref_pack(qv, q.w_bits, q.sym), N, K, q.w_bits)
            else:
                self.B = weightonly.mi355x_pack(qv, q.w_bits, q.sym)
            self.A = a.numpy()
            self.sa = None
        elif q.is_quant:
            bits = q.a_bits
            qa, sa = quant_rtn_sym(a, bits, q.gsize)
            qb, sb = quant_rtn_sym(b, bits, q.gsize)
            self.qa, self.qb = qa.numpy(), qb.numpy()
            self.A = pack_wxax(qa, bits).numpy()
            self.B = pack_wxax(qb, bits).numpy()
            self.sa, self.sb = sa.numpy(), sb.numpy()
        else:
            self.A, self.B = a.numpy(), b.numpy()
            self.sa = self.sb = None
        self._bind(device, ldc, C, c_col0)

    @classmethod
    def from_raw(cls, raw: "Raw", device: str | None, ldc: int = 0) -> "HostProblem":
        """A problem from given operands (tests/_util.py generators below) instead of quantised random
        data: packed A / B bytes (or fp16 arrays) and scale arrays exactly as the kernels read them.
        ``expected()`` goes through the same oracle calls. device None: host side only (no Problem)."""
        hp = cls.__new__(cls)
        hp.M, hp.N, hp.K, hp.q = raw.M, raw.N, raw.K, raw.q
        hp.A, hp.B, hp.sa, hp.sb, hp.qb = raw.A, raw.B, raw.sa, raw.sb, raw.qb
        hp.raw = raw
        if device is None:
            hp.problem = None
        else:
            hp._bind(device, ldc, None, 0)
        return hp

    def _bind(self, device, ldc, C, c_col0):
        M, N, K, q = self.M, self.N, self.K, self.q
        self.ldc = ldc or N
        dev = torch.device(device)
        if C is None:
            self.Cbuf = torch.full((max(M, 1), self.ldc), float("nan"), dtype=torch.float16, device=dev)
            Cview = self.Cbuf
        else:
            self.Cbuf = C
            Cview = C[:, c_col0:]
        self.c_col0 = c_col0
        if q.fmt == "bf16":
            tA = torch.from_numpy(self.A.view(np.int16)).view(torch.bfloat16).to(dev)
            tB = torch.from_numpy(self.B.view(np.int16)).view(torch.bfloat16).to(dev)
        else:
            tA, tB = torch.from_numpy(self.A).to(dev), torch.from_numpy(self.B).to(dev)
        self.problem = Problem(
            A=tA, B=tB, C=Cview, M=M, N=N, K=K, q=q,
            scale_a=None if self.sa is None else torch.from_numpy(self.sa).to(dev),
            scale_b=None if self.sb is None else torch.from_numpy(self.sb).to(dev),
            ldc=self.ldc if C is None else C.shape[1])

    def expected(self) -> np.ndarray:
        if self.q.is_fp8:
            return oracle.gg_e4m3(self.A, self.B, self.sa, self.sb, self.M, self.N, self.K)
        if self.q.fmt == "bf16":
            return oracle.gg_bf16(self.A, self.B, self.M, self.N, self.K)
        if self.q.is_weight_only:
            q = self.q
            return weightonly.gemm(self.A, weightonly.dequant(self.qb, self.sb, self.N, self.K, q.w_bits, q.gsize, q.sym))
        if self.q.is_quant and self.q.gsize != -1:
            return oracle.gg_quant_grouped(self.A, self.B, self.sa, self.sb, self.M, self.N, self.K, self.q.a_bits,
                                           self.q.gsize)
        if self.q.is_quant:
            return oracle.gg_quant(self.A, self.B, self.sa, self.sb, self.M, self.N, self.K, self.q.a_bits)
        return oracle.gg_f16(self.A, self.B, self.M, self.N, self.K)

    def result(self) -> np.ndarray:
        c = self.problem.C
        return c[: self.M, : self.N].cpu().numpy()


def assert_f16_close(out: np.ndarray, ref: np.ndarray, K: int):
    """fp16 GroupGEMM tolerance: relative 1e-3 (north_star) plus an absolute floor for cancellation,
    |out-ref| <= 1e-3*|ref| + 1e-3*rms(ref) + 2^-10 * (K * 2^-24 * |a||b| bound ~ 0)."""
    out = out.astype(np.float64)
    ref = ref.astype(np.float64)
    assert np.isfinite(out).all(), "non-finite output"
    rms = float(np.sqrt(np.mean(ref * ref))) if ref.size else 0.0
    tol = 1e-3 * np.abs(ref) + 1e-3 * rms + 1e-6
    bad = np.abs(out - ref) > tol
    assert not bad.any(), f"{bad.sum()} / {bad.size} fp16 outputs outside tolerance; max err " \
                          f"{np.max(np.abs(out - ref))}"


def assert_fakequant_close(out: np.ndarray, ref_fq: np.ndarray, what: str = ""):
    """Parity against the reference's executed definition of a quantised linear,
    C_fq = F.linear(Quantizer.fake_quant(a), Quantizer.fake_quant(b)) in fp32 (quant.py:87-106).

    The two computations are equal in exact arithmetic; they round differently: fake_quant rounds
    every dequantised operand q*s (+zp) to fp16 (relative 2^-11 each) and sums in fp32, the kernel
    path forms the exact integer dot product, rounds sa*sb to fp16 and the output to fp16. Bar:
      norm-wise  ||out - C_fq|| <= 1e-3 ||C_fq||            (north_star's 1e-3 relative)
      elementwise |out - C_fq| <= 1e-3 |C_fq| + 4e-3 rms(C_fq)   (cancellation floor)
    Measured on the fixtures: norm-wise 2-5e-4, elementwise excess <= 1.9e-3 rms."""
    out = out.astype(np.float64)
    ref = ref_fq.astype(np.float64)
    assert out.shape == ref.shape, (out.shape, ref.shape)
    if ref.size == 0:
        return
    assert np.isfinite(out).all(), f"{what}: non-finite output"
    nref = float(np.linalg.norm(ref))
    assert float(np.linalg.norm(out - ref)) <= 1e-3 * nref, f"{what}: norm-wise error above 1e-3"
    rms = nref / np.sqrt(ref.size)
    bad = np.abs(out - ref) > 1e-3 * np.abs(ref) + 4e-3 * rms
    assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} outputs outside the fake-quant tolerance"


def codes_f64(packed: torch.Tensor, rows: int, bits: int, K: int) -> torch.Tensor:
    """pack_wxax rows -> their integer codes as f64 [rows, K]. The codes come out in the packed byte /
    nibble order (pack_wxax puts element 0 of each 16-bit word in its high bits, oracle/gg_oracle.c
    unpack_row), the same permutation of K for A and B, which leaves every dot product unchanged."""
    b = packed.contiguous().view(torch.int8).view(rows, -1)[:, :K * bits // 8]
    if bits == 8:
        return b.double()
    lo = torch.bitwise_right_shift(torch.bitwise_left_shift(b, 4), 4)  # sign-extended low nibble
    hi = torch.bitwise_right_shift(b, 4)                               # (arithmetic shift)
    return torch.stack((lo, hi), dim=-1).view(rows, -1).double()


def quant_epilogue_ref(acc, sa, sb):
    """oracle_gg_quant's epilogue on a whole f64 accumulator matrix (torch, any device):
    fp16_rn(0 + f32(acc) * f32(fp16_rn(sa[m] * sb[n]))) — the fp16 product of two fp16 scales is
    exact in f32 and rounded once, f32(acc) and the f32 product round to nearest, +0 turns -0 into +0."""
    s16 = sa.view(-1, 1).half() * sb.view(1, -1).half()
    return (acc.float() * s16.float() + 0.0).half()


# =================================================================================================
# Value-edge operands (tests/test_value_edges.py on the CPU, tests/test_value_edges_gpu.py on the
# GPU): problems built from chosen codes and scales instead of quantised uniform data. Every
# generator is pure numpy and seeded; both files call the same ones, so what the CPU file proves
# about an input family (which value classes occur, which wrong arithmetic it exposes) holds for
# what the GPU file runs.
# =================================================================================================

@dataclasses.dataclass
class Raw:
    """Operands of one problem as the kernels read them: packed A / B bytes (or fp16 arrays), scale
    arrays in the kernel layout; weight-only problems also keep their logical codes (``qb``)."""

    M: int
    N: int
    K: int
    q: QParams
    A: np.ndarray
    B: np.ndarray
    sa: np.ndarray | None = None
    sb: np.ndarray | None = None
    qb: np.ndarray | None = None
    info: dict = dataclasses.field(default_factory=dict)


def p2(e: int) -> np.float16:
    """2^e as fp16 (exact for -24 <= e <= 15; e < -14 is subnormal)."""
    return np.float16(2.0 ** e)


def raw_codes(raw: Raw) -> tuple[np.ndarray, np.ndarray]:
    """Logical integer codes (int64 [M, K], [N, K]) of an integer problem's packed operands."""
    bits = raw.q.a_bits
    return (oracle.unpack_wxax(raw.A, bits, raw.K).astype(np.int64),
            oracle.unpack_wxax(raw.B, bits, raw.K).astype(np.int64))


def raw_acc(raw: Raw) -> np.ndarray:
    """Exact integer accumulators: [M, N], or [G, M, N] per 128-group for w4a4 g128."""
    qa, qb = raw_codes(raw)
    if raw.q.gsize == -1:
        return oracle.acc_exact(qa, qb)
    G = raw.K // raw.q.gsize
    return np.stack([oracle.acc_exact(qa[:, g * raw.q.gsize:(g + 1) * raw.q.gsize],
                                      qb[:, g * raw.q.gsize:(g + 1) * raw.q.gsize]) for g in range(G)])


def raw_scale_product(raw: Raw) -> tuple[np.ndarray, np.ndarray]:
    """(exact f64 product sa*sb, its fp16 rounding), [M, N] or [G, M, N]."""
    if raw.q.gsize == -1:
        ex = raw.sa.astype(np.float64)[:, None] * raw.sb.astype(np.float64)[None, :]
    else:
        G = raw.K // raw.q.gsize
        ex = raw.sa.reshape(G, raw.M).astype(np.float64)[:, :, None] * \
            raw.sb.reshape(G, raw.N).astype(np.float64)[:, None, :]
    return ex, ex.astype(np.float16)  # (f64 -> fp16 is one correct rounding of the exact product)


def _ordinary_scales(rng, n: int) -> np.ndarray:
    return (rng.uniform(0.5, 1.5, n) * 2.0 ** -7).astype(np.float16)


def gen_full_range(M: int, N: int, K: int, q: QParams, seed: int) -> Raw:
    """(a) A and B bytes uniform over 0..255: every int8 code including -128, every nibble including
    -8; the first byte of row 0 is the extreme code on both sides (the product (-128)^2 / (-8)^2
    occurs), and the last 256 bytes of B (of A when it has room) hold every byte value once. Ordinary
    scales in [2^-8, 1.5 * 2^-7]: |out| <= 16384 K * 1.5^2 * 2^-14 stays finite."""
    rng = np.random.default_rng(seed)
    bits = q.a_bits
    kb = K * bits // 8
    A = rng.integers(0, 256, (M, kb), dtype=np.uint8)
    B = rng.integers(0, 256, (N, kb), dtype=np.uint8)
    B.reshape(-1)[-256:] = np.arange(256, dtype=np.uint8)
    if A.size >= 512:
        A.reshape(-1)[-256:] = np.arange(256, dtype=np.uint8)
    A[0, 0] = B[0, 0] = 0x80 if bits == 8 else 0x88
    G = 1 if q.gsize == -1 else K // q.gsize
    return Raw(M, N, K, q, A, B, _ordinary_scales(rng, G * M), _ordinary_scales(rng, G * N))


def gen_large_acc(M: int, N: int, K: int, seed: int) -> Raw:
    """(b) w8a8 rows of +127 / -128 runs with matching signs in B: |acc| reaches 16384 K (> 2^24 from
    K = 1025). A rows by m % 4: all -128 | all +127 | -128 with 8 random codes | +127 then -127 halves
    (cancels to exactly 0 against a constant B row); B rows by n % 4: all -128 | all +127 | -128 with
    8 random codes | runs of 64 alternating +127 / -128.

    The pair (M-1, N-1) is built so that acc = X 2^14 + 2^13 + 1 with X = 1100 (even): f32(acc) drops
    the low bit by a tie to even, X 2^14 + 2^13, which times the scale product 2^-12 is an fp16 tie
    and rounds to the even 4 X, while the exact acc lies above the tie and rounds to 4 (X + 1). A row:
    -128 with code 1 first; B row: code 1 first, then -v_k with sum v_k = (acc - 1) / 128."""
    assert K >= 1152 and K % 2 == 0
    rng = np.random.default_rng(seed)
    qa = np.empty((M, K), np.int64)
    qb = np.empty((N, K), np.int64)
    for m in range(M):
        t = m % 4
        qa[m] = -128 if t in (0, 2) else 127
        if t == 2:
            qa[m, rng.choice(K, 8, replace=False)] = rng.integers(-128, 128, 8)
        if t == 3:
            qa[m, K // 2:] = -127
    for n in range(N):
        t = n % 4
        qb[n] = -128 if t in (0, 2) else 127
        if t == 2:
            qb[n, rng.choice(K, 8, replace=False)] = rng.integers(-128, 128, 8)
        if t == 3:
            qb[n] = np.where((np.arange(K) // 64) % 2 == 0, 127, -128)
    X = 1100
    target = X * 2 ** 14 + 2 ** 13 + 1
    S = (target - 1) // 128
    v = np.full(K - 1, S // (K - 1), np.int64)
    v[:S % (K - 1)] += 1
    assert v.max() <= 128 and v.sum() == S
    qa[M - 1] = -128
    qa[M - 1, 0] = 1
    qb[N - 1, 0] = 1
    qb[N - 1, 1:] = -v
    sa, sb = _ordinary_scales(rng, M), _ordinary_scales(rng, N)
    sa[M - 1] = sb[N - 1] = p2(-6)
    return Raw(M, N, K, W8A8, oracle.pack_wxax(qa.astype(np.int8), 8), oracle.pack_wxax(qb.astype(np.int8), 8), sa, sb,
               info=dict(tie=(M - 1, N - 1), target=target, X=X))


# sa[m] = LADDER_A[m % 6], sb[n] = LADDER_B[n % 7] (coprime lengths: every pair occurs). Products:
# ordinary (1 * 0.0123), a rounding tie ((1 + 2^-10) * 1.5 = 1.5 + 1.5 * 2^-10), subnormal (2^-14 *
# 2^-10 = 2^-24), a subnormal tie (1.5 * 2^-10 * 2^-14), zero by underflow (2^-14 * 2^-14, 2^-24 *
# 2^-24), and 240 * 200 = 48000: finite, but any |acc| >= 2 overflows the output to +-inf.
LADDER_A = np.array([1.0, 1 + 2.0 ** -10, 2.0 ** -14, 2.0 ** -24, 1.5 * 2.0 ** -10, 240.0]).astype(np.float16)
LADDER_B = np.array([1.0, 1.5, 2.0 ** -10, 2.0 ** -14, 2.0 ** -24, 200.0, 0.0123]).astype(np.float16)


def _ladder_codes(rng, rows: int, K: int, bits: int, lo: int | None = None) -> np.ndarray:
    """A-side codes: full range, rows m % 5 == 0 all zero, m % 5 == 1 a single code 1 (|acc| <= 128:
    with a subnormal scale product the output is subnormal)."""
    hi = 1 << (bits - 1)
    qa = rng.integers(-hi if lo is None else lo, hi, (rows, K))
    for m in range(rows):
        if m % 5 == 0:
            qa[m] = 0
        elif m % 5 == 1:
            qa[m] = 0
            qa[m, (7 * m) % K] = 1
    return qa


def gen_scale_ladder(M: int, N: int, K: int, q: QParams, seed: int) -> Raw:
    """(c) per-row / per-column scales from LADDER_A / LADDER_B, full-range codes, zero and one-code
    A rows."""
    assert q.gsize == -1 and M >= 30 and N >= 7
    rng = np.random.default_rng(seed)
    bits = q.a_bits
    hi = 1 << (bits - 1)
    qa = _ladder_codes(rng, M, K, bits)
    qb = rng.integers(-hi, hi, (N, K))
    return Raw(M, N, K, q, oracle.pack_wxax(qa.astype(np.int8), bits), oracle.pack_wxax(qb.astype(np.int8), bits),
               LADDER_A[np.arange(M) % 6].copy(), LADDER_B[np.arange(N) % 7].copy())


G128_KINDS = ("steps", "dominant", "cancel")


def gen_g128_ladder(M: int, N: int, K: int, kind: str, seed: int) -> Raw:
    """(c) w4a4 g128 with group scales that differ by powers of two along K; sa[g][m] = mant_a[m] 2^ea[g],
    sb[g][n] = mant_b[n] 2^eb[g] with fp16 mantissas in [1, 2).
      steps ..... exponents step up and down by 2 along K on both sides (products 2^-8 or more apart); rows m % 6 == 5 /
                  columns n % 7 == 6 carry 2^-12 (product 2^-24: subnormal), m % 6 == 4 / n % 7 == 5
                  carry 2^-14 (every product with them underflows to 0 or is subnormal)
      dominant .. one group 2^24 above the others (scale products up to 2^14: most outputs overflow)
      cancel .... groups 0 and 1 huge, with A's codes negated in group 1 and B's repeated, so that
                  acc_1 = -acc_0 and the two folds cancel exactly; the rest 2^-14: the small groups
                  survive only if they are added after the cancellation (group order)."""
    assert K % 128 == 0 and K >= 512 and M >= 30 and N >= 7
    rng = np.random.default_rng(seed)
    G = K // 128
    qa = _ladder_codes(rng, M, K, 4, lo=-7 if kind == "cancel" else None)
    qb = rng.integers(-8, 8, (N, K))
    ma = np.frombuffer(rng.integers(0x3C00, 0x4000, M).astype(np.uint16).tobytes(), np.float16).astype(np.float64)
    mb = np.frombuffer(rng.integers(0x3C00, 0x4000, N).astype(np.uint16).tobytes(), np.float16).astype(np.float64)
    g = np.arange(G)
    if kind == "steps":
        ea = np.maximum(-2 * np.abs(g - G // 2), -6)  # K = 512: -4 -2 0 -2; K = 1408: -6 -6 -6 -4 -2 0 -2 ...
        eb = ea - 2
    elif kind == "dominant":
        ea = np.where(g == G // 2, 6, -6)
        eb = ea.copy()
    else:
        ea = np.where(g < 2, 5, -7)
        eb = ea.copy()
        qa[:, 128:256] = -qa[:, 0:128]
        qb[:, 128:256] = qb[:, 0:128]
    sa = (ma[None, :] * 2.0 ** ea[:, None]).astype(np.float16)
    sb = (mb[None, :] * 2.0 ** eb[:, None]).astype(np.float16)
    if kind == "steps":
        sa[:, np.arange(M) % 6 == 5] = p2(-12)
        sb[:, np.arange(N) % 7 == 6] = p2(-12)
        sa[:, np.arange(M) % 6 == 4] = p2(-14)
        sb[:, np.arange(N) % 7 == 5] = p2(-14)
    return Raw(M, N, K, W4A4_G128, oracle.pack_wxax(qa.astype(np.int8), 4), oracle.pack_wxax(qb.astype(np.int8), 4),
               np.ascontiguousarray(sa).reshape(-1), np.ascontiguousarray(sb).reshape(-1), info=dict(kind=kind))


def permuted_identity(K: int, rng) -> tuple[np.ndarray, np.ndarray]:
    """fp16 A [K, K] with row m holding 1.0 at column pi[m]: C[m, n] = B[n, pi[m]] exactly."""
    pi = rng.permutation(K)
    A = np.zeros((K, K), np.float16)
    A[np.arange(K), pi] = 1.0
    return A, pi


def wo_scale_zp_sets(bits: int) -> tuple[np.ndarray, np.ndarray]:
    """The crafted (scale, zero point) values of the dequant readout. Largest |value|: 255 * 64 + 1000."""
    s = np.array([37 * 2.0 ** -24, 2.0 ** -14, 0.0123, 64.0, 0.5 / ((1 << bits) - 1)]).astype(np.float16)
    z = np.array([0.0, 1000.0, -3.5, 5 * 2.0 ** -24, 100.0]).astype(np.float16)
    return s, z


def gen_dequant_readout(K: int, N: int, q: QParams, seed: int) -> Raw:
    """(d) weight-only problem whose A is a permuted identity (M = K), so C reads the dequantised
    weights back: C[m, n] = dequant[n, pi[m]]. Stored codes uniform over 0 .. 2^bits - 1 (every code in
    the first columns of row 0); per (column, group) a scale from {subnormal, 2^-14, ordinary, 64,
    0.5 / (2^bits - 1)} and, asym, a zero point from {+0, 1000, -3.5, subnormal, 100} in every
    combination (the last scale with zp 100 is what weights in [100, 100.5] quantise to)."""
    rng = np.random.default_rng(seed)
    bits, sym = q.w_bits, q.sym
    G = 1 if q.gsize == -1 else K // q.gsize
    u = rng.integers(0, 1 << bits, (N, K))
    u[0, :1 << bits] = np.arange(1 << bits)
    qv = (u - weightonly.sym_offset(bits, sym)).astype(np.int32)
    S, Z = wo_scale_zp_sets(bits)
    i = np.arange(N * G)
    scale = S[i % 5]
    if sym:
        sz = scale
    else:
        sz = np.stack([scale, Z[(i // 5) % 5]], axis=1)
    A, pi = permuted_identity(K, rng)
    return Raw(K, N, K, q, A, weightonly.mi355x_pack(qv, bits, sym), None,
               weightonly.permute_scale(sz, N, K, q.gsize, sym), qv, info=dict(pi=pi))


def gen_f16_readout(K: int, N: int, seed: int, subnormal: bool = False) -> Raw:
    """(d) the same readout for fp16: B holds normal finite fp16 bit patterns of every exponent (1..30),
    both signs, and +-65504. subnormal: the even columns of B hold subnormal patterns instead
    (info['sub'] marks them in C's coordinates)."""
    rng = np.random.default_rng(seed)
    e = rng.integers(1, 31, (N, K))
    e[0, 1:61:2] = np.arange(1, 31)  # (odd columns: they stay normal in the subnormal case)
    bits = (rng.integers(0, 2, (N, K)) << 15) | (e << 10) | rng.integers(0, 1024, (N, K))
    bits[1, 1], bits[1, 3] = 0x7BFF, 0xFBFF
    sub = np.zeros((N, K), bool)
    if subnormal:
        sub[:, 0::2] = True
        sb_ = (rng.integers(0, 2, (N, K)) << 15) | rng.integers(1, 1024, (N, K))
        sb_[2, 0], sb_[2, 2] = 0x0001, 0x83FF
        bits = np.where(sub, sb_, bits)
    B = bits.astype(np.uint16).view(np.float16)
    A, pi = permuted_identity(K, rng)
    return Raw(K, N, K, FP16, A, np.ascontiguousarray(B), info=dict(pi=pi, sub=np.ascontiguousarray(sub[:, pi].T)))


# ------------------------------------------------------------------ (e) activation kernels
ACT_IDS = np.array([[0, 1], [2, 3], [0, 2], [1, 3], [0, 3]], np.int32)  # T = 5, topk = 2, E = 4: all non-empty
ACT_TAGS = (0, 1, 2, 3)  # expert e quantises with tag e (fp16, int8, int4, int4 g128)
ACT_KINDS = ("zero", "one_nonzero", "tiny", "subscale", "amax_max", "tie", "clamp", "rand", "zero_group", "neg_zero")
ACT_WIDTHS = (512, 1024, 1536, 2048, 3072, 4096, 6144, 8192, 16384, 640, 2688, 5248)
ACT_MAXC = (1, 2, 3, 4, 6, 8, 12, 16, 32)  # act_quant_kernel<MODE, MAXC> instantiations (moe_ops.hip)


def act_launch_plan(ntk: int, nshared: int, w_routed: int, w_shared: int) -> list[tuple[str, int]]:
    """moe_ops.hip launch_act / launch_act_w restated: the launches of one call as (branch, MAXC),
    branch "split_row" (one launch, each shared row over a workgroup's four waves), "two_launch"
    (routed rows, then shared rows) or "one_launch"."""
    def maxc(w):
        return next((c for c in ACT_MAXC if (w + 511) // 512 <= c), ACT_MAXC[-1])

    if ntk + nshared == 0:
        return []
    qw = (w_shared // 4 + 127) & ~127
    if nshared > 0 and ntk > 0 and w_shared > w_routed and qw <= w_routed:
        return [("split_row", maxc(w_routed))]
    if nshared > 0 and ntk > 0 and w_routed != w_shared:
        return [("two_launch", maxc(w_routed)), ("two_launch", maxc(w_shared))]
    return [("one_launch", maxc(max(w_routed, w_shared) if nshared > 0 else w_routed))]


def act_qmax(tag: int) -> int:
    return 127 if tag in (0, 1) else 7


def clamp_amax(qmax: int) -> np.float16:
    """The first fp16 a in [1, 2) whose scale s = fp16(a / qmax) rounds down far enough that
    fp16(a / s) > qmax: the quantiser's clamp acts on the row's own maximum."""
    a = np.arange(0x3C00, 0x4000, dtype=np.uint16).view(np.float16)
    s = (a.astype(np.float32) / np.float32(qmax)).astype(np.float16)
    d = (a.astype(np.float32) / s.astype(np.float32)).astype(np.float16)
    return a[np.nonzero(d > np.float16(qmax))[0][0]]


_ACT_ROWS: dict = {}


def act_special_rows(W: int, tag: int) -> np.ndarray:
    """fp16 [len(ACT_KINDS), W]: one row per kind, built for tag's qmax (127, or 7 for the int4 tags).
    The element that sets the scale sits at the start of every 128-group, so a g128 row has the same
    class in each group.
      zero ......... all +0: scale exactly 1, codes 0
      one_nonzero .. 0.37 in the last column only (g128: zero groups before one live group)
      tiny ......... amax = 2^-24: amax / qmax underflows to 0 in fp16, the scale becomes 1
      subscale ..... amax = 3 qmax 2^-24: the scale is the subnormal 3 * 2^-24
      amax_max ..... amax = 65504 at both signs
      tie .......... scale 2^-3 exactly (amax = qmax / 8), x = (k + 0.5) / 8 for every k in
                     [-qmax, qmax): x / s is a tie for even and odd k; holds -0 and +0
      clamp ........ amax = clamp_amax(qmax): fp16(amax / scale) > qmax
      rand ......... uniform in (-3, 3)
      zero_group ... rand with columns 128..255 zero (g128: a zero group between live ones)
      neg_zero ..... rand with every 7th element -0"""
    if (W, tag) in _ACT_ROWS:
        return _ACT_ROWS[(W, tag)]
    rng = np.random.default_rng(1000 * tag + W)
    qmax = act_qmax(tag)
    g0 = np.arange(0, W, 128)
    rows = {}
    rows["zero"] = np.zeros(W)
    x = np.zeros(W)
    x[W - 1] = 0.37
    rows["one_nonzero"] = x
    x = np.zeros(W)
    x[g0], x[g0 + 1] = 2.0 ** -24, -2.0 ** -24
    rows["tiny"] = x
    x = rng.integers(-3 * qmax, 3 * qmax + 1, W).astype(np.float64)
    x[g0] = 3 * qmax
    rows["subscale"] = x * 2.0 ** -24
    x = rng.uniform(-1, 1, W) * 65504
    x[g0], x[g0 + 1] = 65504, -65504
    rows["amax_max"] = x
    x = (np.arange(W) % (2 * qmax) - qmax + 0.5) / 8
    x[g0], x[g0 + 5], x[g0 + 6] = qmax / 8, -0.0, 0.0
    rows["tie"] = x
    a = float(clamp_amax(qmax))
    x = rng.uniform(-1, 1, W) * a
    x[g0], x[g0 + 1] = a, -a
    rows["clamp"] = x
    rows["rand"] = rng.uniform(-3, 3, W)
    x = rng.uniform(-3, 3, W)
    x[128:256] = 0
    rows["zero_group"] = x
    x = rng.uniform(-3, 3, W)
    x[::7] = -0.0
    rows["neg_zero"] = x
    out = np.stack([rows[k] for k in ACT_KINDS]).astype(np.float16)
    out.setflags(write=False)
    _ACT_ROWS[(W, tag)] = out
    return out


def act_slot_call(W: int, Ws: int, shared_tag: int, c: int) -> tuple[np.ndarray, np.ndarray]:
    """Call c of the slot-order modes (quant_slots): (routed [10, W] in slot order, shared [5, Ws]).
    Slot s of expert e holds kind (s + c) % 10 of the rows built for tag e, shared row t kind
    (t + c) % 10 of shared_tag's: over c = 0..9 every expert meets every kind."""
    from oracle import moe_ref

    sorted_e = moe_ref.route(ACT_IDS, 4)[0]
    R = len(ACT_KINDS)
    routed = np.stack([act_special_rows(W, ACT_TAGS[e])[(s + c) % R] for s, e in enumerate(sorted_e)])
    shared = np.stack([act_special_rows(Ws, shared_tag)[(t + c) % R] for t in range(ACT_IDS.shape[0])])
    return routed, shared


def act_hidden_call(K: int, c: int, parity: int) -> tuple[np.ndarray, np.ndarray]:
    """Call (c, parity) of quant_act: (hidden [5, K], ids [5, 2]). A hidden row is gathered by both of
    its token's experts, so tokens go to experts (0, 1) (fp16, int8: rows built for qmax 127) or
    (2, 3) (int4, int4 g128: qmax 7), alternating with the token and the parity; token t holds kind
    (t + c) % 10. Over c = 0..9 and both parities every expert meets every kind."""
    T, R = ACT_IDS.shape[0], len(ACT_KINDS)
    low = [(t + parity) % 2 == 0 for t in range(T)]
    ids = np.array([[0, 1] if lo else [2, 3] for lo in low], np.int32)
    hidden = np.stack([act_special_rows(K, 1 if lo else 2)[(t + c) % R] for t, lo in enumerate(low)])
    return hidden, ids


def act_segments(routed_slots: np.ndarray, shared: np.ndarray | None, ids: np.ndarray, E: int = 4) -> list:
    """Rows per segment (expert 0..E-1, then the shared expert) from slot-order routed rows."""
    from oracle import moe_ref

    counts = moe_ref.route(ids, E)[3]
    starts = np.concatenate([[0], np.cumsum(counts)])
    segs = [routed_slots[starts[e]:starts[e + 1]] for e in range(E)]
    return segs + ([shared] if shared is not None else [])


SILU_G = (-30.0, -17.0, -10.0, -1e-3, 0.0, 10.0, 20.0)


def gen_silu_inputs(rows: int, N: int, seed: int) -> np.ndarray:
    """fp16 [rows, 2N] = [gate | up]: gate uniform in (-4, 4) with every 4th column from SILU_G in turn,
    up uniform in (-4, 4): |silu(g) u| <= 80. Three of four columns are ordinary, so every row and
    every 128-group has amax of order 1: a 1-ulp difference in an activation moves the scale by at most
    1 ulp (no group sits at the scale's 0 -> 1 switch, where it would jump)."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-4, 4, (rows, N))
    g[:, ::4] = np.array(SILU_G)[(np.arange(0, N, 4) // 4 + np.arange(rows)[:, None]) % len(SILU_G)]
    u = rng.uniform(-4, 4, (rows, N))
    return np.concatenate([g, u], axis=1).astype(np.float16)


def interleave_gate_up_cols(gu: np.ndarray) -> np.ndarray:
    """[gate | up] columns -> alternating 16-column blocks gate b, up b (mxmoe_moe_silu_mul_quant_il)."""
    R, N2 = gu.shape
    N = N2 // 2
    return np.ascontiguousarray(np.stack([gu[:, :N].reshape(R, N // 16, 16), gu[:, N:].reshape(R, N // 16, 16)],
                                         axis=2).reshape(R, N2))


def split_row_peaks(Ws: int) -> list[int]:
    """Columns of the shared rows' maxima in a split-row launch: one in each non-empty quarter run
    (width (Ws / 4 rounded up to 128)), then one in the last 128 columns."""
    qw = (Ws // 4 + 127) & ~127
    cols = [min(p * qw + 3, Ws - 130 + p) for p in range(4) if p * qw < Ws]
    return cols + [Ws - 5]


def gen_split_rows(Ws: int, seed: int, silu: bool = False) -> np.ndarray:
    """Shared rows for the split-row branch, one per split_row_peaks column: |x| < 1 except the peak
    (50). silu: [gate | up] rows whose activation has that shape (g = 10, u = 5 at the peak:
    silu(10) * 5 = 49.998; elsewhere |g|, |u| < 1, |act| < 0.74)."""
    rng = np.random.default_rng(seed)
    peaks = split_row_peaks(Ws)
    if not silu:
        x = rng.uniform(-1, 1, (len(peaks), Ws))
        x[np.arange(len(peaks)), peaks] = 50.0
        return x.astype(np.float16)
    g, u = rng.uniform(-1, 1, (len(peaks), Ws)), rng.uniform(-1, 1, (len(peaks), Ws))
    g[np.arange(len(peaks)), peaks], u[np.arange(len(peaks)), peaks] = 10.0, 5.0
    return np.concatenate([g, u], axis=1).astype(np.float16)


def gen_combine(T: int, topk: int, H: int, seed: int) -> dict:
    """(f) combine inputs: ids (topk of E = 8 distinct experts per token), y fp16 [T topk, H] in (-1, 1),
    weights k / 8 with |k| <= 8 (4 mantissa bits: every fma operand sum is exact in f64, which
    moe_ref.combine asserts), a zero and a negative weight; shared rows and shared weights likewise."""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation(8)[:topk] for _ in range(T)]).astype(np.int32)
    w = (rng.integers(-8, 9, (T, topk)) / 8).astype(np.float32)
    w[0, 0], w[T - 1, topk - 1] = 0.0, -0.75
    return dict(ids=ids, y=rng.uniform(-1, 1, (T * topk, H)).astype(np.float16), w=w,
                shared=rng.uniform(-1, 1, (T, H)).astype(np.float16),
                shared_w=np.array([0.5, -1.25, 0.0] * T, np.float32)[:T])


# ------------------------------------------------------------------ the problem lists both files run
def _kq(q: QParams, k8: int) -> int:
    """K with the byte length of an 8-bit problem of K = k8 (so K tails fall alike for 4-bit codes)."""
    return k8 * 8 // q.a_bits


def full_range_problems(q: QParams) -> list[Raw]:
    """(a): M = 1 / several blocks / N tails, and 3 stages + 48 bytes (a K tail inside a 128-byte
    stage); g128 at K = 512 and 1408 (1408: 5.5 stages, the last stage holds one group)."""
    if q.gsize == 128:
        shapes = [(1, 128, 512), (130, 264, 1408), (300, 136, 512), (70, 136, 1408)]
    else:
        shapes = [(1, 128, 256), (130, 264, 512), (300, 136, 1152), (70, 136, _kq(q, 432))]
    return [gen_full_range(M, N, K, q, seed=700 + i) for i, (M, N, K) in enumerate(shapes)]


def large_acc_problems(splitk: bool) -> list[Raw]:
    """(b): |acc| up to 16384 K > 2^24; splitk: the two smaller shapes of
    tests/test_gg_gpu.py::test_splitk_long_k_low_fill (a low-fill long-K call the planner splits)."""
    shapes = [(40, 2048, 1408), (3, 256, 1408)] if splitk else [(130, 264, 1152), (33, 136, 1408)]
    return [gen_large_acc(M, N, K, seed=720 + i) for i, (M, N, K) in enumerate(shapes)]


def ladder_problems(q: QParams) -> list[Raw]:
    """(c): the scale ladder over one tile with tails and over several blocks; g128: every kind at
    K = 512 and one at K = 1408."""
    if q.gsize == 128:
        return [gen_g128_ladder(37, 136, 512, kind, seed=740 + i) for i, kind in enumerate(G128_KINDS)] + \
               [gen_g128_ladder(130, 264, 1408, kind, seed=750 + i) for i, kind in enumerate(G128_KINDS)]
    return [gen_scale_ladder(M, N, _kq(q, K), q, seed=730 + i) for i, (M, N, K) in enumerate([(37, 136, 256), (130, 264, 512)])]


WO_READOUT_QS = [QParams(16, b, g, s) for b in (2, 4, 8) for g in (-1, 64, 128) for s in (True, False)]


def dequant_readout_problems(q: QParams) -> list[Raw]:
    """(d): K = M = 256, N = 264; grouped types also K = M = 1408, N = 136."""
    shapes = [(256, 264)] + ([(1408, 136)] if q.gsize != -1 else [])
    return [gen_dequant_readout(K, N, q, seed=760 + i) for i, (K, N) in enumerate(shapes)]


ACT_BRANCH_WIDTHS = {"split_row": (1408, 5632), "two_launch_wide_quarter": (128, 1024), "two_launch_narrow_shared": (1024, 256)}
COMBINE_H = (8, 264, 2056, 4104)
COMBINE_TOPK = (1, 8)


def f16_ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in fp16 steps along the real line (sign-aware: -0 and +0 are 0 apart)."""
    def key(x):
        u = np.ascontiguousarray(x, np.float16).view(np.uint16).astype(np.int32)
        return np.where(u & 0x8000, -(u & 0x7FFF), u)

    return np.abs(key(a) - key(b))
