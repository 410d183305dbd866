"""GPU tests of the weight-only MXFP4 tile (w4a16_g32_sym_MXFP4: fp16 A on the MXFP4 B operand,
gg_tile_wo's MXFP4 body) on the small-batch kernel wo3, on v2x and through AUTO.

"Exact" cases: every b[n][k] = e2m1 * 2^(scale - 127) with scale codes in [104, 140] is an fp16 value,
and the A data are chosen so that every partial sum, in any order, is exact in f32 (T1: integers in
[-3, 3] times 2^-8 .. 2^1, |sum| < 2^12 on a 2^-8 grid; T2 / T4: one product per output; T3: multiples
of 2^-3 below 2^15), so the result must equal fp16_rn of the f64 reference bit for bit. Random cases
compare against the f64 reference under assert_f16_close.

Every C buffer carries one guard row behind row M and, where ldc > N, guard columns: they must keep
their fill value.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import (FP16, W4A4, W4A4_MXFP4, W4A16_G128_ASYM, W4A16_MXFP4, W8A8, W8A16_ASYM, GroupGemm,
                                 Problem)
from oracle import moe_ref
from tests import _mxfp4_ref as ref
from tests._util import HostProblem, assert_f16_close, exact_compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -1234.0
MXW_BIT, MX_BIT, SILU_BIT = 1 << 11, 1 << 10, 1 << 16  # plan-info qtype_mask bits
WO3, V2X = "wo3_64x256_w8_3wg", "v2x_256x256_w8_b3_buf_spread_edma"


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _names():
    return [ln.split()[1] for ln in nat.list_variants()]


VARIANTS = pytest.mark.parametrize("variant", ["wo3", "v2x", "auto"])


def _variant(name):
    return None if name == "auto" else _names().index(WO3 if name == "wo3" else V2X)


class A16Problem:
    """fp16 A and canonical MXFP4 B operands (numpy) + the device Problem with a guarded C."""

    def __init__(self, a, bc, bsc, ldc: int = 0):
        self.a, self.bc, self.bsc = np.ascontiguousarray(a, np.float16), bc, bsc
        self.M, self.N, self.K = a.shape[0], bc.shape[0], a.shape[1]
        self.ldc = ldc or self.N
        self._ref = None
        self.bind()

    def bind(self):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.Cbuf = torch.full((self.M + 1, self.ldc), GUARD, dtype=torch.float16, device=DEV)
        self.problem = Problem(A=t(self.a), B=t(self.bc), C=self.Cbuf, M=self.M, N=self.N, K=self.K, q=W4A16_MXFP4,
                               scale_b=qz.pack_mxfp4_scales(t(self.bsc)), ldc=self.ldc)

    @property
    def expected(self) -> np.ndarray:  # f64, computed once
        if self._ref is None:
            self._ref = self.a.astype(np.float64) @ ref.dequant(self.bc, self.bsc).T
        return self._ref

    def result(self) -> np.ndarray:
        c = self.Cbuf.cpu().numpy()
        assert (c[self.M] == np.float16(GUARD)).all(), "guard row behind C was written"
        assert (c[: self.M, self.N:] == np.float16(GUARD)).all(), "guard columns behind N were written"
        return c[: self.M, : self.N]

    def check_exact(self, what=""):
        want = self.expected.astype(np.float16)
        out = self.result()
        bad = out.view(np.uint16) != want.view(np.uint16)
        assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}"

    def check_close(self):
        assert_f16_close(self.result(), self.expected, self.K)


def _rand(M, N, K, seed, b_scale=1.0) -> A16Problem:
    g = torch.Generator().manual_seed(seed)
    a = (torch.rand(M, K, generator=g) * 2 - 1).half()
    bc, bsc = qz.quant_mxfp4((torch.randn(N, K, generator=g) * b_scale).half())
    return A16Problem(a.numpy(), bc.numpy(), bsc.numpy())


def _run(problems, variant, want_variant=None):
    gg = GroupGemm([p.problem for p in problems], variant=_variant(variant))
    if want_variant is not None:
        assert _names()[gg.variant] == want_variant
    gg.launch()
    torch.cuda.synchronize()
    return gg


@VARIANTS
@pytest.mark.parametrize("K", [448, 64])
def test_t1_scale_map_exact(variant, K):
    """Every B element is 1.0 and A is constant over each 32-K block, so C[m][n] =
    32 sum_b a[m][b] 2^(sb[n][b] - 127): only the pairing of the scale bytes with the K blocks decides
    the result (K = 448: 7 stages, 14 blocks, a partial 16-byte scale group)."""
    M, N = 33, 40
    rng = np.random.default_rng(11 + K)
    ab = rng.integers(-3, 4, (M, K // 32)).astype(np.float64)
    bsc = rng.integers(119, 129, (N, K // 32)).astype(np.uint8)
    p = A16Problem(np.repeat(ab, 32, axis=1), np.full((N, K // 2), 0x22, np.uint8), bsc)  # nibble 2 = 1.0
    want = 32.0 * (ab @ np.exp2(bsc.astype(np.float64) - 127).T)
    assert np.array_equal(p.expected, want)
    _run([p], variant)
    p.check_exact("scale map")


@VARIANTS
def test_t2_element_map_exact(variant):
    """A is one-hot, A[m][perm(m)] = 1 (M = K = 128: two 64-row tiles), so C[m][n] = b[n][perm(m)] reads
    out every B element: nibble order, lane map and K order are pinned."""
    M = K = 128
    N = 48
    rng = np.random.default_rng(12)
    perm = rng.permutation(K)
    a = np.zeros((M, K), np.float16)
    a[np.arange(M), perm] = 1.0
    nib = rng.integers(0, 16, (N, K)).astype(np.uint8)
    bsc = rng.integers(124, 131, (N, K // 32)).astype(np.uint8)
    p = A16Problem(a, ref.pack_nibbles(nib), bsc)
    assert np.array_equal(p.expected, ref.dequant(p.bc, bsc)[:, perm].T)
    _run([p], variant)
    p.check_exact("element map")


@VARIANTS
def test_t3_exact_arithmetic(variant):
    """A holds multiples of 0.5 in [-4, 4], B random codes with scale codes 126..128: every product is a
    multiple of 2^-3 of magnitude <= 48 and K <= 512, so any-order f32 sums are exact."""
    rng = np.random.default_rng(13)
    ps = []
    for M, N, K in [(70, 136, 512), (33, 40, 192), (130, 264, 64)]:
        a = rng.integers(-8, 9, (M, K)) * 0.5
        nib = rng.integers(0, 16, (N, K)).astype(np.uint8)
        ps.append(A16Problem(a, ref.pack_nibbles(nib), rng.integers(126, 129, (N, K // 32)).astype(np.uint8)))
    _run(ps, variant)
    for p in ps:
        p.check_exact("exact sums")


def _t4_problem(bsc_cols: np.ndarray) -> A16Problem:
    M, N, K = 33, len(bsc_cols), 128
    rng = np.random.default_rng(14)
    a = np.zeros((M, K), np.float16)
    a[np.arange(M), (np.arange(M) * 5) % K] = 1.0
    nib = rng.integers(0, 16, (N, K)).astype(np.uint8)
    return A16Problem(a, ref.pack_nibbles(nib), np.repeat(bsc_cols.astype(np.uint8)[:, None], K // 32, 1))


@VARIANTS
def test_t4_scale_range(variant, capsys):
    """One nonzero A element (1.0) per row, one scale code per column sweeping 104..140 — every code of
    the range in which all b values are fp16 values, subnormals (down to 2^-24) included: bit-exact.
    A second run puts codes outside the range (and 255) on ten columns; what those columns return is
    recorded, the only assertion is that every other column is unchanged."""
    inr = 104 + np.arange(40) % 37
    p = _t4_problem(inr)
    want = p.expected.astype(np.float16)
    assert (np.abs(want[want != 0]) < 2.0 ** -14).any() and np.abs(want).max() >= 2.0 ** 12  # both ends are exercised
    _run([p], variant)
    p.check_exact("scale range")
    odd = np.array([0, 1, 50, 100, 103, 141, 142, 200, 254, 255])
    cols = np.arange(10) * 4 + 1
    mixed = inr.copy()
    mixed[cols] = odd
    q = _t4_problem(mixed)
    _run([q], variant)
    got, base = q.result(), p.result()
    keep = np.ones(40, bool)
    keep[cols] = False
    assert np.array_equal(got[:, keep].view(np.uint16), base[:, keep].view(np.uint16))
    nib = ref.nibbles(q.bc)
    with capsys.disabled():
        for c, code in zip(cols, odd):
            k = (np.arange(33) * 5) % 128
            seen = {int(nib[c, kk]): float(got[m, c]) for m, kk in enumerate(k)}
            print(f"\n[{variant}] scale code {code}: e2m1 code -> output {dict(sorted(seen.items()))}", end="")
        print()


T5_SHAPES = [(1, 128, 256), (17, 256, 128), (130, 136, 384), (257, 264, 512), (513, 512, 1408), (0, 256, 256),
             (64, 8, 1024), (35, 512, 64)]
_t5_cache: list = []


def _t5_problems():
    if not _t5_cache:
        _t5_cache.extend(_rand(M, N, K, seed=500 + i) for i, (M, N, K) in enumerate(T5_SHAPES))
    return _t5_cache


@VARIANTS
def test_t5_random_parity(variant):
    ps = _t5_problems()
    for p in ps:
        p.bind()  # fresh guarded C per variant; operands and references are shared
    gg = _run(ps, variant)
    assert gg.info.qtype_mask == MXW_BIT  # the kernel that holds this tile body alone
    for p in ps:
        p.check_close()


@VARIANTS
def test_t6_strided_c_graph_rebind(variant):
    g = torch.Generator().manual_seed(61)
    a = (torch.rand(70, 320, generator=g) * 2 - 1).half().numpy()
    bc, bsc = (t.numpy() for t in qz.quant_mxfp4(torch.randn(136, 320, generator=g).half()))
    p = A16Problem(a, bc, bsc, ldc=136 + 24)  # ldc > N: guard columns
    gg = _run([p], variant, WO3 if variant == "auto" else None)
    p.check_close()
    first = p.result().copy()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        gg.launch(s)
    p.Cbuf[: p.M, : p.N].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(p.result().view(np.uint16), first.view(np.uint16))  # bit-identical across launches
    p2 = A16Problem(a, bc, bsc, ldc=136 + 24)
    gg.rebind([p2.problem])
    gg.launch()
    torch.cuda.synchronize()
    assert np.array_equal(p2.result().view(np.uint16), first.view(np.uint16))


_t6_cache: list = []


@VARIANTS
def test_t6_split_k(variant):
    """A low-fill call (a shared expert's long K beside four small routed problems): the planner cuts
    the long tiles along K at whole 64-K stages, so a slice starts anywhere in an 8-stage scale group."""
    if not _t6_cache:
        _t6_cache.append(_rand(128, 2048, 5632, seed=62, b_scale=0.05))
        _t6_cache.extend(_rand(9, 2048, 1408, seed=63 + i, b_scale=0.05) for i in range(4))
    ps = _t6_cache
    for p in ps:
        p.bind()
    gg = _run(ps, variant, WO3 if variant == "auto" else None)
    assert gg.info.splitk_slabs > 0
    for p in ps:
        p.check_close()
    first = [p.result().copy() for p in ps]
    gg.launch()
    torch.cuda.synchronize()
    for p, f in zip(ps, first):
        assert np.array_equal(p.result().view(np.uint16), f.view(np.uint16))


def _check_host(h: HostProblem):
    out, want = h.result(), h.expected()
    if exact_compare(h.q):
        assert (out.view(np.uint16) == want.view(np.uint16)).all(), h.q.qcfg
    else:
        assert_f16_close(out, want, h.K)


@VARIANTS
def test_t6_mixed_launch(variant):
    """The type beside w4a16 g128 asym, w8a16, w8a8, fp16 and w4a4 problems in one launch (the wide builds)."""
    mx = [_rand(35, 264, 576, seed=71), _rand(130, 136, 128, seed=72)]
    others = [HostProblem(40, 256, 512, W4A16_G128_ASYM, seed=73, device=DEV), HostProblem(33, 128, 256, W8A16_ASYM, seed=74, device=DEV),
              HostProblem(50, 256, 512, W8A8, seed=75, device=DEV), HostProblem(29, 128, 192, FP16, seed=76, device=DEV),
              HostProblem(66, 384, 512, W4A4, seed=77, device=DEV)]
    gg = GroupGemm([mx[0].problem] + [h.problem for h in others] + [mx[1].problem], variant=_variant(variant))
    if variant == "auto":
        assert _names()[gg.variant] == WO3
    assert gg.info.qtype_mask & MXW_BIT and gg.info.qtype_mask & 31 == 31
    gg.launch()
    torch.cuda.synchronize()
    for p in mx:
        p.check_close()
    for h in others:
        _check_host(h)


def test_t6_a4_and_a16_share_b_on_v2x():
    """One launch in which a w4a4 MXFP4 problem and a w4a16 MXFP4 problem take the SAME B and scale_b
    tensors; AUTO keeps v2x for the pair."""
    g = torch.Generator().manual_seed(81)
    M, N, K = 70, 264, 448
    a = torch.randn(M, K, generator=g).half()
    bc, bsc = qz.quant_mxfp4((torch.randn(N, K, generator=g) * 0.5).half())
    ac, asc = qz.quant_mxfp4(a)
    p16 = A16Problem(a.numpy(), bc.numpy(), bsc.numpy())
    c4 = torch.full((M + 1, N), GUARD, dtype=torch.float16, device=DEV)
    p4 = Problem(A=ac.to(DEV), B=p16.problem.B, C=c4, M=M, N=N, K=K, q=W4A4_MXFP4,
                 scale_a=qz.pack_mxfp4_scales(asc.to(DEV)), scale_b=p16.problem.scale_b)
    assert p4.B.data_ptr() == p16.problem.B.data_ptr() and p4.scale_b.data_ptr() == p16.problem.scale_b.data_ptr()
    for variant in (None, _names().index(V2X)):
        p16.Cbuf.fill_(GUARD)
        c4.fill_(GUARD)
        gg = GroupGemm([p4, p16.problem], variant=variant)
        assert _names()[gg.variant] == V2X and gg.info.qtype_mask == MX_BIT | MXW_BIT
        gg.launch()
        torch.cuda.synchronize()
        p16.check_close()
        out4 = c4.cpu().numpy()
        assert (out4[M] == np.float16(GUARD)).all()
        assert_f16_close(out4[:M], ref.gemm(ac.numpy(), asc.numpy(), bc.numpy(), bsc.numpy()), K)


def _w8a8_gate_up(M, Nh, K, seed):
    """A w8a8 gate_up problem, plain and with the SiLU flag (interleaved rows), on the same operands."""
    from mxmoe_amd.groupgemm import interleave_gate_up

    g = torch.Generator().manual_seed(seed)
    qa, sa = qz.quant_rtn_sym((torch.rand(M, K, generator=g) * 2 - 1).half().to(DEV), 8, -1)
    qb, sb = qz.quant_rtn_sym(((torch.rand(2 * Nh, K, generator=g) * 2 - 1) * 0.25).half().to(DEV), 8, -1)
    A, B = qz.pack_wxax(qa, 8), qz.pack_wxax(qb, 8)
    Bi, sbi = interleave_gate_up(B, sb)
    C = torch.empty(M, 2 * Nh, dtype=torch.float16, device=DEV)
    Cf = torch.full((M, Nh), float("nan"), dtype=torch.float16, device=DEV)
    return (Problem(A=A, B=B, C=C, M=M, N=2 * Nh, K=K, q=W8A8, scale_a=sa, scale_b=sb),
            Problem(A=A, B=Bi, C=Cf, M=M, N=2 * Nh, K=K, q=W8A8, scale_a=sa, scale_b=sbi, silu=True))


def test_t7_silu_epilogue():
    """On wo3 a fused problem (silu=True, gate / up rows interleaved) returns, bit for bit, the activation
    mxmoe_moe_silu_mul_quant computes from the plain problem's output; v2x refuses the flag for this type."""
    wo3 = _names().index(WO3)
    shapes = [(35, 256, 256), (70, 1408, 512), (1, 128, 128), (129, 512, 384), (0, 256, 256), (64, 128, 1024), (200, 384, 192)]
    plain, fused = [], []
    for i, (M, Nh, K) in enumerate(shapes):
        g = torch.Generator().manual_seed(90 + i)
        a = (torch.rand(M, K, generator=g) * 2 - 1).half().to(DEV)
        w = (torch.randn(2 * Nh, K, generator=g) * 0.25).half().to(DEV)
        wp, wi = moe.prepare_weight(w, W4A16_MXFP4), moe.prepare_weight(w, W4A16_MXFP4, interleave=True)
        ldc = Nh + 24 if i == 6 else 0
        C = torch.empty(max(M, 1), 2 * Nh, dtype=torch.float16, device=DEV)
        Cf = torch.full((max(M, 1), ldc or Nh), float("nan"), dtype=torch.float16, device=DEV)
        plain.append(Problem(A=a, B=wp.B, C=C, M=M, N=2 * Nh, K=K, q=W4A16_MXFP4, scale_b=wp.scale_b))
        fused.append(Problem(A=a, B=wi.B, C=Cf, M=M, N=2 * Nh, K=K, q=W4A16_MXFP4, scale_b=wi.scale_b, silu=True, ldc=ldc))
    GroupGemm(plain, variant=wo3).launch()
    gg = GroupGemm(fused)  # AUTO: the small-batch kernel, with the flag
    assert _names()[gg.variant] == WO3 and gg.info.qtype_mask == MXW_BIT | SILU_BIT
    gg.launch()
    torch.cuda.synchronize()
    for (M, Nh, K), p, f in zip(shapes, plain, fused):
        if M == 0:
            continue
        r = moe.route(torch.zeros(M, 1, dtype=torch.int32, device=DEV), 1)
        act = moe.silu_mul_quant(p.C[:M], None, r, [moe.ACT_FP16]).A(0)
        torch.cuda.synchronize()
        assert torch.equal(f.C[:M, :Nh].view(torch.int16), act.view(torch.int16)), (M, Nh, K)
        if f.C.shape[1] > Nh:
            assert torch.isnan(f.C[:M, Nh:]).all()
    with pytest.raises(nat.GGError, match="SiLU epilogue needs"):
        GroupGemm([fused[0]], variant=_names().index(V2X))
    # beside a w8a8 problem with the flag: the wide WO_SILU build
    p8, f8 = _w8a8_gate_up(48, 256, 512, seed=99)
    GroupGemm([p8], variant=wo3).launch()
    fused[0].C.fill_(float("nan"))
    gg = GroupGemm([fused[0], f8], variant=wo3)
    assert gg.info.qtype_mask == MXW_BIT | SILU_BIT | 2
    gg.launch()
    torch.cuda.synchronize()
    r = moe.route(torch.zeros(35, 1, dtype=torch.int32, device=DEV), 1)
    act = moe.silu_mul_quant(plain[0].C[:35], None, r, [moe.ACT_FP16]).A(0)
    assert torch.equal(fused[0].C[:35].view(torch.int16), act.view(torch.int16))
    want8 = moe_ref.silu_mul(p8.C[:48].cpu().numpy())
    d = np.abs(f8.C[:48, :256].cpu().numpy().view(np.uint16).astype(np.int32) - want8.view(np.uint16).astype(np.int32))
    assert (d <= 1).all()


# ---------------------------------------------------------------------------------------------
# T8: the layer
def _segment_rows(r, slot_rows: torch.Tensor, shared_rows):
    starts = np.concatenate([[0], np.cumsum(r.counts)])
    return [slot_rows[starts[e]:starts[e + 1]] for e in range(r.E)] + [shared_rows]


def _deq(w) -> np.ndarray:
    return ref.dequant(w.B.cpu().numpy(), qz.unpack_mxfp4_scales(w.scale_b.cpu(), w.K).numpy())


def _check_stages(layer, h, ids, wts, sw, out, mid):
    """A plain-form (no SiLU epilogue) layer of fp16-activation experts, stage by stage against the f64
    reference on the dequantised weights."""
    E, topk = layer.E, ids.shape[1]
    r, a1, h1, h1s, a2, y, ys = (mid[k] for k in ("routing", "a1", "h1", "h1s", "a2", "y", "ys"))
    _, perm, _, _ = moe_ref.route(ids.cpu().numpy(), E)
    hc = h.cpu()
    for e, rows in enumerate(_segment_rows(r, hc[torch.from_numpy(perm).long()], hc)):  # a1: the gathered rows, untouched
        if rows.shape[0]:
            assert torch.equal(a1.A(e).cpu().view(torch.int16), rows.view(torch.int16)), f"a1 seg {e}"
    for e, s in enumerate(a1.segs):
        if s.rows:
            C = (h1s if e == E else h1[s.first_slot:s.first_slot + s.rows]).cpu().numpy()
            assert_f16_close(C, a1.A(e).cpu().numpy().astype(np.float64) @ _deq(layer.w1[e]).T, layer.H)
    want = _segment_rows(r, torch.from_numpy(moe_ref.silu_mul(h1.cpu().numpy())), torch.from_numpy(moe_ref.silu_mul(h1s.cpu().numpy())))
    for e, s in enumerate(a2.segs):
        if s.rows:
            d = (a2.A(e).cpu().view(torch.int16).int() - want[e].view(torch.int16).int()).abs()
            assert d.max() <= 1, f"a2 seg {e}: {d.max()} fp16 steps"
    for e, s in enumerate(a2.segs):
        if s.rows:
            C = (ys if e == E else y[s.first_slot:s.first_slot + s.rows]).cpu().numpy()
            assert_f16_close(C, a2.A(e).cpu().numpy().astype(np.float64) @ _deq(layer.w2[e]).T, layer.w2[e].K)
    want_out = moe_ref.combine(y.cpu().numpy(), r.inv_slot.cpu().numpy(), wts.cpu().numpy(), topk, ys.cpu().numpy(),
                               None if sw is None else sw.cpu().numpy())
    assert (out.cpu().numpy().view(np.uint16) == want_out.view(np.uint16)).all()
    assert torch.isfinite(out.float()).all()


def _layer_weights(seed):
    E, H, N, Ns = 4, 256, 128, 256
    g = torch.Generator().manual_seed(seed)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)
    gate_up = [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)]
    down = [mk(H, N) for _ in range(E)] + [mk(H, Ns)]
    return E, H, g, gate_up, down


def test_t8_layer_stagewise():
    T, topk = 40, 2
    E, H, g, gate_up, down = _layer_weights(101)
    qcfg = [(W4A16_MXFP4, W4A16_MXFP4)] * (E + 1)
    plain = moe.MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=False)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
    h = torch.randn(T, H, generator=g).half().to(DEV)
    out, mid = plain.forward(h, ids, wts, return_intermediates=True)
    torch.cuda.synchronize()
    _check_stages(plain, h, ids, wts, None, out, mid)
    # the default layer fuses the SiLU epilogue on the small-batch kernel: bit-identical
    fused = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    assert fused.fuse_silu
    pf = moe.PlannedForward(fused, h, ids, wts)
    assert pf.mode == "fused" and _names()[pf.g1.variant] == WO3
    o2, m2 = fused.forward(h, ids, wts, return_intermediates=True)
    torch.cuda.synchronize()
    assert torch.equal(mid["a2"].out, m2["a2"].out) and torch.equal(out.view(torch.int16), o2.view(torch.int16))
    # the same through MoEBlock (router in front)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).half().to(DEV)
    ob, mb = moe.MoEBlock(plain, w_gate, topk, w_shared_gate=w_sg).forward(h, return_intermediates=True)
    torch.cuda.synchronize()
    _check_stages(plain, h, mb["topk_ids"], mb["topk_weights"], mb["shared_w"], ob, mb)


def test_t8_a16_view_of_an_a4_layer():
    T, topk = 40, 2
    E, H, g, gate_up, down = _layer_weights(102)
    a4 = moe.MoEFFN(gate_up, down, [(W4A4_MXFP4, W4A4_MXFP4)] * (E + 1), num_routed=E)
    v = a4.a16_view()
    for x, y in zip(a4.w1 + a4.w2, v.w1 + v.w2):
        assert x.B.data_ptr() == y.B.data_ptr() and x.scale_b.data_ptr() == y.scale_b.data_ptr() and y.q == W4A16_MXFP4
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
    h = torch.randn(T, H, generator=g).half().to(DEV)
    out, mid = v.forward(h, ids, wts, return_intermediates=True)
    torch.cuda.synchronize()
    _check_stages(v, h, ids, wts, None, out, mid)  # each GEMM within assert_f16_close of the fp16-activation reference
    assert torch.isfinite(a4.forward(h, ids, wts).float()).all()  # the a4 layer still runs on its own tensors
