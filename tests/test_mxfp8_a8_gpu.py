"""GPU tests of w4a8_g32_sym_MXFP8 (MXFP8 activations on the MXFP4 B operand): the mixed-format
block-scaled MFMA body of gg_tile_v2, forced onto the small-batch kernel wo3 (64 x 128 tiles), forced onto
v2x (256 / 128-row tiles) and through AUTO; the activation quantiser's MXFP8 tag; the layer.

"Exact" cases use A values that are multiples of 1/8 with |a| <= 8, any e2m1 B code (multiples of 0.5,
|b| <= 6) and scale codes 126..128 on both sides with K <= 416: every product is a multiple of 2^-4, every
scaled partial sum a multiple of 2^-6 below 416 * 8 * 6 * 4 < 2^17 — 23 bits, exact in f32 in any
order — so the fp16 result must equal fp16_rn of the f64 reference bit for bit. Random cases compare
against the f64 reference under assert_f16_close.

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
from mxmoe_amd.groupgemm import FP16, W4A4, W4A4_MXFP4, W4A8_MXFP8, W8A8, GroupGemm, Problem
from oracle import moe_ref
from tests import _mxfp4_ref as ref4
from tests import _mxfp8_ref as ref
from tests._util import HostProblem, assert_f16_close, exact_compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -1234.0
MX8_BIT, MX_BIT = 1 << 12, 1 << 10  # plan-info qtype_mask bits of QT_MXF8A / QT_MXF4
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


# e4m3 codes whose value is a multiple of 1/8 with |v| <= 8 (both signs, both zeros)
_EXACT_A = np.array([c for c in range(256) if not np.isnan(ref.CODE_VALUES[c]) and abs(ref.CODE_VALUES[c]) <= 8
                     and ref.CODE_VALUES[c] * 8 == np.round(ref.CODE_VALUES[c] * 8)], np.uint8)
ONE8, ONE4 = 0x38, 2  # e4m3 1.0, e2m1 1.0


class Mx8Problem:
    """Canonical operands (numpy: A MXFP8 codes [M, K], B MXFP4 codes [N, K/2], e8m0 scales [rows, K/32])
    + the device Problem with a guarded C."""

    def __init__(self, ac, asc, bc, bsc, ldc: int = 0, b_dev=None):
        self.ac, self.asc, self.bc, self.bsc = ac, asc, bc, bsc
        self.M, self.N, self.K = ac.shape[0], bc.shape[0], ac.shape[1]
        self.ldc = ldc or self.N
        self._ref = None
        self.b_dev = b_dev  # (B codes, device-layout scale_b) shared with another problem
        self.bind()

    def bind(self):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.Cbuf = torch.full((self.M + 1, self.ldc), GUARD, dtype=torch.float16, device=DEV)
        if self.b_dev is None:
            self.b_dev = (t(self.bc), qz.pack_mxfp4_scales(t(self.bsc)))
        self.problem = Problem(A=t(self.ac), B=self.b_dev[0], C=self.Cbuf, M=self.M, N=self.N, K=self.K, q=W4A8_MXFP8,
                               scale_a=qz.pack_mxfp4_scales(t(self.asc)), scale_b=self.b_dev[1], ldc=self.ldc)

    @property
    def expected(self) -> np.ndarray:  # f64, computed once
        if self._ref is None:
            self._ref = ref.gemm(self.ac, self.asc, self.bc, self.bsc)
        return self._ref

    def result(self) -> np.ndarray:
        c = self.Cbuf.cpu().numpy()
        assert (c[self.M] == np.float16(GUARD)).all(), "guard row behind C was written"
        assert (c[: self.M, self.N:] == np.float16(GUARD)).all(), "guard columns behind N were written"
        return c[: self.M, : self.N]

    def check_exact(self, what=""):
        with np.errstate(over="ignore"):
            want = self.expected.astype(np.float16)
        out = self.result()
        bad = out.view(np.uint16) != want.view(np.uint16)
        assert not bad.any(), f"{what}: {bad.sum()} / {bad.size} differ, first at {np.argwhere(bad)[:4].tolist()}"

    def check_close(self):
        assert_f16_close(self.result(), self.expected, self.K)


def _rand_quant(M, N, K, seed, b_scale=1.0, ldc=0) -> Mx8Problem:
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).half()
    b = (torch.randn(N, K, generator=g) * b_scale).half()
    ac, asc = qz.quant_mxfp8(a)
    bc, bsc = qz.quant_mxfp4(b)
    return Mx8Problem(ac.numpy(), asc.numpy(), bc.numpy(), bsc.numpy(), ldc=ldc)


def _run(problems, variant, expect=None):
    gg = GroupGemm([p.problem for p in problems], variant=_variant(variant))
    if variant != "auto":
        assert _names()[gg.variant] == (WO3 if variant == "wo3" else V2X)
    elif expect is not None:
        assert _names()[gg.variant] == expect
    gg.launch()
    torch.cuda.synchronize()
    return gg


def _scales(rng, rows, K):
    return rng.integers(126, 129, (rows, K // 32)).astype(np.uint8)


@VARIANTS
def test_t1_scale_map_exact(variant):
    """Every element is 1.0 on both sides, so C[m][n] = 32 sum_b 2^(sa[m][b] + sb[n][b] - 254): only the
    pairing of the scale bytes with the blocks (lane -> scale dword, the byte of the dword per K = 128
    stage, the 3.25-stage tail with its pad scales) decides the result."""
    M, N, K = 17, 136, 416
    rng = np.random.default_rng(11)
    asc, bsc = _scales(rng, M, K), _scales(rng, N, K)
    p = Mx8Problem(np.full((M, K), ONE8, np.uint8), asc, np.full((N, K // 2), ONE4 * 0x11, np.uint8), bsc)
    want = 32.0 * (np.exp2(asc.astype(np.float64) - 127) @ np.exp2(bsc.astype(np.float64) - 127).T)
    assert np.array_equal(p.expected, want)
    _run([p], variant, expect=WO3)
    p.check_exact("scale map")


@VARIANTS
def test_t2_element_map_exact(variant):
    """B row n one-hot at k = n: C[m][n] = a[m][n] 2^(sa + sb - 254) reads out every A byte position (the
    K position of each byte inside a lane's 32-byte block, the two 16-B halves of the block); the
    transposed problem (A one-hot e4m3 1.0) reads out every B nibble position."""
    M, N, K = 16, 416, 416
    rng = np.random.default_rng(12)
    a = _EXACT_A[rng.integers(0, len(_EXACT_A), (M, K))]
    hot4 = np.zeros((N, K), np.uint8)
    hot4[np.arange(N), np.arange(N)] = ONE4
    asc, bsc = _scales(rng, M, K), _scales(rng, N, K)
    p = Mx8Problem(a, asc, ref4.pack_nibbles(hot4), bsc)
    hot8 = np.zeros((N, K), np.uint8)
    hot8[np.arange(N), np.arange(N)] = ONE8
    nib = rng.integers(0, 16, (M, K)).astype(np.uint8)
    pt = Mx8Problem(hot8, bsc, ref4.pack_nibbles(nib), asc)  # M = 416 one-hot rows, N = 16 varied rows
    assert len(np.unique(p.expected)) > 60 and len(np.unique(pt.expected)) > 20
    _run([p, pt], variant)
    p.check_exact("A element map")
    pt.check_exact("B element map")


@VARIANTS
def test_t2b_exact_sums(variant):
    """Dense operands of the exact family (module docstring): the whole sum, bit for bit."""
    rng = np.random.default_rng(13)
    ps = []
    for M, N, K in ((70, 136, 416), (130, 264, 96), (300, 16, 288)):
        a = _EXACT_A[rng.integers(0, len(_EXACT_A), (M, K))]
        nib = rng.integers(0, 16, (N, K)).astype(np.uint8)
        ps.append(Mx8Problem(a, _scales(rng, M, K), ref4.pack_nibbles(nib), _scales(rng, N, K)))
    _run(ps, variant)
    for p in ps:
        p.check_exact(f"exact sums K={p.K}")


T3_SHAPES = [(M, 136, 1408) for M in (0, 1, 17, 130, 257, 513)] + [(130, N, 1408) for N in (8, 264, 520)] + \
            [(130, 136, K) for K in (32, 96, 128, 2048)]
_t3_cache: list = []


def _t3_problems():
    if not _t3_cache:
        _t3_cache.extend(_rand_quant(M, N, K, seed=300 + i) for i, (M, N, K) in enumerate(T3_SHAPES))
    return _t3_cache


@VARIANTS
def test_t3_random_parity(variant):
    ps = _t3_problems()
    for p in ps:
        p.bind()  # fresh guarded C per variant; operands and references are shared
    _run(ps, variant)
    for p in ps:
        p.check_close()


@VARIANTS
def test_t4_scale_range_exact(variant):
    """sa + sb - 254 spans [-40, 40] (one scale per row, so the unscaled sums stay exact and the comparison
    is bit for bit): fp16 subnormal results, and overflow to +-inf exactly where the reference's fp16
    conversion overflows."""
    M, N, K = 41, 48, 96
    rng = np.random.default_rng(14)
    a = _EXACT_A[rng.integers(0, len(_EXACT_A), (M, K))]
    bn = rng.integers(0, 16, (N, K)).astype(np.uint8)
    asc = np.repeat((127 - 20 + np.arange(M) % 41).astype(np.uint8)[:, None], K // 32, 1)
    bsc = np.repeat((127 - 20 + (np.arange(N) * 7) % 41).astype(np.uint8)[:, None], K // 32, 1)
    p = Mx8Problem(a, asc, ref4.pack_nibbles(bn), bsc)
    e = asc[:, :1].astype(int) + bsc[:, 0][None, :].astype(int) - 254
    assert e.min() == -40 and e.max() == 40
    with np.errstate(over="ignore"):
        want = p.expected.astype(np.float16)
    assert np.isinf(want).any() and (np.abs(want[want != 0]) < 2.0 ** -14).any()  # both ends are exercised
    _run([p], variant)
    p.check_exact("scale range")


@VARIANTS
def test_t5_mixed_launch(variant):
    """The new type beside w8a8, w4a4 and fp16 problems in one launch and — where the kernel has that
    body (v2x) — beside a w4a4_g32_sym_MXFP4 problem on the SAME B tensors."""
    mx = [_rand_quant(130, 136, 544, seed=51), _rand_quant(300, 264, 96, seed=52)]
    others = [HostProblem(150, 256, 512, W8A8, seed=53, device=DEV), HostProblem(129, 384, 512, W4A4, seed=54, device=DEV),
              HostProblem(77, 128, 192, FP16, seed=55, device=DEV)]
    probs = [mx[0].problem] + [h.problem for h in others] + [mx[1].problem]
    a4 = None
    if variant != "wo3":  # the a4 type has no wo3 body; with it AUTO keeps v2x
        g = torch.Generator().manual_seed(56)
        a4c, a4s = qz.quant_mxfp4(torch.randn(90, 544, generator=g).half())
        c4 = torch.full((91, 136), GUARD, dtype=torch.float16, device=DEV)
        a4 = (a4c, a4s, c4)
        probs.append(Problem(A=a4c.to(DEV), B=mx[0].b_dev[0], C=c4, M=90, N=136, K=544, q=W4A4_MXFP4,
                             scale_a=qz.pack_mxfp4_scales(a4s).to(DEV), scale_b=mx[0].b_dev[1]))
    gg = GroupGemm(probs, variant=_variant(variant))
    assert _names()[gg.variant] == (WO3 if variant == "wo3" else V2X)
    assert gg.info.qtype_mask & MX8_BIT and gg.info.qtype_mask & 7 == 7
    assert bool(gg.info.qtype_mask & MX_BIT) == (a4 is not None)
    gg.launch()
    torch.cuda.synchronize()
    for p in mx:
        p.check_close()
    if a4 is not None:
        got = a4[2].cpu().numpy()
        assert (got[90] == np.float16(GUARD)).all()
        assert_f16_close(got[:90], ref4.gemm(a4[0].numpy(), a4[1].numpy(), mx[0].bc, mx[0].bsc), 544)
    for h in others:
        out, want = h.result(), h.expected()
        if exact_compare(h.q):
            assert (out.view(np.uint16) == want.view(np.uint16)).all(), h.q.qcfg
        else:
            assert_f16_close(out, want, h.K)


@VARIANTS
def test_t6_strided_c_graph_rebind(variant):
    p = _rand_quant(70, 136, 352, seed=61, ldc=136 + 24)  # ldc > N: guard columns
    gg = _run([p], variant, expect=WO3)
    assert gg.info.qtype_mask == MX8_BIT  # the kernel that holds this tile body alone
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
    p2 = Mx8Problem(p.ac, p.asc, p.bc, p.bsc, ldc=136 + 24)  # rebind to fresh buffers of the same shapes
    gg.rebind([p2.problem])
    gg.launch()
    torch.cuda.synchronize()
    assert np.array_equal(p2.result().view(np.uint16), first.view(np.uint16))


@VARIANTS
def test_t6_split_k(variant):
    """A lone long-K call: the planner cuts its tiles along K at whole K = 128 stages; slices that start
    at a stage s with s % 4 != 0 begin in the middle of a four-stage scale dword."""
    ps = [_rand_quant(256, 256, 9984, seed=62, b_scale=0.05), _rand_quant(96, 256, 9984, seed=63, b_scale=0.05)]
    gg = _run(ps, variant)
    assert gg.info.splitk_slabs > 0
    tiles, _ = nat.plan_tiles([p.problem.to_c() for p in ps], gg.variant)
    starts = tiles[tiles[:, 0] >= 0][:, 4]
    assert (starts % 4 != 0).any(), sorted(set(starts.tolist()))
    for p in ps:
        p.check_close()
    first = [p.result().copy() for p in ps]
    gg.launch()
    torch.cuda.synchronize()
    for p, f in zip(ps, first):
        assert np.array_equal(p.result().view(np.uint16), f.view(np.uint16))


@VARIANTS
def test_nan_scale_stays_in_its_row_and_column(variant):
    """One A scale byte and one B scale byte are 255 (NaN): every output outside that row and column
    is bit-identical to the run without them."""
    p = _rand_quant(40, 72, 160, seed=71)
    q = _rand_quant(40, 72, 160, seed=71)
    q.asc[5, 2] = 255
    q.bsc[9, 0] = 255
    q.b_dev = None
    q.bind()
    _run([p, q], variant)
    want, got = p.result(), q.result()
    keep = np.ones_like(want, bool)
    keep[5, :] = False
    keep[:, 9] = False
    assert np.array_equal(got.view(np.uint16)[keep], want.view(np.uint16)[keep])
    print("NaN-scale row:", got[5, :4], "column:", got[:4, 9])


@pytest.mark.parametrize("variant", ["wo3", "v2x"])
def test_silu_epilogue_bit_identical(variant):
    """MXMOE_GG_EPI_SILU_MUL on interleaved B rows: bit-identical to the plain call on the same rows
    followed by the SiLU arithmetic of the activation kernel (mxmoe_moe_silu_mul_quant_il, fp16 tag)."""
    M, N, K = 75, 256, 544
    g = torch.Generator().manual_seed(65)
    ac, asc = qz.quant_mxfp8(torch.randn(M, K, generator=g).half())
    w = moe.prepare_weight((torch.randn(N, K, generator=g) * 0.1).half().to(DEV), W4A8_MXFP8, interleave=True)
    A, SA = ac.to(DEV), qz.pack_mxfp4_scales(asc).to(DEV)
    plain = torch.full((M + 1, N), GUARD, dtype=torch.float16, device=DEV)
    fused = torch.full((M + 1, N // 2 + 8), GUARD, dtype=torch.float16, device=DEV)
    v = _variant(variant)
    GroupGemm([Problem(A=A, B=w.B, C=plain, M=M, N=N, K=K, q=W4A8_MXFP8, scale_a=SA, scale_b=w.scale_b)], variant=v).launch()
    GroupGemm([Problem(A=A, B=w.B, C=fused, M=M, N=N, K=K, q=W4A8_MXFP8, scale_a=SA, scale_b=w.scale_b, ldc=N // 2 + 8,
                       silu=True)], variant=v).launch()
    ids = torch.zeros(M, 1, dtype=torch.int32, device=DEV)
    r = moe.route(ids, 1)
    act = moe.silu_mul_quant(plain[:M].contiguous(), None, r, [moe.ACT_FP16], interleaved=True)
    torch.cuda.synchronize()
    want = act.A(0)[r.inv_slot.view(-1).long()].cpu().numpy()
    got = fused.cpu().numpy()
    assert (got[M] == np.float16(GUARD)).all() and (got[:M, N // 2:] == np.float16(GUARD)).all()
    assert np.array_equal(got[:M, : N // 2].view(np.uint16), want.view(np.uint16))
    assert np.isfinite(want.astype(np.float32)).all() and np.abs(want.astype(np.float32)).max() > 0.1


# ---------------------------------------------------------------------------------------------
# T7: the activation quantiser's MXFP8 tag (act_quant_kernel), bit-exact against quant_mxfp8 and
# pack_mxfp4_scales; T8: the layer.
MXT = moe.ACT_MXFP8
ACT_E = 5
ACT_TAGS = [MXT, moe.ACT_INT8, MXT, moe.ACT_FP16, MXT]  # expert 2 gets no rows


def _act_ids(T, seed):
    """top-3 of experts {0, 1, 3, 4}; tokens 0 and 1 (the special rows) avoid the int8 expert, whose
    oracle does not define NaN rows. T * 3 routed slots: odd for odd T."""
    rng = np.random.default_rng(seed)
    ids = np.stack([rng.permutation([0, 1, 3, 4])[:3] for _ in range(T)]).astype(np.int32)
    ids[0] = ids[1] = [0, 4, 3]
    return torch.from_numpy(ids)


def _special_rows(x: torch.Tensor):
    """Rows 0 and 1 of fp16 [rows, W >= 128] get the quantiser's special blocks."""
    x[0, :32] = 0
    x[0, 32:64] = 0
    x[0, 33] = 2.0 ** -24
    x[0, 64:96] = torch.tensor([65504.0, -65504.0, 3.0e4, -1.0] * 8).half()
    # amax just below a power of two (saturation), exact ties, -0
    x[0, 96:128] = torch.tensor([1.999, -1.8, 1.75, 1.5, 0.0664, 0.0742, -0.0, 0.0, 2.0 ** -8, 3 * 2.0 ** -10, 1.0625,
                                 1.1875, -1.3125, 0.5625, 0.6875, -1.9375] * 2).half()
    x[1, :32] = 0
    x[1, 7] = -0.0
    x[1, 37] = float("nan")
    x[1, 70] = float("inf")
    x[1, 100] = float("-inf")
    return x


def _check_mx_seg(b, e, rows: torch.Tensor, what):
    codes, sc = qz.quant_mxfp8(rows)
    got = b.A(e).cpu()
    assert got.shape == codes.shape
    assert torch.equal(got, codes), f"{what}: seg {e} codes, {(got != codes).sum().item()} bytes differ"
    gs = b.scale(e).cpu()
    assert gs.dtype == torch.uint8 and torch.equal(gs, qz.pack_mxfp4_scales(sc)), f"{what}: seg {e} scales"


def _check_act_batch(b, rows, tags, what):
    for e, (x, tag) in enumerate(zip(rows, tags)):
        if x.shape[0] == 0:
            continue
        if tag == MXT:
            _check_mx_seg(b, e, x, what)
            continue
        stored, scale = moe_ref.quant_rows(x.numpy(), tag)
        got = b.A(e).cpu().numpy()
        if tag == moe.ACT_FP16:
            assert (got.view(np.uint16) == stored.view(np.uint16)).all(), f"{what}: seg {e}"
        else:
            assert (got == stored).all(), f"{what}: seg {e}"
            assert (b.scale(e).cpu().numpy().view(np.uint16) == scale.view(np.uint16)).all(), f"{what}: seg {e} scales"


def _segment_rows(r, slot_rows: torch.Tensor, shared_rows):
    starts = np.concatenate([[0], np.cumsum(r.counts)])
    rows = [slot_rows[starts[e]:starts[e + 1]] for e in range(r.E)]
    return rows + ([shared_rows] if shared_rows is not None else [])


def test_quantiser_rule_matches_the_restatement_on_the_special_rows():
    x = _special_rows(torch.zeros(2, 128, dtype=torch.float16))
    codes, sc = qz.quant_mxfp8(x)
    rc, rs = ref.quant(x.numpy())
    assert np.array_equal(codes.numpy(), rc) and np.array_equal(sc.numpy(), rs)


@pytest.mark.parametrize("with_shared", [False, True])
@pytest.mark.parametrize("K", [128, 512, 1408, 2048, 5632])
def test_t7_act_gather_bit_exact(K, with_shared):
    T = 33  # 99 routed slots
    ids = _act_ids(T, K)
    g = torch.Generator().manual_seed(K)
    h = _special_rows((torch.randn(T, K, generator=g) * torch.exp2(torch.randint(-6, 6, (T, 1), generator=g).float())).half())
    r = moe.route(ids.to(DEV), ACT_E)
    assert r.counts[2] == 0 and sum(r.counts) % 2 == 1
    tags = ACT_TAGS + ([MXT] if with_shared else [])
    b = moe.quant_act(h.to(DEV), r, tags, with_shared=with_shared)
    torch.cuda.synchronize()
    _, perm, _, _ = moe_ref.route(ids.numpy(), ACT_E)
    _check_act_batch(b, _segment_rows(r, h[torch.from_numpy(perm).long()], h if with_shared else None), tags, f"gather K={K}")


@pytest.mark.parametrize("N,Ns", [(128, 512), (1408, 5632), (2048, 2048)])  # the first two split the shared rows over 4 waves
def test_t7_act_slots_bit_exact(N, Ns):
    T = 33
    ids = _act_ids(T, N)
    r = moe.route(ids.to(DEV), ACT_E)
    g = torch.Generator().manual_seed(N)
    routed = (torch.randn(T * 3, N, generator=g) * 2).half()
    _special_rows(routed[r.first_slot[0]:])  # the first two slots of expert 0 (MXFP8)
    shared = _special_rows((torch.randn(T, Ns, generator=g) * 0.01).half())
    tags = ACT_TAGS + [MXT]
    b = moe.silu_mul_quant(routed.to(DEV), shared.to(DEV), r, tags, activated=True)
    torch.cuda.synchronize()
    _check_act_batch(b, _segment_rows(r, routed, shared), tags, f"slots N={N}")


@pytest.mark.parametrize("interleaved", [False, True], ids=["silu", "silu_interleaved"])
def test_t7_act_silu_modes(interleaved):
    """SiLU modes: the kernel's own activations (the same launch with fp16 tags) are within one fp16
    step of the libm restatement, and their MXFP8 quantisation is exact."""
    T, N, Ns = 33, 256, 512
    ids = _act_ids(T, 7)
    r = moe.route(ids.to(DEV), ACT_E)
    g = torch.Generator().manual_seed(8)
    routed = ((torch.rand(T * 3, 2 * N, generator=g) * 2 - 1) * 4).half()
    shared = ((torch.rand(T, 2 * Ns, generator=g) * 2 - 1) * 4).half()

    def plain(x):  # [gate | up] columns of an interleaved row (element e at 2 (e & ~15) + (e & 15), up 16 further)
        if not interleaved:
            return x
        w = x.shape[1] // 2
        v = x.reshape(x.shape[0], w // 16, 2, 16)
        return torch.cat([v[:, :, 0].reshape(-1, w), v[:, :, 1].reshape(-1, w)], dim=1)

    nseg = ACT_E + 1
    act = moe.silu_mul_quant(routed.to(DEV), shared.to(DEV), r, [moe.ACT_FP16] * nseg, interleaved=interleaved)
    b = moe.silu_mul_quant(routed.to(DEV), shared.to(DEV), r, [MXT] * nseg, interleaved=interleaved)
    torch.cuda.synchronize()
    want = _segment_rows(r, torch.from_numpy(moe_ref.silu_mul(plain(routed).numpy())),
                         torch.from_numpy(moe_ref.silu_mul(plain(shared).numpy())))
    for e in range(nseg):
        if want[e].shape[0] == 0:
            continue
        own = act.A(e).cpu()
        d = (own.view(torch.int16).int() - want[e].view(torch.int16).int()).abs()
        assert d.max() <= 1, f"seg {e}: act differs by {d.max()} fp16 steps"
        _check_mx_seg(b, e, own, "silu")


def _layer_weights(E, H, N, Ns, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half()
    gate_up = [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)]
    down = [mk(H, N) for _ in range(E)] + [mk(H, Ns)]
    return [w.to(DEV) for w in gate_up], [w.to(DEV) for w in down], g


def _mx_gemm_ref(a, e, w):  # f64 reference GEMM of the GPU's own quantised activations
    asc = qz.unpack_mxfp4_scales(a.scale(e).cpu(), w.K).numpy()
    bsc = qz.unpack_mxfp4_scales(w.scale_b.cpu(), w.K).numpy()
    return ref.gemm(a.A(e).cpu().numpy(), asc, w.B.cpu().numpy(), bsc)


def test_t8_layer_stagewise():
    """quant -> gate_up -> SiLU -> quant -> down -> combine, each stage against the restatement (the
    unfused layer: h1 holds the gate_up output)."""
    T, topk, E, H, N, Ns = 60, 2, 4, 256, 128, 256
    gate_up, down, g = _layer_weights(E, H, N, Ns, 81)
    MX = W4A8_MXFP8
    qcfg = [(MX, MX), (W8A8, W8A8), (FP16, FP16), (MX, MX), (MX, MX)]
    layer = moe.MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=False)
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1)
    h = (torch.randn(T, H, generator=g)).half()
    out, mid = layer.forward(h.to(DEV), ids.to(DEV), wts.to(DEV), return_intermediates=True)
    torch.cuda.synchronize()
    r, a1, h1, h1s, a2, y, ys = (mid[k] for k in ("routing", "a1", "h1", "h1s", "a2", "y", "ys"))
    _, perm, _, _ = moe_ref.route(ids.numpy(), E)
    _check_act_batch(a1, _segment_rows(r, h[torch.from_numpy(perm).long()], h), layer.tag1, "a1")
    for e, s in enumerate(a1.segs):
        if s.rows and layer.w1[e].q.fmt == "MXFP8":
            C = (h1s if e == E else h1[s.first_slot:s.first_slot + s.rows]).cpu().numpy()
            assert_f16_close(C, _mx_gemm_ref(a1, e, layer.w1[e]), H)
    act = moe.silu_mul_quant(h1, h1s, r, [moe.ACT_FP16] * (E + 1))
    torch.cuda.synchronize()
    want = _segment_rows(r, torch.from_numpy(moe_ref.silu_mul(h1.cpu().numpy())), torch.from_numpy(moe_ref.silu_mul(h1s.cpu().numpy())))
    for e, s in enumerate(a2.segs):
        if not s.rows:
            continue
        own = act.A(e).cpu()
        assert (own.view(torch.int16).int() - want[e].view(torch.int16).int()).abs().max() <= 1
        if layer.tag2[e] == MXT:
            _check_mx_seg(a2, e, own, "a2")
    for e, s in enumerate(a2.segs):
        if s.rows and layer.w2[e].q.fmt == "MXFP8":
            C = (ys if e == E else y[s.first_slot:s.first_slot + s.rows]).cpu().numpy()
            assert_f16_close(C, _mx_gemm_ref(a2, e, layer.w2[e]), layer.w2[e].K)
    want_out = moe_ref.combine(y.cpu().numpy(), r.inv_slot.cpu().numpy(), wts.numpy(), topk, ys.cpu().numpy())
    assert (out.cpu().numpy().view(np.uint16) == want_out.view(np.uint16)).all()
    assert torch.isfinite(out.float()).all()


@pytest.mark.parametrize("T", [60, 1500], ids=["wo3", "v2x"])
def test_t8_fused_silu_and_views(T):
    """The all-a8 layer: the fused SiLU epilogue is bit-identical to the unfused layer on the kernel AUTO
    picks (small batch: wo3, large: v2x), and a8_view() of an a4 layer equals a layer built as a8."""
    topk, E, H, N, Ns = 2, 4, 256, 128, 256
    gate_up, down, g = _layer_weights(E, H, N, Ns, 82)
    MX = W4A8_MXFP8
    fused = moe.MoEFFN(gate_up, down, [(MX, MX)] * (E + 1), num_routed=E)
    unfused = moe.MoEFFN(gate_up, down, [(MX, MX)] * (E + 1), num_routed=E, fuse_silu=False)
    view = moe.MoEFFN(gate_up, down, [(W4A4_MXFP4, W4A4_MXFP4)] * (E + 1), num_routed=E).a8_view()
    assert fused.fuse_silu and not unfused.fuse_silu and not view.fuse_silu
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
    h = torch.randn(T, H, generator=g).half().to(DEV)
    a1 = moe.quant_act(h, moe.route(ids, E), fused.tag1, True)
    g1, _, _, mode = fused.gate_up_call(a1, T, topk, h.device)
    assert mode == "fused" and _names()[g1.variant] == (WO3 if T == 60 else V2X) and g1.info.qtype_mask == MX8_BIT
    outs = [layer.forward(h, ids, wts) for layer in (fused, unfused, view)]
    torch.cuda.synchronize()
    assert torch.isfinite(outs[0].float()).all() and outs[0].float().abs().max() > 0
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))
    assert torch.equal(outs[2].view(torch.int16), outs[1].view(torch.int16))


def test_t8_moe_block_equals_gate_plus_ffn():
    T, topk, E, H, N, Ns = 40, 2, 4, 256, 128, 256
    gate_up, down, g = _layer_weights(E, H, N, Ns, 83)
    MX = W4A8_MXFP8
    ffn = moe.MoEFFN(gate_up, down, [(MX, MX)] * (E + 1), num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * 0.1).half().to(DEV)
    w_sg = (torch.randn(H, generator=g) * 0.1).half().to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, w_shared_gate=w_sg)
    h = torch.randn(T, H, generator=g).half().to(DEV)
    out = block.forward(h)
    ids, wts, sw = moe.gate(h, w_gate, topk, w_shared_gate=w_sg)[:3]
    want = ffn.forward(h, ids, wts, shared_w=sw)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int16), want.view(torch.int16))
