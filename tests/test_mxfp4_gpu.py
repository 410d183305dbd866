"""GPU tests of the MXFP4 (w4a4_g32_sym_MXFP4) GroupGEMM tile: the block-scaled fp4 MFMA body of
gg_tile_v2, on the v2x variant and through AUTO.

"Exact" cases use operand codes (multiples of 0.5) and scale codes 126..128 on both sides with
K <= 416: every partial sum, in any order, is a multiple of 2^-4 below 2^17, so the f32 accumulation is
exact and the fp16 result must equal fp16_rn of the f64 reference bit for bit (the E4M3 known-answer
test's argument). Random cases compare against the f64 reference under assert_f16_close.

Every C buffer carries one guard row behind row M and, where ldc > N, guard columns: they must keep
their fill value.
"""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import FP16, W4A4, W4A4_MXFP4, W8A8, GroupGemm, Problem
from tests import _mxfp4_ref as ref
from tests._util import HostProblem, assert_f16_close, exact_compare

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -1234.0
MX_BIT = 1 << 10  # plan-info qtype_mask bit of QT_MXF4


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    nat.lib()


def _v2x():
    return nat.default_variant()


VARIANTS = pytest.mark.parametrize("variant", ["v2x", "auto"])


def _variant(name):
    return _v2x() if name == "v2x" else None


class MxProblem:
    """Canonical MXFP4 operands (numpy) + the device Problem with a guarded C."""

    def __init__(self, ac, asc, bc, bsc, ldc: int = 0):
        self.ac, self.asc, self.bc, self.bsc = ac, asc, bc, bsc
        self.M, self.N, self.K = ac.shape[0], bc.shape[0], 2 * ac.shape[1]
        self.ldc = ldc or self.N
        self._ref = None
        self.bind()

    def bind(self):
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
        self.Cbuf = torch.full((self.M + 1, self.ldc), GUARD, dtype=torch.float16, device=DEV)
        self.problem = Problem(A=t(self.ac), B=t(self.bc), C=self.Cbuf, M=self.M, N=self.N, K=self.K, q=W4A4_MXFP4,
                               scale_a=qz.pack_mxfp4_scales(t(self.asc)), scale_b=qz.pack_mxfp4_scales(t(self.bsc)),
                               ldc=self.ldc)

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


def _rand_quant(M, N, K, seed, b_scale=1.0) -> MxProblem:
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).half()
    b = (torch.randn(N, K, generator=g) * b_scale).half()
    ac, asc = qz.quant_mxfp4(a)
    bc, bsc = qz.quant_mxfp4(b)
    return MxProblem(ac.numpy(), asc.numpy(), bc.numpy(), bsc.numpy())


def _run(problems, variant):
    gg = GroupGemm([p.problem for p in problems], variant=_variant(variant))
    if variant == "auto":
        assert gg.variant == _v2x()  # AUTO sends every call with an MXFP4 problem to v2x
    gg.launch()
    torch.cuda.synchronize()
    return gg


@VARIANTS
def test_t1_scale_map_exact(variant):
    """Every element is 1.0, so C[m][n] = 32 sum_b 2^(sa[m][b] + sb[n][b] - 254): only the pairing of
    the scale bytes with the blocks (lane -> scale byte, the op_sel sequence over the MFMAs of two
    stages, the 1.625-stage tail with its pad scales) decides the result."""
    M, N, K = 17, 136, 416
    rng = np.random.default_rng(11)
    ones = np.full((1, K // 2), 0x22, np.uint8)  # nibble 2 = 1.0
    asc = rng.integers(126, 129, (M, K // 32)).astype(np.uint8)
    bsc = rng.integers(126, 129, (N, K // 32)).astype(np.uint8)
    p = MxProblem(np.repeat(ones, M, 0), asc, np.repeat(ones, N, 0), bsc)
    want = 32.0 * (np.exp2(asc.astype(np.float64) - 127) @ np.exp2(bsc.astype(np.float64) - 127).T)
    assert np.array_equal(p.expected, want)
    _run([p], variant)
    p.check_exact("scale map")


@VARIANTS
def test_t2_element_map_exact(variant):
    """B row n is one-hot at k = n (every k of every block is hit): C[m][n] = a[m][n] 2^(sa + sb - 254)
    reads out every A element, so the K position of each nibble inside a lane's block is pinned; the
    transposed problem (A one-hot) pins B's."""
    M, N, K = 16, 416, 416
    rng = np.random.default_rng(12)
    nib = rng.integers(0, 16, (M, K)).astype(np.uint8)
    hot = np.zeros((N, K), np.uint8)
    hot[np.arange(N), np.arange(N) % K] = 2  # 1.0
    asc = rng.integers(126, 129, (M, K // 32)).astype(np.uint8)
    bsc = rng.integers(126, 129, (N, K // 32)).astype(np.uint8)
    p = MxProblem(ref.pack_nibbles(nib), asc, ref.pack_nibbles(hot), bsc)
    # the transpose: M = 416 one-hot rows (two row tiles' worth of classes), N = 16 varied rows
    pt = MxProblem(ref.pack_nibbles(hot), bsc, ref.pack_nibbles(nib), asc)
    _run([p, pt], variant)
    p.check_exact("A element map")
    pt.check_exact("B element map")


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
    """sa + sb - 254 spans [-40, 40] (one scale per row, so the unscaled sums stay exact and the
    comparison is bit for bit): fp16 subnormal results, and overflow to +-inf exactly where the
    reference's fp16 conversion overflows. Scale codes that would take a product or a sum into the
    f32-subnormal range (sa + sb - 254 below about -120) are left out: the MFMA's handling of f32
    denormals is not part of this contract."""
    M, N, K = 41, 48, 96
    rng = np.random.default_rng(14)
    an = rng.integers(0, 16, (M, K)).astype(np.uint8)
    bn = rng.integers(0, 16, (N, K)).astype(np.uint8)
    asc = np.repeat((127 - 20 + np.arange(M) % 41).astype(np.uint8)[:, None], K // 32, 1)
    bsc = np.repeat((127 - 20 + (np.arange(N) * 7) % 41).astype(np.uint8)[:, None], K // 32, 1)
    p = MxProblem(ref.pack_nibbles(an), asc, ref.pack_nibbles(bn), bsc)
    e = asc[:, :1].astype(int) + bsc[:, 0][None, :].astype(int) - 254
    assert e.min() == -40 and e.max() == 40
    with np.errstate(over="ignore"):
        want = p.expected.astype(np.float16)
    assert np.isinf(want).any() and (np.abs(want[want != 0]) < 2.0 ** -14).any()  # both ends are exercised
    _run([p], variant)
    p.check_exact("scale range")


@VARIANTS
def test_t5_mixed_launch(variant):
    """MXFP4 beside w8a8, w4a4 and fp16 problems in one launch (the every-body kernel)."""
    mx = [_rand_quant(130, 136, 544, seed=51), _rand_quant(300, 264, 96, seed=52)]
    others = [HostProblem(150, 256, 512, W8A8, seed=53, device=DEV), HostProblem(129, 384, 512, W4A4, seed=54, device=DEV),
              HostProblem(77, 128, 192, FP16, seed=55, device=DEV)]
    gg = GroupGemm([mx[0].problem] + [h.problem for h in others] + [mx[1].problem], variant=_variant(variant))
    assert gg.variant == _v2x() and gg.info.qtype_mask & MX_BIT and gg.info.qtype_mask & 7 == 7
    gg.launch()
    torch.cuda.synchronize()
    for p in mx:
        p.check_close()
    for h in others:
        out, want = h.result(), h.expected()
        if exact_compare(h.q):
            assert (out.view(np.uint16) == want.view(np.uint16)).all(), h.q.qcfg
        else:
            assert_f16_close(out, want, h.K)


@VARIANTS
def test_t6_strided_c_graph_rebind(variant):
    g = torch.Generator().manual_seed(61)
    a, b = torch.randn(70, 352, generator=g).half(), torch.randn(136, 352, generator=g).half()
    (ac, asc), (bc, bsc) = qz.quant_mxfp4(a), qz.quant_mxfp4(b)
    p = MxProblem(ac.numpy(), asc.numpy(), bc.numpy(), bsc.numpy(), ldc=136 + 24)  # ldc > N: guard columns
    gg = _run([p], variant)
    assert gg.info.qtype_mask == MX_BIT  # the MXFP4-only kernel
    p.check_close()
    first = p.result().copy()
    # graph capture and replay
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        gg.launch(s)
    p.Cbuf[: p.M, : p.N].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(p.result().view(np.uint16), first.view(np.uint16))  # bit-identical across launches
    # rebind to fresh buffers of the same shapes
    p2 = MxProblem(ac.numpy(), asc.numpy(), bc.numpy(), bsc.numpy(), ldc=136 + 24)
    gg.rebind([p2.problem])
    gg.launch()
    torch.cuda.synchronize()
    assert np.array_equal(p2.result().view(np.uint16), first.view(np.uint16))


@VARIANTS
def test_t6_split_k(variant):
    """A lone long-K call: the planner cuts its tiles along K at whole 128-B stages — an odd first
    stage starts in the middle of a two-stage scale group."""
    ps = [_rand_quant(256, 256, 9984, seed=62, b_scale=0.05), _rand_quant(96, 256, 9984, seed=63, b_scale=0.05)]
    gg = _run(ps, variant)
    assert gg.info.splitk_slabs > 0
    for p in ps:
        p.check_close()
    first = [p.result().copy() for p in ps]
    gg.launch()
    torch.cuda.synchronize()
    for p, f in zip(ps, first):
        assert np.array_equal(p.result().view(np.uint16), f.view(np.uint16))


@pytest.mark.parametrize("mixed", [False, True], ids=["mxfp4_only", "mixed"])
def test_nan_scale_stays_in_its_row_and_column(mixed):
    """One A scale byte and one B scale byte are 255 (NaN). What the kernel returns in that row and
    column is recorded in DESIGN.md, not asserted; every other output must be unaffected — in the
    MXFP4-only kernel and, with a w8a8 problem in the call, in the every-body kernel."""
    p = _rand_quant(40, 72, 160, seed=71)
    q = _rand_quant(40, 72, 160, seed=71)
    q.asc[5, 2] = 255
    q.bsc[9, 0] = 255
    q.bind()
    w8 = HostProblem(150, 256, 512, W8A8, seed=72, device=DEV)
    gg = GroupGemm([p.problem, q.problem] + ([w8.problem] if mixed else []), variant=_v2x())
    assert (gg.info.qtype_mask == MX_BIT) != mixed
    gg.launch()
    torch.cuda.synchronize()
    want, got = p.result(), q.result()
    keep = np.ones_like(want, bool)
    keep[5, :] = False
    keep[:, 9] = False
    assert np.array_equal(got.view(np.uint16)[keep], want.view(np.uint16)[keep])
    if mixed:
        assert (w8.result().view(np.uint16) == w8.expected().view(np.uint16)).all()
    print("NaN-scale row:", got[5, :4], "column:", got[:4, 9])


# ---------------------------------------------------------------------------------------------
# T7: the activation quantiser's MXFP4 tag (act_quant_kernel), bit-exact against quant_mxfp4 and
# pack_mxfp4_scales; T8: the layer.
from mxmoe_amd import moe  # noqa: E402
from oracle import moe_ref  # noqa: E402

MXT = moe.ACT_MXFP4
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
    x[0, 96:128] = torch.tensor([6.0, -0.0, 0.25, -0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, -5.0, 7.5, 0.0, 0.1, -0.1, 4.0] * 2).half()
    x[1, 5] = float("nan")
    x[1, 40] = float("inf")
    x[1, 70] = float("-inf")
    return x


def _check_mx_seg(b, e, rows: torch.Tensor, what):
    codes, sc = qz.quant_mxfp4(rows)
    got = b.A(e).cpu()
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
    _special_rows(routed[r.first_slot[0]:])  # the first two slots of expert 0 (MXFP4)
    shared = _special_rows((torch.randn(T, Ns, generator=g) * 0.01).half())
    tags = ACT_TAGS + [MXT]
    b = moe.silu_mul_quant(routed.to(DEV), shared.to(DEV), r, tags, activated=True)
    torch.cuda.synchronize()
    _check_act_batch(b, _segment_rows(r, routed, shared), tags, f"slots N={N}")


@pytest.mark.parametrize("interleaved", [False, True], ids=["silu", "silu_interleaved"])
def test_t7_act_silu_modes(interleaved):
    """SiLU modes: the kernel's own activations (the same launch with fp16 tags) are within one fp16
    step of the libm restatement, and their MXFP4 quantisation is exact."""
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


def test_t8_layer_stagewise():
    T, topk, E, H, N, Ns = 60, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(81)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half()
    gate_up = [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)]
    down = [mk(H, N) for _ in range(E)] + [mk(H, Ns)]
    MX = W4A4_MXFP4
    qcfg = [(MX, MX), (W8A8, W8A8), (FP16, FP16), (MX, MX), (MX, MX)]
    layer = moe.MoEFFN([w.to(DEV) for w in gate_up], [w.to(DEV) for w in down], qcfg, num_routed=E)
    assert not layer.fuse_silu  # MXFP4 has no SiLU epilogue: the plain form
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1)
    h = (torch.randn(T, H, generator=g)).half()
    out, mid = layer.forward(h.to(DEV), ids.to(DEV), wts.to(DEV), return_intermediates=True)
    torch.cuda.synchronize()
    r, a1, h1, h1s, a2, y, ys = (mid[k] for k in ("routing", "a1", "h1", "h1s", "a2", "y", "ys"))
    _, perm, _, _ = moe_ref.route(ids.numpy(), E)
    # a1: bit-exact quantisation of the gathered hidden rows
    _check_act_batch(a1, _segment_rows(r, h[torch.from_numpy(perm).long()], h), layer.tag1, "a1")

    def mx_gemm_ref(a, e, w):  # f64 reference GEMM of the GPU's own quantised activations
        K = w.K
        asc = qz.unpack_mxfp4_scales(a.scale(e).cpu(), K).numpy()
        bsc = qz.unpack_mxfp4_scales(w.scale_b.cpu(), K).numpy()
        return ref.gemm(a.A(e).cpu().numpy(), asc, w.B.cpu().numpy(), bsc)

    # h1 against the reference GEMM of a1 (MXFP4 experts; the others are covered by tests/test_moe.py)
    for e, s in enumerate(a1.segs):
        if s.rows and layer.w1[e].q.fmt == "MXFP4":
            C = (h1s if e == E else h1[s.first_slot:s.first_slot + s.rows]).cpu().numpy()
            assert_f16_close(C, mx_gemm_ref(a1, e, layer.w1[e]), H)
    # a2 consistent with h1: the kernel's own activations of h1 (fp16 tags), quantised exactly
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
    # y against the reference down GEMM of a2, then the combine bit-exact
    for e, s in enumerate(a2.segs):
        if s.rows and layer.w2[e].q.fmt == "MXFP4":
            C = (ys if e == E else y[s.first_slot:s.first_slot + s.rows]).cpu().numpy()
            assert_f16_close(C, mx_gemm_ref(a2, e, layer.w2[e]), layer.w2[e].K)
    want_out = moe_ref.combine(y.cpu().numpy(), r.inv_slot.cpu().numpy(), wts.numpy(), topk, ys.cpu().numpy())
    assert (out.cpu().numpy().view(np.uint16) == want_out.view(np.uint16)).all()
    assert torch.isfinite(out.float()).all()


def test_reference_named_entry_points_take_mxfp4_tuples():
    """quant_inp_act and gg_mxmoe_share_fused with qparams (4, 4, 32, 1) for some experts: the tuple
    alone selects MXFP4 (there is no integer g32 type), beside w8a8 experts in the same fused call."""
    from oracle import oracle

    T, topk, E, H, N = 40, 2, 4, 256, 128
    g = torch.Generator().manual_seed(91)
    qs = [W4A4_MXFP4, W8A8, W4A4_MXFP4, W8A8, W4A4_MXFP4]  # shared expert last
    qparams = [(q.a_bits, q.w_bits, q.gsize, int(q.sym)) for q in qs]
    ws = [moe.prepare_weight((((torch.rand(2 * N, H, generator=g) * 2 - 1) * 0.2).half()).to(DEV), q) for q in qs]
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32)
    h = torch.randn(T, H, generator=g).half().to(DEV)
    inp, sc, out, *_rest = moe.quant_inp_act(h, ids.to(DEV), E, N, 1, qparams)
    counts = _rest[3]
    moe.gg_mxmoe_share_fused(inp, [w.B for w in ws], sc, [w.scale_b for w in ws], out, 2 * N, H, 2 * N, H, qparams, counts)
    torch.cuda.synchronize()
    experts = [e for e in range(E) if int(counts[e]) > 0] + [E]
    assert len(experts) == len(inp) == E + 1
    for pi, e in enumerate(experts):
        w, got = ws[e], out[pi].cpu().numpy()
        if w.q.fmt == "MXFP4":
            assert sc[pi].dtype == torch.uint8
            want = ref.gemm(inp[pi].cpu().numpy(), qz.unpack_mxfp4_scales(sc[pi].cpu(), H).numpy(),
                            w.B.cpu().numpy(), qz.unpack_mxfp4_scales(w.scale_b.cpu(), H).numpy())
            assert_f16_close(got, want, H)
        else:
            want = oracle.gg_quant(inp[pi].cpu().numpy(), w.B.cpu().numpy(), sc[pi].cpu().numpy(), w.scale_b.cpu().numpy(),
                                   got.shape[0], w.N, w.K, 8)
            assert (got.view(np.uint16) == want.view(np.uint16)).all(), f"expert {e}"
