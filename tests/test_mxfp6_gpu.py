"""w6a6_g32_sym_MXFP6 on the GPU: the tile body (exact v2x build and the widest fallback) read out bit for bit and on
random operands against float64, the activation quantiser (tag 12) bit for bit against ``pack_mxfp6(quant_mxfp6(x))``,
and layers stage by stage. The reference is ``quantize.dequant_mxfp6`` throughout. GEMM bound (derived, not tuned):
|C - ref| <= 2^-11 |ref| (the fp16 rounding) + K 2^-24 sum |a_k b_k| (f32 accumulation, any order) + 2^-25."""
import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import FP16, W6A6_MXFP6 as M6, W8A8, GroupGemm, Problem
from oracle import moe_ref
from tests._decode_util import assert_act_close
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 128, 128), (130, 264, 512), (300, 520, 1152)]  # one stage | a ring that wraps | both tile classes, guards
BUILDS = pytest.mark.parametrize("mixed", [False, True], ids=["exact", "widest"])


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _deq(image, dev_scales, K):
    return qz.dequant_mxfp6(qz.unpack_mxfp6(image.cpu()), qz.unpack_mxfp4_scales(dev_scales.cpu(), K))


def _within_bound(got, a, b, K):
    ref, mag = a @ b.T, a.abs() @ b.abs().T
    return ((got.cpu().double() - ref).abs() <= 2.0 ** -11 * ref.abs() + K * 2.0 ** -24 * mag + 2.0 ** -25).all()


def _run(ca, sa, cb, sb, mixed):
    """(C, a, b): C of one MXFP6 problem from 6-bit codes [rows, K] and scales [rows, K/32], alone (the exact build) or
    beside one fp16 problem (the kernel with every tile body), and the operands' float64 values."""
    (M, K), N = ca.shape, cb.shape[0]
    A, B = (qz.pack_mxfp6(qz._pack6(c)).to(DEV) for c in (ca, cb))
    SA, SB = (qz.pack_mxfp4_scales(s).to(DEV) for s in (sa, sb))
    C = torch.full((M + 1, N), 777.0, dtype=torch.float16, device=DEV)
    probs = [Problem(A=A, B=B, C=C, M=M, N=N, K=K, q=M6, scale_a=SA, scale_b=SB)]
    if mixed:
        z = torch.zeros(16, 64, dtype=torch.float16, device=DEV)
        probs.append(Problem(A=z, B=z, C=torch.zeros(16, 16, dtype=torch.float16, device=DEV), M=16, N=16, K=64, q=FP16))
    gg = GroupGemm(probs, variant=nat.default_variant())
    assert (gg.info.qtype_mask == 1 << 14) == (not mixed) and gg.info.qtype_mask & (1 << 14)
    gg.launch()
    torch.cuda.synchronize()
    assert (C[M] == 777.0).all(), "guard row behind C was written"
    return C[:M].cpu(), _deq(A, SA, K), _deq(B, SB, K)


@BUILDS
@pytest.mark.parametrize("dense_a", [True, False], ids=["denseA", "denseB"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_readout_bit_for_bit(M, N, K, dense_a, mixed):
    """Every output is ONE product times two scales: the dense side holds code (row + k) % 64 — from 64 rows on, every
    code at every position of every block of every lane group — the other side one non-zero code per row. Scales walk
    a ladder, with 0, 254 and 255 on chosen rows and blocks. Expected: fp16_rn of the float64 value, NaN where it is
    NaN; a zero may carry either sign (the f32 sum of a -0 product onto the +0 accumulator is +0)."""
    rows_d, rows_o = (M, N) if dense_a else (N, M)
    dense = ((torch.arange(rows_d)[:, None] + torch.arange(K)[None, :]) % 64).to(torch.uint8)
    onehot = torch.zeros(rows_o, K, dtype=torch.uint8)
    r = torch.arange(rows_o)
    onehot[r, (r * 37 + 5) % K] = ((r * 11 + 9) % 63 + 1).to(torch.uint8)
    ladder = torch.tensor([127, 125, 130, 127, 124, 129], dtype=torch.uint8)

    def scales(rows, special):
        s = ladder[(torch.arange(rows)[:, None] + torch.arange(K // 32)[None, :]) % 6].clone()
        for row, blk, code in special:
            if row < rows:
                s[row, blk if blk is not None else slice(None)] = code
        return s

    sd = scales(rows_d, [(3, None, 0), (4, None, 254), (5, 1, 255)])
    so = scales(rows_o, [(6, None, 254), (7, None, 0), (9, 0, 255)])
    got, a, b = _run(*((dense, sd, onehot, so) if dense_a else (onehot, so, dense, sd)), mixed)
    with np.errstate(over="ignore", invalid="ignore"):
        want = torch.from_numpy((a.numpy() @ b.numpy().T).astype(np.float16))
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan)
    got[nan] = want[nan] = 0
    bad = (got != want) | ((got.view(torch.int16) != want.view(torch.int16)) & (want != 0))
    assert not bad.any(), f"{int(bad.sum())} of {bad.numel()} differ, first at {bad.nonzero()[:4].tolist()}"


@BUILDS
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_gemm_random_codes_and_scales(M, N, K, mixed):
    """Scale codes in [121, 127] (2^-6 .. 1 per side): sum |a_k b_k| <= 1152 * 56.25 = 64800 < 65504, so no reference
    output or partial sum leaves fp16's finite range (checked below)."""
    g = torch.Generator().manual_seed(M + K)
    ca, cb = (torch.randint(0, 64, (n, K), generator=g, dtype=torch.uint8) for n in (M, N))
    sa, sb = (torch.randint(121, 128, (n, K // 32), generator=g, dtype=torch.uint8) for n in (M, N))
    got, a, b = _run(ca, sa, cb, sb, mixed)
    assert (a.abs() @ b.abs().T).max() < 65504 and _within_bound(got, a, b, K)


def _check_seg(b, e, x, what):
    codes, sc = qz.quant_mxfp6(x)
    assert torch.equal(b.A(e).cpu(), qz.pack_mxfp6(codes)), f"{what}: segment {e} codes"
    assert torch.equal(b.scale(e).cpu(), qz.pack_mxfp4_scales(sc)), f"{what}: segment {e} scales"


@pytest.mark.parametrize("src", ["fp16", "bf16"])
def test_quantiser_gather_bit_for_bit(src):
    """Tag 12 through the gather (mxmoe_moe_act_quant / mxmoe_moe_gather_quant from bf16), width 2048, routed rows and the
    shared expert's: every finite fp16 bit pattern once in a fixed seeded order, then an all-zero block, a -0 block, a
    block with Inf and one with NaN. bf16: the same rows rounded to bf16 first."""
    W, E = 2048, 2
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7C00) != 0x7C00]
    bits = bits[torch.randperm(bits.numel(), generator=torch.Generator().manual_seed(6))].to(torch.int16)
    tail = torch.zeros(4, 32, dtype=torch.float16)
    tail[1] = -0.0
    tail[2], tail[3] = 1.0, -2.0
    tail[2, 7], tail[3, 30] = float("inf"), float("nan")
    x = torch.cat([bits.view(torch.float16), tail.reshape(-1)])
    x = torch.cat([x, torch.zeros(-x.numel() % W, dtype=torch.float16)]).reshape(-1, W)
    hidden = x.to(DEV)
    if src == "bf16":
        hidden = x.float().to(torch.bfloat16).to(DEV)
        x = hidden.cpu().to(torch.float16)
    r = moe.route((torch.arange(x.shape[0], dtype=torch.int32)[:, None] % E).contiguous().to(DEV), E)
    b = moe.quant_act(hidden, r, [moe.ACT_MXFP6] * (E + 1), with_shared=True)
    torch.cuda.synchronize()
    perm, starts = r.perm_token.cpu().long(), np.concatenate([[0], np.cumsum(r.counts)])
    for e in range(E + 1):
        _check_seg(b, e, x if e == E else x[perm[starts[e]:starts[e + 1]]], src)


def test_quantiser_glu_bias_swiglu_clamp_bit_for_bit():
    """Tag 12 behind mxmoe_moe_glu_quant (a gate_up bias and SwigluClamp, width 256): the host rule applied to the
    kernel's own activations (the same launch with fp16 tags)."""
    T, E, N = 33, 2, 256
    g = torch.Generator().manual_seed(3)
    r = moe.route((torch.arange(T, dtype=torch.int32)[:, None] % E).contiguous().to(DEV), E)
    routed, shared = (((torch.rand(T, 2 * N, generator=g) * 2 - 1) * 6).half().to(DEV) for _ in range(2))
    kw = dict(activation=moe.SwigluClamp(), bias_routed=torch.randn(E, 2 * N, generator=g).half().to(DEV),
              bias_shared=torch.randn(2 * N, generator=g).half().to(DEV))
    act = moe.glu_quant(routed, shared, r, [moe.ACT_FP16] * (E + 1), **kw)
    b = moe.glu_quant(routed, shared, r, [moe.ACT_MXFP6] * (E + 1), **kw)
    torch.cuda.synchronize()
    for e in range(E + 1):
        _check_seg(b, e, act.A(e).cpu(), "glu")


@pytest.mark.parametrize("qcfg", [[(M6, M6)] * 4, [(M6, M6), (W8A8, M6), (FP16, FP16), (M6, W8A8), (M6, M6)]],
                         ids=["all_mxfp6", "mixed_shared"])
def test_layer_stagewise_planned_and_graph(qcfg):
    """E = 4, topk = 2, H = 256, N = 128, T = 33, every expert MXFP6, or MXFP6 / w8a8 / fp16 mixed per expert and per
    linear with an MXFP6 shared expert. Each stage against the restatement of the stage before it: a1 = quant_mxfp6 of
    the gathered rows; h1 = dequant(a1) . dequant(w1)^T under the GEMM bound (fp16 experts: the fp16 tolerance); the
    activation of h1, in slot order, under assert_act_close, and a2 = quant_mxfp6 of it; y likewise from a2; out = the
    oracle's combine of y, bit for bit. PlannedForward and GraphForward (its second pass replays the plans on another
    routing) equal the eager out bit for bit."""
    T, topk, E, H, N, Ns = 33, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(13)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)  # noqa: E731
    sh = len(qcfg) > E
    layer = moe.MoEFFN([mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)] * sh, [mk(H, N) for _ in range(E)] + [mk(H, Ns)] * sh,
                       qcfg, num_routed=E)
    gf = moe.GraphForward(layer, T, topk)
    for rep in range(2):
        h = torch.randn(T, H, generator=g).half().to(DEV)
        ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
        wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
        out, mid = layer.forward(h, ids, wts, return_intermediates=True)
        r, h1, h1s, ys = mid["routing"], mid["h1"], mid.get("h1s"), mid.get("ys")
        act = moe.silu_mul_quant(h1, h1s, r, [moe.ACT_FP16] * len(qcfg))  # the kernel's activations, one segment per expert
        torch.cuda.synchronize()
        gathered = h.cpu()[r.perm_token.cpu().long()]
        stages = ((mid["a1"], layer.w1, layer.tag1, h1, h1s, lambda s: gathered[s], h.cpu()),
                  (mid["a2"], layer.w2, layer.tag2, mid["y"], ys, None, None))
        for a, ws, tags, c, cs, routed_in, shared_in in stages:
            for e, s in enumerate(a.segs):
                if not s.rows:
                    continue
                sl = slice(s.first_slot, s.first_slot + s.rows)
                x = act.A(e).cpu() if routed_in is None else shared_in if e == E else routed_in(sl)
                got = cs if e == E else c[sl]
                if routed_in is None:  # the activation pass read the right rows and halves of h1, in slot order
                    assert_act_close(x.numpy(), (h1s if e == E else h1[sl]).cpu().numpy(), None, "silu", {})
                if tags[e] == moe.ACT_MXFP6:
                    _check_seg(a, e, x, f"rep {rep}")
                    assert _within_bound(got, _deq(a.A(e), a.scale(e), ws[e].K), _deq(ws[e].B, ws[e].scale_b, ws[e].K), ws[e].K), e
                elif tags[e] == moe.ACT_FP16:
                    assert_f16_close(got.cpu().numpy(), x.double().numpy() @ ws[e].B.cpu().double().numpy().T, ws[e].K)
        want = moe_ref.combine(mid["y"].cpu().numpy(), r.inv_slot.cpu().numpy(), wts.cpu().numpy(), topk,
                               ys.cpu().numpy() if sh else None)
        assert (out.cpu().numpy().view(np.uint16) == want.view(np.uint16)).all() and torch.isfinite(out.float()).all()
        assert torch.equal(moe.PlannedForward(layer, h, ids, wts)(), out)
        assert torch.equal(gf.launch(h, ids, wts), out), rep
    assert gf.status() == 0
