"""GPU tests of the decode forward for gpt-oss layers (moe.DecodeForwardEx; mxmoe_moe_decode_gate_up_ex /
mxmoe_moe_decode_down_ex, DESIGN.md §4 "Decode forward: gpt-oss layers"): w4a16_g32_sym_MXFP4 experts, gate_up and down
biases and the clamped SwiGLU in a layer call of 1..16 tokens without a planner, against the eager layer
(MoEFFN.forward / MoEBlock.forward).

The MXFP4 dot products are f32 sums in the kernel's own order: bit for bit where the data make every partial sum exact,
within the project's fp16 tolerance on random data. The integer kinds stay bit-exact with biases and the clamp, since
every step is the eager arithmetic. The eager intermediates are in slot order (sorted by expert), the decode buffers in
pair order: row p of ``act`` / ``y`` is row inv_slot[p] of the eager one."""
from __future__ import annotations

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe, quantize
from mxmoe_amd.groupgemm import FP16, W4A4, W4A16_MXFP4, W8A8
from tests._decode_util import DEV, GUARD, biases, bits, check_stages, down_raw, f16_weights, guard, hidden, mx_codes, routing
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
MX = W4A16_MXFP4
INT_QCFG = [(W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8)]


def _mx_weight(g, rows, K, lo=126, hi=128):
    codes, scales = mx_codes(g, rows, K, lo, hi)
    return moe.prepare_weight_mx(codes.to(DEV), scales.to(DEV), MX)


def _gptoss(g, E, H, N):
    """a synthetic gpt-oss layer: random codes, scale bytes in [118, 126], biases in +-0.5"""
    u8 = lambda *shape, lo=0, hi=256: torch.randint(lo, hi, shape, generator=g, dtype=torch.uint8)
    parts = (u8(E, 2 * N, H // 32, 16), u8(E, 2 * N, H // 32, lo=118, hi=127), torch.rand(E, 2 * N, generator=g) - 0.5,
             u8(E, H, N // 32, 16), u8(E, H, N // 32, lo=118, hi=127), torch.rand(E, H, generator=g) - 0.5)
    return moe.gptoss_layer(*(t.to(DEV) for t in parts))


EXACT_CASES = [(384, "interleaved", 7), (384, "plain", 1), (384, "bias_clamp", 16), (640, "interleaved", 16),
               (640, "plain", 7), (640, "bias_clamp", 1)]


@pytest.mark.parametrize("H,variant,T", EXACT_CASES)
def test_mx_gate_up_exact(H, variant, T):
    """★ 4. MXFP4 gate_up on exact data: hidden multiples of 1/8 in [-2, 2], random codes, scale bytes 126..128, so
    every product is a multiple of 1/32 below 24 and a sum of 640 stays below 2^24 / 32: every f32 partial sum is exact
    in any order. H = 384: a weight row of 192 bytes, less than one 256-byte step; H = 640: the row ends inside the
    second step. N = 384, Ns = 640. act and act_shared equal the eager layer's fp16 activation rows bit for bit, with
    both gate_up layouts (no bias, SiLU) and with biases and the clamped SwiGLU (plain layout)."""
    topk, E, N, Ns = 2, 4, 384, 640
    g = torch.Generator().manual_seed(500 + H + T)
    gate_up = [_mx_weight(g, 2 * n, H) for n in [N] * E + [Ns]]
    down = [_mx_weight(g, H, n) for n in [N] * E + [Ns]]
    kw = {}
    if variant == "bias_clamp":
        b1, b2 = biases(g, E, H, N, Ns)
        kw = dict(gate_up_bias=b1, down_bias=b2, activation=moe.SwigluClamp())
    elif variant == "interleaved":
        # the same weights as fp16 tensors (exact: scale bytes 126..128), which MoEFFN interleaves and quantises again
        # (exact too: every value is an e2m1 value times the power of two its block's amax selects)
        deq = lambda w: quantize.dequant_mxfp4(w.B.cpu(), quantize.unpack_mxfp4_scales(w.scale_b.cpu(), w.K)).half().to(DEV)
        gate_up, down = [deq(w) for w in gate_up], [deq(w) for w in down]
        kw = dict(fuse_silu=True)
    ffn = moe.MoEFFN(gate_up, down, [(MX, MX)] * (E + 1), num_routed=E, **kw)
    df = moe.DecodeForwardEx(ffn, T, topk)
    assert df.layout == (nat.DECODE_GU_INTERLEAVED if variant == "interleaved" else nat.DECODE_GU_PLAIN)
    assert df.mask1 == df.mask2 == 1 << nat.DECODE_W4A16_MX and (df._glu is not None) == (variant == "bias_clamp")
    bufs = guard(df)
    for _ in range(2):
        ids, wts, sw = routing(g, T, E, topk)
        check_stages(df, ffn, hidden(g, T, H, grid=True), ids, wts, sw, stages=("act",))
    for t in bufs:
        assert not (bits(t) == GUARD).all(dim=1).any()
    assert df.status() == 0


@pytest.mark.parametrize("T", [1, 7, 16])
def test_mx_down_scale_ladder(T):
    """★ 5. mxmoe_moe_decode_down_ex alone: act multiples of 1/8 in [-2, 2], one scale byte per weight row cycling
    through 104..140, against fp16(float64 sum) of quantize.dequant_mxfp4's weights — the check that does not go through
    the GroupGEMM. With one scale per row every partial sum is an exact multiple of 2^(byte - 127) / 16 below 2^24
    steps, so the f32 sum is exact in any order, and overflow to +-inf happens on both sides. N = 384 and Ns = 640: the
    rows end inside a step."""
    topk, E, H, N, Ns = 2, 4, 128, 384, 640
    g = torch.Generator().manual_seed(520 + T)
    ladder = (104 + torch.arange(H) % 37).to(torch.uint8)
    ws, tables = [], (nat.MoeDecodeExpertC * (E + 1))()
    for e, K in enumerate([N] * E + [Ns]):
        codes, _ = mx_codes(g, H, K, 127, 127)
        scales = ladder.roll(e)[:, None].expand(H, K // 32).contiguous()
        w = moe.prepare_weight_mx(codes.to(DEV), scales.to(DEV), MX, warn=False)
        ws.append((w, quantize.dequant_mxfp4(codes, scales)))
        tables[e].b1, tables[e].sb1, tables[e].kind1 = w.B.data_ptr(), w.scale_b.data_ptr(), nat.DECODE_W4A16_MX
        tables[e].b2, tables[e].sb2, tables[e].kind2 = w.B.data_ptr(), w.scale_b.data_ptr(), nat.DECODE_W4A16_MX
    experts = torch.frombuffer(bytearray(bytes(tables)), dtype=torch.uint8).to(DEV)
    ids, _, _ = routing(g, T, E, topk)
    act, act_s = hidden(g, T * topk, N, grid=True), hidden(g, T, Ns, grid=True)
    y = torch.empty(T * topk, H, dtype=torch.float16, device=DEV)
    ys = torch.empty(T, H, dtype=torch.float16, device=DEV)
    bits(y).fill_(GUARD), bits(ys).fill_(GUARD)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    down_raw("ex", T, topk, E, 1, ids, experts, 1 << nat.DECODE_W4A16_MX, H, N, Ns, act, act_s, y, ys, status)
    torch.cuda.synchronize()
    flat = ids.view(-1).cpu().tolist()
    want = torch.stack([act[p].cpu().double() @ ws[e][1].T for p, e in enumerate(flat)]).float().half()
    want_s = (act_s.cpu().double() @ ws[E][1].T).float().half()
    # the ladder reaches both ends of fp16: overflow, and nonzero subnormals
    assert torch.isinf(want).any() and ((want != 0) & (want.abs() < 2.0 ** -14)).any()
    assert torch.equal(bits(y.cpu()), bits(want)) and torch.equal(bits(ys.cpu()), bits(want_s))
    assert int(status.item()) == 0


def _int_layer(g, E, H, N, Ns, biased, fuse=None):
    gate_up, down = f16_weights(g, E, H, N, Ns)
    kw = {}
    if biased:
        b1, b2 = biases(g, E, H, N, Ns)
        kw = dict(gate_up_bias=b1, down_bias=b2, activation=moe.SwigluClamp())
    return moe.MoEFFN(gate_up, down, INT_QCFG, num_routed=E, fuse_silu=fuse, **kw), (gate_up, down)


@pytest.mark.parametrize("T", [1, 7, 16])
def test_int_kinds_with_bias_and_clamp(T):
    """★ 6. A w8a8 / w4a4 layer with all four biases and the clamped SwiGLU on random data: act, y and out equal the
    eager layer's bit for bit (every step is the eager arithmetic). The same weights with "silu" and no bias: the
    buffers equal DecodeForward's bit for bit, in both gate_up layouts."""
    topk, E, H, N, Ns = 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(540 + T)
    ffn, (gate_up, down) = _int_layer(g, E, H, N, Ns, biased=True)
    df = moe.DecodeForwardEx(ffn, T, topk)
    assert df._glu is not None and ffn.b1 is not None and ffn.b1s is not None and ffn.b2 is not None and ffn.b2s is not None
    guard(df)
    for _ in range(2):
        ids, wts, sw = routing(g, T, E, topk)
        h = hidden(g, T, H)
        check_stages(df, ffn, h, ids, wts, sw)
        check_stages(df, ffn, h, ids, wts, None)
    assert df.status() == 0
    for fuse in (None, False):
        plain = moe.MoEFFN(gate_up, down, INT_QCFG, num_routed=E, fuse_silu=fuse)
        new, old = moe.DecodeForwardEx(plain, T, topk), moe.DecodeForward(plain, T, topk)
        assert new._glu is None and new.layout == old.layout
        new.launch(h, ids, wts, sw), old.launch(h, ids, wts, sw)
        torch.cuda.synchronize()
        for a, b in ((new.act, old.act), (new.act_shared, old.act_shared), (new.y, old.y), (new.ys, old.ys), (new.out, old.out)):
            assert torch.equal(bits(a), bits(b))
        assert new.status() == 0 == old.status()


@pytest.fixture(scope="module")
def oss_small():
    return _gptoss(torch.Generator().manual_seed(560), 4, 384, 384)


@pytest.mark.parametrize("T", [1, 7, 16])
def test_gptoss_layer_random_data(oss_small, T):
    """★ 7. A gptoss_layer (random codes, scale bytes in [118, 126], biases in +-0.5; H = N = 384) on random hidden
    states: out within the project's fp16 tolerance of the eager layer's (the f32 summation orders differ)."""
    ffn, topk = oss_small, 2
    g = torch.Generator().manual_seed(561 + T)
    df = moe.DecodeForwardEx(ffn, T, topk)
    guard(df)
    for _ in range(2):
        ids, wts, _ = routing(g, T, ffn.E, topk)
        check_stages(df, ffn, hidden(g, T, ffn.H), ids, wts, None, stages=("close",))
    assert df.status() == 0


def test_gptoss_width_rereads_the_weights():
    """★ 7. H = N = 2880 -> 2944 (the gpt-oss width: fp16 rows of 5888 -> 6144 bytes, 10 rows per batch in the 60 KB
    budget), T = 16, topk = 1 and every id = 1: 16 rows on one expert, so the second batch re-reads the weights."""
    T, E, topk = 16, 2, 1
    g = torch.Generator().manual_seed(570)
    ffn = _gptoss(g, E, 2880, 2880)
    assert (ffn.H, ffn.N) == (2944, 2944)
    df = moe.DecodeForwardEx(ffn, T, topk)
    guard(df)
    ids, wts, _ = routing(g, T, E, topk)
    ids.fill_(1)
    h = moe.pad_cols(torch.randn(T, 2880, generator=g).half(), ffn.H).to(DEV)
    mid = check_stages(df, ffn, h, ids, wts, None, stages=("close",))
    assert mid["routing"].counts == [0, 16]
    assert df.status() == 0


def test_mixed_kinds_in_one_call():
    """★ 7. MXFP4, w8a8 and fp16 linears in one call: the LDS rows are sized by the fp16 rows of the MXFP4 kind and the
    integer kinds' quantised rows lie in them. An MXFP4 gate_up feeds an MXFP4 or fp16 down (on random data a last-bit
    difference in act could move an integer code), the w8a8 gate_ups feed either."""
    T, topk, E, H, N, Ns = 16, 2, 4, 384, 384, 640
    g = torch.Generator().manual_seed(580)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    qcfg = [(MX, MX), (W8A8, W8A8), (W8A8, MX), (MX, FP16), (W8A8, W8A8)]
    b1, b2 = biases(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=False, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    df = moe.DecodeForwardEx(ffn, T, topk)
    assert df.mask1 == 0b1010 and df.mask2 == 0b1011
    guard(df)
    for _ in range(2):
        ids, wts, sw = routing(g, T, E, topk)
        check_stages(df, ffn, hidden(g, T, H), ids, wts, sw, stages=("close",))
    assert df.status() == 0


def test_bf16_ends():
    """★ 8. A block with a bf16 router over MXFP4 gate_ups (exact data, as in test_mx_gate_up_exact) and w8a8 downs, with
    biases and the clamp: every stage is exact or integer, so out equals the bf16 block.forward bit for bit, and y
    equals the fp16 layer's y on hidden.to(torch.float16) — the row is converted as it is loaded."""
    T, topk, E, H, N, Ns = 16, 2, 4, 384, 384, 640
    g = torch.Generator().manual_seed(590)
    _, down = f16_weights(g, E, H, N, Ns)
    gate_up = [_mx_weight(g, 2 * n, H) for n in [N] * E + [Ns]]
    b1, b2 = biases(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, [(MX, W8A8)] * (E + 1), num_routed=E, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    bf = torch.bfloat16
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(bf).to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(bf).to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=w_sg)
    df = moe.DecodeForwardEx(block, T, dtype=bf)
    assert df.out.dtype == bf
    h = hidden(g, T, H, grid=True, dtype=bf)
    got = df.launch(h).clone()
    want, mid = block.forward(h, return_intermediates=True)
    torch.cuda.synchronize()
    assert torch.equal(df.gate_out[0], mid["topk_ids"])
    assert got.dtype == bf and torch.equal(bits(got), bits(want))
    df16 = moe.DecodeForwardEx(ffn, T, topk)
    df16.launch(h.to(torch.float16), mid["topk_ids"], mid["topk_weights"], mid["shared_w"])
    torch.cuda.synchronize()
    assert torch.equal(bits(df.y), bits(df16.y)) and torch.equal(bits(df.ys), bits(df16.ys))
    assert torch.equal(bits(df.y), bits(mid["y"][mid["routing"].inv_slot.long()]))
    assert df.status() == 0
    with pytest.raises(ValueError):
        df.launch(h.to(torch.float16))
    with pytest.raises(ValueError):
        moe.DecodeForwardEx(block, T, dtype=torch.float16)


def test_block_under_a_graph():
    """★ 9. A gpt-oss MoEBlock (E = 32, topk = 4, a router logit bias, gptoss_layer at H = N = 384) captured once —
    router, both decode kernels, the bias combine — and replayed on two hidden states: each replay equals the
    uncaptured launch bit for bit."""
    T, E, topk, H = 7, 32, 4, 384
    g = torch.Generator().manual_seed(600)
    ffn = _gptoss(g, E, H, H)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, logit_bias=(torch.randn(E, generator=g) * 0.5).to(DEV))
    df, ref = moe.DecodeForwardEx(block, T), moe.DecodeForwardEx(block, T)
    hiddens = [hidden(g, T, H) for _ in range(2)]
    static_hidden = hiddens[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.launch(static_hidden)  # warm-up outside the capture (module loading)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        df.launch(static_hidden)
    torch.cuda.current_stream().wait_stream(side)
    seen = []
    for h in hiddens:
        static_hidden.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        want = ref.launch(h).clone()
        torch.cuda.synchronize()
        assert torch.equal(df.gate_out[0], ref.gate_out[0])
        for a, b in ((df.act, ref.act), (df.y, ref.y), (df.out, want)):
            assert torch.equal(bits(a), bits(b))
        seen.append(df.gate_out[0].clone())
    assert not torch.equal(seen[0], seen[1])  # two routings
    eager = block.forward(hiddens[1])
    torch.cuda.synchronize()
    assert_f16_close(df.out.float().cpu().numpy(), eager.float().cpu().numpy(), H)
    assert df.status() == 0 == ref.status()


def test_bad_ids_and_short_calls_keep_their_guard(oss_small):
    """★ 10. Capacity 16, a call of 7 tokens with an id of E and an id of -1 among valid ones, biases present: those
    pairs' act / y rows and every row past the call keep the guard pattern, status() is DECODE_BAD_ID, and out is
    finite for the tokens whose ids are valid (the bias combine adds no bias for an id outside [0, E))."""
    ffn, cap, T, topk = oss_small, 16, 7, 2
    g = torch.Generator().manual_seed(610)
    df = moe.DecodeForwardEx(ffn, cap, topk)
    guard(df)
    ids, wts, _ = routing(g, T, ffn.E, topk)
    ids[2, 0], ids[5, 1] = ffn.E, -1
    bad = [2 * topk + 0, 5 * topk + 1]
    out = df.launch(hidden(g, T, ffn.H), ids, wts, None)
    torch.cuda.synchronize()
    good = [p for p in range(T * topk) if p not in bad]
    for t in (df.act, df.y):
        assert (bits(t[bad]) == GUARD).all() and (bits(t[T * topk:]) == GUARD).all()
        assert not (bits(t[good]) == GUARD).all(dim=1).any()
    assert (bits(df.out[T:]) == GUARD).all() and out.shape[0] == T
    assert torch.isfinite(out[[t for t in range(T) if t not in (2, 5)]].float()).all()
    assert df.status(reset=True) == nat.DECODE_BAD_ID and df.status() == 0
