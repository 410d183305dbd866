"""GPU tests of the decode forward for gpt-oss layers (moe.DecodeForwardEx; mxmoe_moe_decode_gate_up_ex /
mxmoe_moe_decode_down_ex, DESIGN.md §4 "Decode forward: gpt-oss layers"): w4a16_g32_sym_MXFP4 experts, gate_up and down
biases and the clamped SwiGLU in a layer call of 1..16 tokens without a planner, against the eager layer
(MoEFFN.forward / MoEBlock.forward).

The MXFP4 dot products are f32 sums in the kernel's own order: bit for bit where the data make every partial sum exact,
within the project's fp16 tolerance on random data. The integer kinds stay bit-exact with biases and the clamp, since
every step is the eager arithmetic. The eager intermediates are in slot order (sorted by expert), the decode buffers in
pair order: row p of ``act`` / ``y`` is row inv_slot[p] of the eager one."""
from __future__ import annotations

import ctypes

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe, quantize
from mxmoe_amd.groupgemm import FP16, W4A4, W4A16_MXFP4, W8A8
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7B7B
MX = W4A16_MXFP4
INT_QCFG = [(W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8)]


def _bits(t):
    return t.view(torch.int16)


def _guard(df):
    bufs = [t for t in (df.act, df.act_shared, df.y, df.ys, df.out) if t is not None]
    for t in bufs:
        _bits(t).fill_(GUARD)
    return bufs


def _hidden(g, T, H, grid=False, dtype=torch.float16):
    if grid:  # multiples of 1/8 in [-2, 2] (exact in bf16 too)
        return (torch.randint(-16, 17, (T, H), generator=g).float() / 8).to(dtype).to(DEV)
    return torch.randn(T, H, generator=g).to(dtype).to(DEV)


def _routing(g, T, E, topk):
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
    sw = torch.rand(T, generator=g).to(DEV)
    return ids, wts, sw


def _mx_codes(g, rows, K, lo, hi):
    """random e2m1 codes [rows, K/2] and e8m0 scale bytes [rows, K/32] in [lo, hi] (host)"""
    return (torch.randint(0, 256, (rows, K // 2), generator=g, dtype=torch.uint8),
            torch.randint(lo, hi + 1, (rows, K // 32), generator=g, dtype=torch.uint8))


def _mx_weight(g, rows, K, lo=126, hi=128):
    codes, scales = _mx_codes(g, rows, K, lo, hi)
    return moe.prepare_weight_mx(codes.to(DEV), scales.to(DEV), MX)


def _f16_weights(g, E, H, N, Ns):
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)
    return [mk(2 * N, H) for _ in range(E)] + ([mk(2 * Ns, H)] if Ns else []), \
        [mk(H, N) for _ in range(E)] + ([mk(H, Ns)] if Ns else [])


def _biases(g, E, H, N, Ns):
    """gate_up and down bias rows in +-0.5, the shared expert's last"""
    mk = lambda n: (torch.rand(n, generator=g) - 0.5).half().to(DEV)
    return [mk(2 * N) for _ in range(E)] + ([mk(2 * Ns)] if Ns else []), [mk(H) for _ in range(E + (1 if Ns else 0))]


def _gptoss(g, E, H, N):
    """a synthetic gpt-oss layer: random codes, scale bytes in [118, 126], biases in +-0.5"""
    u8 = lambda *shape, lo=0, hi=256: torch.randint(lo, hi, shape, generator=g, dtype=torch.uint8)
    parts = (u8(E, 2 * N, H // 32, 16), u8(E, 2 * N, H // 32, lo=118, hi=127), torch.rand(E, 2 * N, generator=g) - 0.5,
             u8(E, H, N // 32, 16), u8(E, H, N // 32, lo=118, hi=127), torch.rand(E, H, generator=g) - 0.5)
    return moe.gptoss_layer(*(t.to(DEV) for t in parts))


def _eager_act(ffn, mid):
    """The eager layer's fp16 activation rows (routed in slot order, shared): its own activation pass run with fp16
    tags on its gate_up output — for a layer whose down tags are fp16, the rows it fed to the down GroupGEMM."""
    r, tags = mid["routing"], [moe.ACT_FP16] * (ffn.E + (1 if ffn.has_shared else 0))
    if mid["h1"].shape[1] == ffn.N:  # the SiLU epilogue ran: h1 is act
        return mid["h1"], mid["h1s"]
    if ffn.biased_or_gated:
        a = moe.glu_quant(mid["h1"], mid["h1s"], r, tags, ffn.activation, ffn.b1, ffn.b1s)
    else:
        a = moe.silu_mul_quant(mid["h1"], mid["h1s"], r, tags, interleaved=ffn.gate_up_layout() != "plain")
    torch.cuda.synchronize()
    return torch.cat([a.A(e) for e in range(ffn.E)]), a.A(ffn.E) if ffn.has_shared else None


def _check_stages(df, ffn, h, ids, wts, sw, stages=("act", "y", "out")):
    """One call through ``df`` against the eager layer: the stages "act", "y", "out" bit for bit, "close": out within the
    project's fp16 tolerance."""
    T, topk = ids.shape
    n = T * topk
    got = df.launch(h, ids, wts, sw).clone()
    want, mid = ffn.forward(h, ids, wts, sw, return_intermediates=True)
    torch.cuda.synchronize()
    inv = mid["routing"].inv_slot.long()
    if "act" in stages:
        act, act_s = _eager_act(ffn, mid)
        assert torch.equal(_bits(df.act[:n]), _bits(act[inv])), "gate_up (routed act)"
        if ffn.has_shared:
            assert torch.equal(_bits(df.act_shared[:T]), _bits(act_s)), "gate_up (shared act)"
    if "y" in stages:
        assert torch.equal(_bits(df.y[:n]), _bits(mid["y"][inv])), "down (routed y)"
        if ffn.has_shared:
            assert torch.equal(_bits(df.ys[:T]), _bits(mid["ys"])), "down (shared ys)"
    if "out" in stages:
        assert torch.equal(_bits(got), _bits(want)), "combine"
    if "close" in stages:
        assert_f16_close(got.float().cpu().numpy(), want.float().cpu().numpy(), ffn.H)
    return mid


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
        b1, b2 = _biases(g, E, H, N, Ns)
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
    bufs = _guard(df)
    for _ in range(2):
        ids, wts, sw = _routing(g, T, E, topk)
        _check_stages(df, ffn, _hidden(g, T, H, grid=True), ids, wts, sw, stages=("act",))
    for t in bufs:
        assert not (_bits(t) == GUARD).all(dim=1).any()
    assert df.status() == 0


def _down_ex(T, topk, E, shared, ids, experts, mask, H, N, Ns, act, act_shared, y, ys, status):
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    nat.check(nat.symbol("mxmoe_moe_decode_down_ex")(T, topk, E, shared, p(ids), p(experts), mask, H, N, Ns, p(act),
                                                    p(act_shared), p(y), p(ys), p(status), None))


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
        codes, _ = _mx_codes(g, H, K, 127, 127)
        scales = ladder.roll(e)[:, None].expand(H, K // 32).contiguous()
        w = moe.prepare_weight_mx(codes.to(DEV), scales.to(DEV), MX, warn=False)
        ws.append((w, quantize.dequant_mxfp4(codes, scales)))
        tables[e].b1, tables[e].sb1, tables[e].kind1 = w.B.data_ptr(), w.scale_b.data_ptr(), nat.DECODE_W4A16_MX
        tables[e].b2, tables[e].sb2, tables[e].kind2 = w.B.data_ptr(), w.scale_b.data_ptr(), nat.DECODE_W4A16_MX
    experts = torch.frombuffer(bytearray(bytes(tables)), dtype=torch.uint8).to(DEV)
    ids, _, _ = _routing(g, T, E, topk)
    act, act_s = _hidden(g, T * topk, N, grid=True), _hidden(g, T, Ns, grid=True)
    y = torch.empty(T * topk, H, dtype=torch.float16, device=DEV)
    ys = torch.empty(T, H, dtype=torch.float16, device=DEV)
    _bits(y).fill_(GUARD), _bits(ys).fill_(GUARD)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    _down_ex(T, topk, E, 1, ids, experts, 1 << nat.DECODE_W4A16_MX, H, N, Ns, act, act_s, y, ys, status)
    torch.cuda.synchronize()
    flat = ids.view(-1).cpu().tolist()
    want = torch.stack([act[p].cpu().double() @ ws[e][1].T for p, e in enumerate(flat)]).float().half()
    want_s = (act_s.cpu().double() @ ws[E][1].T).float().half()
    # the ladder reaches both ends of fp16: overflow, and nonzero subnormals
    assert torch.isinf(want).any() and ((want != 0) & (want.abs() < 2.0 ** -14)).any()
    assert torch.equal(_bits(y.cpu()), _bits(want)) and torch.equal(_bits(ys.cpu()), _bits(want_s))
    assert int(status.item()) == 0


def _int_layer(g, E, H, N, Ns, biased, fuse=None):
    gate_up, down = _f16_weights(g, E, H, N, Ns)
    kw = {}
    if biased:
        b1, b2 = _biases(g, E, H, N, Ns)
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
    _guard(df)
    for _ in range(2):
        ids, wts, sw = _routing(g, T, E, topk)
        h = _hidden(g, T, H)
        _check_stages(df, ffn, h, ids, wts, sw)
        _check_stages(df, ffn, h, ids, wts, None)
    assert df.status() == 0
    for fuse in (None, False):
        plain = moe.MoEFFN(gate_up, down, INT_QCFG, num_routed=E, fuse_silu=fuse)
        new, old = moe.DecodeForwardEx(plain, T, topk), moe.DecodeForward(plain, T, topk)
        assert new._glu is None and new.layout == old.layout
        new.launch(h, ids, wts, sw), old.launch(h, ids, wts, sw)
        torch.cuda.synchronize()
        for a, b in ((new.act, old.act), (new.act_shared, old.act_shared), (new.y, old.y), (new.ys, old.ys), (new.out, old.out)):
            assert torch.equal(_bits(a), _bits(b))
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
    _guard(df)
    for _ in range(2):
        ids, wts, _ = _routing(g, T, ffn.E, topk)
        _check_stages(df, ffn, _hidden(g, T, ffn.H), ids, wts, None, stages=("close",))
    assert df.status() == 0


def test_gptoss_width_rereads_the_weights():
    """★ 7. H = N = 2880 -> 2944 (the gpt-oss width: fp16 rows of 5888 -> 6144 bytes, 10 rows per batch in the 60 KB
    budget), T = 16, topk = 1 and every id = 1: 16 rows on one expert, so the second batch re-reads the weights."""
    T, E, topk = 16, 2, 1
    g = torch.Generator().manual_seed(570)
    ffn = _gptoss(g, E, 2880, 2880)
    assert (ffn.H, ffn.N) == (2944, 2944)
    df = moe.DecodeForwardEx(ffn, T, topk)
    _guard(df)
    ids, wts, _ = _routing(g, T, E, topk)
    ids.fill_(1)
    h = moe.pad_cols(torch.randn(T, 2880, generator=g).half(), ffn.H).to(DEV)
    mid = _check_stages(df, ffn, h, ids, wts, None, stages=("close",))
    assert mid["routing"].counts == [0, 16]
    assert df.status() == 0


def test_mixed_kinds_in_one_call():
    """★ 7. MXFP4, w8a8 and fp16 linears in one call: the LDS rows are sized by the fp16 rows of the MXFP4 kind and the
    integer kinds' quantised rows lie in them. An MXFP4 gate_up feeds an MXFP4 or fp16 down (on random data a last-bit
    difference in act could move an integer code), the w8a8 gate_ups feed either."""
    T, topk, E, H, N, Ns = 16, 2, 4, 384, 384, 640
    g = torch.Generator().manual_seed(580)
    gate_up, down = _f16_weights(g, E, H, N, Ns)
    qcfg = [(MX, MX), (W8A8, W8A8), (W8A8, MX), (MX, FP16), (W8A8, W8A8)]
    b1, b2 = _biases(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=False, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    df = moe.DecodeForwardEx(ffn, T, topk)
    assert df.mask1 == 0b1010 and df.mask2 == 0b1011
    _guard(df)
    for _ in range(2):
        ids, wts, sw = _routing(g, T, E, topk)
        _check_stages(df, ffn, _hidden(g, T, H), ids, wts, sw, stages=("close",))
    assert df.status() == 0


def test_bf16_ends():
    """★ 8. A block with a bf16 router over MXFP4 gate_ups (exact data, as in test_mx_gate_up_exact) and w8a8 downs, with
    biases and the clamp: every stage is exact or integer, so out equals the bf16 block.forward bit for bit, and y
    equals the fp16 layer's y on hidden.to(torch.float16) — the row is converted as it is loaded."""
    T, topk, E, H, N, Ns = 16, 2, 4, 384, 384, 640
    g = torch.Generator().manual_seed(590)
    _, down = _f16_weights(g, E, H, N, Ns)
    gate_up = [_mx_weight(g, 2 * n, H) for n in [N] * E + [Ns]]
    b1, b2 = _biases(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, [(MX, W8A8)] * (E + 1), num_routed=E, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    bf = torch.bfloat16
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(bf).to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(bf).to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=w_sg)
    df = moe.DecodeForwardEx(block, T, dtype=bf)
    assert df.out.dtype == bf
    h = _hidden(g, T, H, grid=True, dtype=bf)
    got = df.launch(h).clone()
    want, mid = block.forward(h, return_intermediates=True)
    torch.cuda.synchronize()
    assert torch.equal(df.gate_out[0], mid["topk_ids"])
    assert got.dtype == bf and torch.equal(_bits(got), _bits(want))
    df16 = moe.DecodeForwardEx(ffn, T, topk)
    df16.launch(h.to(torch.float16), mid["topk_ids"], mid["topk_weights"], mid["shared_w"])
    torch.cuda.synchronize()
    assert torch.equal(_bits(df.y), _bits(df16.y)) and torch.equal(_bits(df.ys), _bits(df16.ys))
    assert torch.equal(_bits(df.y), _bits(mid["y"][mid["routing"].inv_slot.long()]))
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
    hiddens = [_hidden(g, T, H) for _ in range(2)]
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
            assert torch.equal(_bits(a), _bits(b))
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
    _guard(df)
    ids, wts, _ = _routing(g, T, ffn.E, topk)
    ids[2, 0], ids[5, 1] = ffn.E, -1
    bad = [2 * topk + 0, 5 * topk + 1]
    out = df.launch(_hidden(g, T, ffn.H), ids, wts, None)
    torch.cuda.synchronize()
    good = [p for p in range(T * topk) if p not in bad]
    for t in (df.act, df.y):
        assert (_bits(t[bad]) == GUARD).all() and (_bits(t[T * topk:]) == GUARD).all()
        assert not (_bits(t[good]) == GUARD).all(dim=1).any()
    assert (_bits(df.out[T:]) == GUARD).all() and out.shape[0] == T
    assert torch.isfinite(out[[t for t in range(T) if t not in (2, 5)]].float()).all()
    assert df.status(reset=True) == nat.DECODE_BAD_ID and df.status() == 0
