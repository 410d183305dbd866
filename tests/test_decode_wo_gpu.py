"""GPU tests of the decode forward with integer weight-only experts (moe.DecodeForwardWo; mxmoe_moe_decode_gate_up_wo /
mxmoe_moe_decode_down_wo, DESIGN.md §4 "Decode forward: weight-only experts"): w4a16 and w8a16 experts, per-channel or
g128, sym or asym, in a layer call of 1..16 tokens without a planner, against quantize.dequant_weightonly (the
dequantised weights, bit for bit) and the eager layer (MoEFFN.forward / MoEBlock.forward).

The weight-only dot products are f32 sums in the kernel's own order: bit for bit where the data make every partial sum
exact, within the project's fp16 tolerance on random data. The eager intermediates are in slot order (sorted by
expert), the decode buffers in pair order: row p of ``act`` / ``y`` is row inv_slot[p] of the eager one."""
from __future__ import annotations

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe, quantize
from mxmoe_amd.groupgemm import FP16, W4A4, W4A16_ASYM, W4A16_G128_SYM, W8A8, W8A16_ASYM, QParams
from tests._decode_util import DEV, GUARD, biases, bits, check_stages, down_raw, f16_weights, guard, routing
from tests._decode_util import hidden as _hidden
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
W8A16_G128_ASYM = QParams(16, 8, 128, False)
EXACT_KINDS = {"w4a16_g-1_asym": W4A16_ASYM, "w4a16_g128_sym": W4A16_G128_SYM, "w8a16_g-1_asym": W8A16_ASYM,
               "w8a16_g128_asym": W8A16_G128_ASYM}
SCHEME = [(W4A16_ASYM, W8A8), (W8A8, W8A8), (W8A8, W4A16_ASYM), (W4A16_ASYM, W4A16_ASYM), (W8A8, W8A8),
          (W4A16_ASYM, W4A16_ASYM)]  # E = 5 and the shared expert


def hidden(g, T, H, grid=False, dtype=torch.float16):
    """randn, or (grid) multiples of 1/4 in [-1, 1] (exact in bf16 too)"""
    return _hidden(g, T, H, grid, dtype, step=4, bound=1)


# ---- 1. the dequantised weights, read back bit for bit ------------------------------------------------------------

def _finite_f16(g, shape, max_exp):
    """fp16 values from random bit patterns, both signs, subnormals and zeros included, |v| < 2^(max_exp - 14)"""
    bits = torch.randint(0, max_exp << 10, shape, generator=g, dtype=torch.int32)
    bits |= torch.randint(0, 2, shape, generator=g, dtype=torch.int32) << 15
    return bits.to(torch.int16).view(torch.float16)


@pytest.mark.parametrize("kind", range(4, 12))
def test_dequant_readback(kind):
    """mxmoe_moe_decode_down_wo alone on one expert, T = 16, topk = 1, H = N = 384: row t of act in call c is 1.0 at K
    position 16 c + t and zero elsewhere, so y[t][h] is fp16(b[h][16 c + t]) — the one nonzero term on a +0
    accumulator (a -0 weight reads back as +0) — against quantize.dequant_weightonly, for every code position, every
    group and both row ends (192 bytes: less than a step; 384: one and a half). Codes cover every value; scales and
    zps are arbitrary finite fp16 values (|scale| < 64, |zp| < 1024, so every weight is finite), negative, subnormal
    and zero ones among them."""
    w_bits, gsize, sym = (8 if (kind - 4) & 1 else 4), (128 if (kind - 4) & 2 else -1), not (kind - 4) & 4
    assert nat.decode_wo_kind(w_bits, gsize, sym) == kind
    T, H, N = 16, 384, 384
    g = torch.Generator().manual_seed(700 + kind)
    G = 1 if gsize == -1 else N // gsize
    codes = torch.randint(0, 1 << w_bits, (H, N), generator=g, dtype=torch.uint8)
    codes[0, :1 << w_bits] = torch.arange(1 << w_bits, dtype=torch.uint8)[:N]  # every value, whatever the draw
    scale = _finite_f16(g, (G, H), 20)
    scale[:, 3], scale[:, 5], scale[:, 6] = 0.0, -(2.0 ** -20), 2.0 ** -24  # a zero and two subnormal scales, in any draw
    if sym:
        sz = scale.reshape(-1)
    else:
        zp = _finite_f16(g, (G, H), 24)
        zp[:, ::7] = 0
        sz = torch.stack([scale, zp], dim=-1).reshape(-1)
    want = quantize.dequant_weightonly(codes, sz, w_bits, gsize, sym)
    assert torch.isfinite(want).all() and (sz == 0).any() and ((sz != 0) & (sz.abs() < 2.0 ** -14)).any() and (sz < 0).any()
    want = (want.float() + 0.0).half()  # -0 -> +0
    B, SZ = quantize.pack_weightonly_mi355x(codes, w_bits).to(DEV), sz.to(DEV)
    rec = (nat.MoeDecodeExpertC * 1)()
    rec[0].b1, rec[0].sb1, rec[0].kind1 = B.data_ptr(), SZ.data_ptr(), kind
    rec[0].b2, rec[0].sb2, rec[0].kind2 = B.data_ptr(), SZ.data_ptr(), kind
    experts = torch.frombuffer(bytearray(bytes(rec)), dtype=torch.uint8).to(DEV)
    ids = torch.zeros(T, 1, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ys = []
    for c in range(N // T):
        act = torch.zeros(T, N, dtype=torch.float16, device=DEV)
        act[torch.arange(T), 16 * c + torch.arange(T)] = 1.0
        y = torch.empty(T, H, dtype=torch.float16, device=DEV)
        bits(y).fill_(GUARD)
        down_raw("wo", T, 1, 1, 0, ids, experts, 1 << kind, H, N, 0, act, None, y, None, status)
        ys.append(y)
    torch.cuda.synchronize()
    got = torch.cat(ys).cpu()  # row 16 c + t = K position: [N][H]
    assert torch.equal(bits(got), bits(want.t().contiguous()))
    assert int(status.item()) == 0


# ---- 2. exact sums: gate_up and down bit for bit against the eager layer --------------------------------------------

def _grid_weight(g, rows, K, q):
    """fp16 [rows, K] that quant_weightonly(q) reproduces exactly: b = (u - off + m) * s with s a power of two in
    2^-6 .. 2^-4 and zp = m * s an integer multiple of it per row and group, every group holding its smallest and its
    largest code. Returns (weight, max |b| / 2^-6)."""
    G = 1 if q.gsize == -1 else K // q.gsize
    top = (1 << q.w_bits) - (2 if q.sym else 1)  # sym codes are 0 .. 2 qmax
    off = (1 << (q.w_bits - 1)) - 1 if q.sym else 0
    u = torch.randint(0, top + 1, (rows, G, K // G), generator=g)
    u[..., 0], u[..., 1] = 0, top
    s = torch.randint(0, 3, (rows, G, 1), generator=g)  # the scale is 2^(s - 6)
    m = torch.zeros_like(s) if q.sym else -torch.randint(0, top // 2 + 1, (rows, G, 1), generator=g)
    units = (u - off + m) * 2 ** s  # b in units of 2^-6
    return (units.double() / 64).half().reshape(rows, K).to(DEV), int(units.abs().max())


def _exact_layer(g, q, E, H, N, Ns, variant):
    ws, bmax = [], 0
    for rows, K in [(2 * N, H)] * E + [(2 * Ns, H)] + [(H, N)] * E + [(H, Ns)]:
        w, b = _grid_weight(g, rows, K, q)
        ws.append(w)
        bmax = max(bmax, b)
    kw = dict(fuse_silu=variant == "interleaved")
    if variant == "bias_clamp":
        b1, b2 = biases(g, E, H, N, Ns)
        kw = dict(gate_up_bias=b1, down_bias=b2, activation=moe.SwigluClamp())
    ffn = moe.MoEFFN(ws[:E + 1], ws[E + 1:], [(q, q)] * (E + 1), num_routed=E, **kw)
    return ffn, bmax


SHAPES = [(384, 384, 640), (640, 384, 384)]
VARIANTS = ("interleaved", "plain", "bias_clamp")
# every kind with every layout, shape and T
EXACT_CASES = [(name, variant, shape, T) for name in EXACT_KINDS for variant in VARIANTS for shape in SHAPES for T in (1, 7, 16)]
# H = 2176: 4-bit rows of 1088 bytes (the four-steps-in-flight loop runs twice), 8-bit rows of 2176 (three times); both
# end inside a step and in the middle of a 128-K group of lanes. Every kind with every layout, T rotating.
EXACT_CASES += [(name, variant, (2176, 384, 384), (1, 7, 16)[(i + j) % 3])
                for i, name in enumerate(EXACT_KINDS) for j, variant in enumerate(VARIANTS)]


@pytest.mark.parametrize("name,variant,shape,T", EXACT_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_exact_gate_up_and_down(name, variant, shape, T):
    """Hidden states and activations multiples of 1/4 in [-1, 1], weights (u - off + m) * s with s a power of two in
    2^-6 .. 2^-4: every product is a multiple of 2^-8, and K * max|x| * max|b| in those units is asserted below 2^24
    before the GPU is touched, so every f32 partial sum is exact in any order. gate_up: act and act_shared of a layer
    call equal the eager layer's activation rows bit for bit (both layouts with SiLU, the plain one with biases and
    the clamped SwiGLU). down: the down entry on grid activations equals the eager layer's own down GroupGEMM on the
    same rows (its activation pass with the rows as they are, then ``down_call``) bit for bit."""
    q, (H, N, Ns), topk, E = EXACT_KINDS[name], shape, 2, 4
    g = torch.Generator().manual_seed(sum(map(ord, name + variant)) + H + T)
    ffn, bmax = _exact_layer(g, q, E, H, N, Ns, variant)
    assert max(H, N, Ns) * 4 * bmax < 2 ** 24  # K * (max|x| / (1/4)) * (max|b| / 2^-6)
    for w in ffn.w1 + ffn.w2:  # the quantiser found the grid: power-of-two scales within a factor of 4
        sc = w.scale_b.float().cpu() if q.sym else w.scale_b.float().cpu()[0::2]
        assert set(sc.tolist()) <= {2.0 ** -6, 2.0 ** -5, 2.0 ** -4}
    df = moe.DecodeForwardWo(ffn, T, topk)
    kind = nat.decode_wo_kind(q.w_bits, q.gsize, q.sym)
    assert df.mask1 == df.mask2 == 1 << kind and (df._glu is not None) == (variant == "bias_clamp")
    assert df.layout == (nat.DECODE_GU_INTERLEAVED if variant == "interleaved" else nat.DECODE_GU_PLAIN)
    bufs = guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    mid = check_stages(df, ffn, hidden(g, T, H, grid=True), ids, wts, sw, stages=("act",))
    for t in bufs:
        assert not (bits(t) == GUARD).all(dim=1).any()
    # down, on grid activations in pair order
    n, r = T * topk, mid["routing"]
    inv = r.inv_slot.long()
    act, act_s = hidden(g, n, N, grid=True), hidden(g, T, Ns, grid=True)
    slots = torch.empty_like(act)
    slots[inv] = act
    a2 = moe.silu_mul_quant(slots, act_s, r, ffn.tag2, activated=True)
    g2, y, ys = ffn.down_call(a2, T, topk, torch.device(DEV))
    g2.launch()
    bits(df.y).fill_(GUARD), bits(df.ys).fill_(GUARD)
    down_raw("wo", T, topk, E, 1, ids, df.experts, df.mask2, H, N, Ns, act, act_s, df.y, df.ys, df.dev_status)
    torch.cuda.synchronize()
    assert torch.equal(bits(df.y[:n]), bits(y[inv])), "down (routed y)"
    assert torch.equal(bits(df.ys[:T]), bits(ys)), "down (shared ys)"
    assert df.status() == 0


# ---- 3. the scheme on random data -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def scheme_layer():
    g = torch.Generator().manual_seed(720)
    gate_up, down = f16_weights(g, 5, 384, 256, 640)
    return moe.MoEFFN(gate_up, down, SCHEME, num_routed=5)


@pytest.mark.parametrize("T", [1, 7, 16])
def test_scheme_random_data(scheme_layer, T):
    """w4a16_g-1_asym and w8a8 mixed per expert and per linear, the shared expert weight-only (E = 5, H = 384, N = 256,
    Ns = 640), random data: out within the project's fp16 tolerance of the eager layer; the y rows of the experts that
    are w8a8 in both linears equal the eager layer's bit for bit (integer arithmetic from end to end)."""
    ffn, topk = scheme_layer, 2
    g = torch.Generator().manual_seed(721 + T)
    df = moe.DecodeForwardWo(ffn, T, topk)
    assert df.mask1 == df.mask2 == 1 << nat.DECODE_W8A8 | 1 << nat.DECODE_W4A16_ASYM
    assert df.layout == nat.DECODE_GU_INTERLEAVED
    guard(df)
    for _ in range(2):
        ids, wts, sw = routing(g, T, ffn.E, topk)
        mid = check_stages(df, ffn, hidden(g, T, ffn.H), ids, wts, sw, stages=("close",))
        inv = mid["routing"].inv_slot.long()
        w8 = torch.tensor([e in (1, 4) for e in ids.view(-1).tolist()])
        assert torch.equal(bits(df.y[:T * topk])[w8], bits(mid["y"][inv])[w8])
    assert df.status() == 0


def test_older_kinds_give_decode_forwards_bytes():
    """On an fp16 / w8a8 / w4a4 layer the _wo entries give DecodeForward's bytes, in both gate_up layouts."""
    T, topk, E, H, N, Ns = 16, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(730)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    qcfg = [(W8A8, W4A4), (W4A4, FP16), (FP16, W8A8), (W4A4, W4A4), (W8A8, W8A8)]
    ids, wts, sw = routing(g, T, E, topk)
    h = hidden(g, T, H)
    for fuse in (None, False):
        layer = moe.MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=fuse)
        new, old = moe.DecodeForwardWo(layer, T, topk), moe.DecodeForward(layer, T, topk)
        assert new._glu is None and new.layout == old.layout and new.mask1 == old.mask1 == 0b111
        new.launch(h, ids, wts, sw), old.launch(h, ids, wts, sw)
        torch.cuda.synchronize()
        for a, b in ((new.act, old.act), (new.act_shared, old.act_shared), (new.y, old.y), (new.ys, old.ys), (new.out, old.out)):
            assert torch.equal(bits(a), bits(b))
        assert new.status() == 0 == old.status()


# ---- 4. more than one batch -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", [W4A16_ASYM, W8A16_G128_ASYM], ids=lambda q: q.qcfg)
def test_wide_rows_reread_the_weights(q):
    """H = 2176: fp16 A rows of 4352 bytes (5120 in LDS), fewer than 16 to a batch in the 60 KB budget; T = 16, topk = 1
    and every id = 1: 16 rows on one expert, so gate_up's second batch re-reads the weights."""
    T, E, topk, H, N = 16, 2, 1, 2176, 256
    g = torch.Generator().manual_seed(740)
    gate_up, down = f16_weights(g, E, H, N, 0)
    ffn = moe.MoEFFN(gate_up, down, [(q, q)] * E, num_routed=E)
    df = moe.DecodeForwardWo(ffn, T, topk)
    guard(df)
    ids, wts, _ = routing(g, T, E, topk)
    ids.fill_(1)
    mid = check_stages(df, ffn, hidden(g, T, H), ids, wts, None, stages=("close",))
    assert mid["routing"].counts == [0, 16]
    assert df.status() == 0


# ---- 5. the rest ----------------------------------------------------------------------------------------------------

def test_bf16_ends():
    """A block with a bf16 router over exact weight-only gate_ups (grid data, as in test_exact_gate_up_and_down) and
    w8a8 downs, with biases and the clamp: every stage is exact or integer, so out equals the bf16 block.forward bit for
    bit, and y equals the fp16 layer's y on hidden.to(torch.float16) — the row is converted as it is loaded."""
    T, topk, E, H, N, Ns = 16, 2, 4, 384, 384, 640
    g = torch.Generator().manual_seed(750)
    _, down = f16_weights(g, E, H, N, Ns)
    gate_up = [_grid_weight(g, 2 * n, H, W4A16_ASYM)[0] for n in [N] * E + [Ns]]
    b1, b2 = biases(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, [(W4A16_ASYM, W8A8)] * (E + 1), num_routed=E, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    bf = torch.bfloat16
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(bf).to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(bf).to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=w_sg)
    df = moe.DecodeForwardWo(block, T, dtype=bf)
    assert df.out.dtype == bf
    h = hidden(g, T, H, grid=True, dtype=bf)
    got = df.launch(h).clone()
    want, mid = block.forward(h, return_intermediates=True)
    torch.cuda.synchronize()
    assert torch.equal(df.gate_out[0], mid["topk_ids"])
    assert got.dtype == bf and torch.equal(bits(got), bits(want))
    df16 = moe.DecodeForwardWo(ffn, T, topk)
    df16.launch(h.to(torch.float16), mid["topk_ids"], mid["topk_weights"], mid["shared_w"])
    torch.cuda.synchronize()
    assert torch.equal(bits(df.y), bits(df16.y)) and torch.equal(bits(df.ys), bits(df16.ys))
    assert torch.equal(bits(df.y), bits(mid["y"][mid["routing"].inv_slot.long()]))
    assert df.status() == 0
    with pytest.raises(ValueError):
        df.launch(h.to(torch.float16))


def test_block_under_a_graph():
    """A MoEBlock over the scheme's kinds (E = 8, topk = 2, H = 384) captured once — router, both decode kernels, the
    combine — and replayed on two hidden states: each replay equals the uncaptured launch bit for bit."""
    T, E, topk, H, N, Ns = 7, 8, 2, 384, 256, 640
    g = torch.Generator().manual_seed(760)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    qcfg = [SCHEME[e % 5] for e in range(E)] + [SCHEME[5]]
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True)
    df, ref = moe.DecodeForwardWo(block, T), moe.DecodeForwardWo(block, T)
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


def test_bad_ids_and_short_calls_keep_their_guard(scheme_layer):
    """Capacity 16, a call of 7 tokens with an id of E and an id of -1 among valid ones: those pairs' act / y rows and
    every row past the call keep the guard pattern, status() is DECODE_BAD_ID, and out is finite for the tokens whose
    ids are valid."""
    ffn, cap, T, topk = scheme_layer, 16, 7, 2
    g = torch.Generator().manual_seed(770)
    df = moe.DecodeForwardWo(ffn, cap, topk)
    guard(df)
    ids, wts, sw = routing(g, T, ffn.E, topk)
    ids[2, 0], ids[5, 1] = ffn.E, -1
    bad = [2 * topk + 0, 5 * topk + 1]
    out = df.launch(hidden(g, T, ffn.H), ids, wts, sw)
    torch.cuda.synchronize()
    good = [p for p in range(T * topk) if p not in bad]
    for t in (df.act, df.y):
        assert (bits(t[bad]) == GUARD).all() and (bits(t[T * topk:]) == GUARD).all()
        assert not (bits(t[good]) == GUARD).all(dim=1).any()
    for t in (df.act_shared, df.ys):
        assert (bits(t[T:]) == GUARD).all() and not (bits(t[:T]) == GUARD).all(dim=1).any()
    assert (bits(df.out[T:]) == GUARD).all() and out.shape[0] == T
    assert torch.isfinite(out[[t for t in range(T) if t not in (2, 5)]].float()).all()
    assert df.status(reset=True) == nat.DECODE_BAD_ID and df.status() == 0


def test_kind_outside_the_mask_writes_nothing(scheme_layer):
    """Masks that name w8a8 only on the scheme's layer: the weight-only records (the shared expert's among them) set
    DECODE_BAD_KIND and their rows keep the guard; the w8a8 experts' rows are written."""
    ffn, T, topk = scheme_layer, 7, 2
    g = torch.Generator().manual_seed(780)
    df = moe.DecodeForwardWo(ffn, T, topk)
    df.mask1 = df.mask2 = 1 << nat.DECODE_W8A8
    guard(df)
    ids, wts, sw = routing(g, T, ffn.E, topk)
    df.launch(hidden(g, T, ffn.H), ids, wts, sw)
    torch.cuda.synchronize()
    flat = ids.view(-1).tolist()
    for buf, lin in ((df.act, 0), (df.y, 1)):
        for p, e in enumerate(flat):
            written = not (bits(buf[p]) == GUARD).all()
            assert written == (SCHEME[e][lin] is W8A8), (p, e, lin)
    assert (bits(df.act_shared) == GUARD).all() and (bits(df.ys) == GUARD).all()
    assert df.status(reset=True) == nat.DECODE_BAD_KIND
