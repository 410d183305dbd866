"""FP8 MoE layers on the GPU: the per-token e4m3 activation tag (MXMOE_ACT_E4M3) in every mode and build family of the
activation kernel, bit for bit against the numpy reference (tests/_e4m3_layer_ref.py, which tests/test_e4m3_layer.py
proves equal to the oracle), and layers of w8a8_g-1_sym_E4M3 experts — alone, mixed with the other types, under a
graph, with bf16 ends and with biases — stage by stage against the oracle's E4M3 GroupGEMM."""
import numpy as np
import pytest
import torch

from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W4A8_MXFP8, W8A8, W8A8_E4M3
from oracle import oracle
from tests import _e4m3_layer_ref as ref
from tests import _gptoss_ref as gref
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F, I8, M4, M8, E8 = moe.ACT_FP16, moe.ACT_INT8, moe.ACT_MXFP4, moe.ACT_MXFP8, moe.ACT_E4M3
# segment tags (3 routed experts, then the shared one) of the two kinds of call that run the E4M3 builds: beside
# integer segments, and beside MX segments (a mask with bits 4, 6 and 8: the same builds take their MX paths)
FAMILIES = {"f8": [E8, I8, E8, E8], "f8_mx": [E8, M8, M4, E8]}
CANARY = 0xA5
PAD = 64  # canary bytes before and after each store (the stores stay 16-byte aligned)


def _ids(T):
    """[T, 2] over 3 experts: every expert non-empty, unequal counts"""
    pairs = [(0, 1), (2, 0), (1, 2), (0, 2), (2, 1)]
    return torch.tensor([pairs[t % 5] for t in range(T)], dtype=torch.int32, device=DEV)


def _run(mode, glu, src, src_shared, r, tags, W, Ws):
    """One activation pass on stores with canaries around them: (segs, out bytes, scale bit patterns), both as numpy
    on the host. The canaries are checked here."""
    rows = list(r.counts) + ([r.T] if src_shared is not None else [])
    first = r.first_slot + ([r.T * r.topk] if src_shared is not None else [])
    widths = [W] * r.E + ([Ws] if src_shared is not None else [])
    segs, dsegs, out, scales = moe._make_segments(rows, first, widths, tags, DEV)
    nb, ns = out.numel(), scales.numel()
    big = torch.full((nb + 2 * PAD,), CANARY, dtype=torch.uint8, device=DEV)
    bigs = torch.full((2 * ns + 2 * PAD,), CANARY, dtype=torch.uint8, device=DEV)
    o, s = big[PAD:PAD + nb], bigs[PAD:PAD + 2 * ns].view(torch.float16)
    perm = r.perm_token if mode == "gather" else None
    moe._launch_act(mode, glu, src, src_shared, r.T, r.topk, W, Ws, r.sorted_expert, perm, dsegs, len(segs),
                    moe._tag_mask(tags), o, s, None)
    torch.cuda.synchronize()
    big, bigs = big.cpu().numpy(), bigs.cpu().numpy()
    for b, n in ((big, nb), (bigs, 2 * ns)):
        assert (b[:PAD] == CANARY).all() and (b[PAD + n:] == CANARY).all(), "a canary byte was overwritten"
    return segs, big[PAD:PAD + nb], bigs[PAD:PAD + 2 * ns].view(np.uint16)


def _seg_bytes(segs, out, scales, e, tag):
    s = segs[e]
    nbytes = s.rows * s.width * moe._BITS[tag] // 8
    nscale = s.rows * moe._scale_elems(tag, s.width)
    return out[s.out_off:s.out_off + nbytes], scales[s.scale_off:s.scale_off + nscale]


def _check(mode, glu, src, src_shared, r, tags, W, Ws, seg_rows):
    """The pass with ``tags``: every E4M3 segment equals the reference on ``seg_rows[e]`` (fp16 [rows, width] numpy)
    bit for bit; every other segment equals, byte for byte, what the call writes when the E4M3 segments are tagged
    INT8 instead (same offsets, and none of the new builds: the mask then has no bit 8)."""
    segs, out, scales = _run(mode, glu, src, src_shared, r, tags, W, Ws)
    old = [I8 if t == E8 else t for t in tags]
    segs0, out0, scales0 = _run(mode, glu, src, src_shared, r, old, W, Ws)
    for e, tag in enumerate(tags):
        got_o, got_s = _seg_bytes(segs, out, scales, e, tag)
        if tag == E8:
            codes, sbits = ref.quant(seg_rows[e])
            assert np.array_equal(got_s, sbits), (mode, e, "scales")
            assert np.array_equal(got_o.reshape(codes.shape), ref.pack(codes)), (mode, e, "codes")
        else:
            assert (segs[e].out_off, segs[e].scale_off) == (segs0[e].out_off, segs0[e].scale_off)
            want_o, want_s = _seg_bytes(segs0, out0, scales0, e, tag)
            assert np.array_equal(got_o, want_o) and np.array_equal(got_s, want_s), (mode, e, "neighbour")


def _rows_by_segment(slot_rows, shared_rows, r):
    first = r.first_slot
    return [slot_rows[first[e]:first[e] + r.counts[e]] for e in range(r.E)] + [shared_rows]


def _fp16_pass(mode, glu, src, src_shared, r, W, Ws):
    """The activated fp16 values of a pass over gate_up outputs: the same input with every segment tagged FP16 (the
    hardware exp2 / rcp have no bit-exact CPU model). (routed rows in slot order, shared rows), numpy."""
    tags = [F] * (r.E + 1)
    segs, out, _ = _run(mode, glu, src, src_shared, r, tags, W, Ws)
    rows = [out[s.out_off:s.out_off + s.rows * s.width * 2].view(np.float16).reshape(s.rows, s.width) for s in segs]
    return np.concatenate(rows[:-1]), rows[-1]


# ------------------------------------------------------------------ test 1: the quantiser

@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("bf16", [False, True], ids=["fp16", "bf16"])
@pytest.mark.parametrize("T, W", [(9, 128), (9, 640), (2, 16384)])
def test_gather(T, W, bf16, family):
    """Mode 0, from fp16 and from bf16 hidden states: against the reference on hidden.to(fp16)."""
    x = torch.from_numpy(ref.edge_rows(W, seed=1)[[2, 4] if T == 2 else slice(None)])
    if bf16:  # (bf16 values whose fp16 conversion is finite: beyond 65280 a bf16 rounds to fp16's Inf)
        x = x.to(torch.bfloat16).clamp(-65280, 65280)
    h16 = x.to(torch.float16).numpy()
    r = moe.route(_ids(T), 3)
    perm = r.perm_token.cpu().numpy()
    hd = x.to(DEV)
    _check("gather", None, hd, hd, r, FAMILIES[family], W, W, _rows_by_segment(h16[perm], h16, r))


# (N, Ns): one launch; the split-row path of wide shared rows (a quarter of 2176, rounded up to 128, fits the routed
# rows' 640: launch_act in moe_ops.hip), its last quarter 256 wide; two launches
SLOT_SHAPES = {"one_launch": (128, 128), "split_row": (640, 2176), "two_launch": (128, 1024)}


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("shape", list(SLOT_SHAPES))
def test_activated_slots(shape, family):
    """Mode 2 on the edge rows themselves. split_row: the amax of every shared row lies in its last quarter only, so
    the scale is right only if the row amax crosses the four waves."""
    N, Ns = SLOT_SHAPES[shape]
    T = 9
    r = moe.route(_ids(T), 3)
    routed = np.concatenate([ref.edge_rows(N, seed=0), ref.edge_rows(N, seed=1)])
    shared = ref.edge_rows(Ns, seed=0, tail=True)
    assert routed.shape[0] == T * 2 and shared.shape[0] == T
    if shape == "split_row":
        assert (np.abs(shared[2:, :Ns - 256].astype(np.float32)).max(axis=1) <
                np.abs(shared[2:, Ns - 256:].astype(np.float32)).max(axis=1)).all()
    _check("fused", None, torch.from_numpy(routed).to(DEV), torch.from_numpy(shared).to(DEV), r, FAMILIES[family], N, Ns,
           _rows_by_segment(routed, shared, r))


def _gate_up(rows, N, seed):
    """fp16 [rows, 2N]: gate and up over several binades (|g| < 32, |u| < 256: every activation is finite in fp16)"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(rows, 2 * N, generator=g) * torch.exp2(torch.randint(-6, 3, (rows, 1), generator=g).float())
    v[:, N:] *= torch.exp2(torch.randint(-8, 4, (rows, N), generator=g).float())
    if rows > 1:
        v[1] = 0  # a zero row: scale 1
    return v.half()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("mode", ["plain", "interleaved", "glu_silu", "glu_clamp"])
@pytest.mark.parametrize("shape", ["one_launch", "split_row"])
def test_silu_modes(shape, mode, family):
    """Modes 1 and 3 and both GLU builds (with biases): the activated values come from the same input run with every
    segment tagged FP16; those are quantised by the reference."""
    from tests._util import interleave_gate_up_cols

    N, Ns = SLOT_SHAPES[shape]
    T = 9
    r = moe.route(_ids(T), 3)
    routed, shared = _gate_up(T * 2, N, 5), _gate_up(T, Ns, 6)
    glu = keep = None
    if mode == "interleaved":
        routed = torch.from_numpy(interleave_gate_up_cols(routed.numpy()))
        shared = torch.from_numpy(interleave_gate_up_cols(shared.numpy()))
    routed, shared = routed.to(DEV), shared.to(DEV)
    if mode.startswith("glu"):
        g = torch.Generator().manual_seed(7)
        keep = ((torch.rand(3, 2 * N, generator=g) - 0.5).half().to(DEV), (torch.rand(2 * Ns, generator=g) - 0.5).half().to(DEV))
        glu = moe._glu_struct("silu" if mode == "glu_silu" else moe.SwigluClamp(), *keep)
    m = "plain" if glu is not None else mode
    act, act_s = _fp16_pass(m, glu, routed, shared, r, N, Ns)
    assert np.isfinite(act).all() and np.isfinite(act_s).all()
    _check(m, glu, routed, shared, r, FAMILIES[family], N, Ns, _rows_by_segment(act, act_s, r))


# ------------------------------------------------------------------ test 2: a non-finite row

def test_non_finite_row_through_the_bf16_gather():
    """A bf16 hidden value beyond 65504 is +Inf to the fp16 experts: every E4M3 row of that token has codes 0 and the
    scale 0x7E00; every other row of every segment is what it is without it."""
    T, W, bad_t = 9, 640, 4
    tags = FAMILIES["f8"]
    r = moe.route(_ids(T), 3)
    x = torch.from_numpy(ref.edge_rows(W, seed=2)).to(torch.bfloat16).clamp(-65280, 65280)
    xb = x.clone()
    xb[bad_t, 77] = 70000.0
    assert torch.isinf(xb.to(torch.float16)[bad_t, 77])
    (segs, out, sc), (_, out0, sc0) = (_run("gather", None, v.to(DEV), v.to(DEV), r, tags, W, W) for v in (xb, x))
    perm = r.perm_token.cpu().numpy()
    seen = 0
    for e, tag in enumerate(tags):
        s = segs[e]
        tokens = np.arange(T) if e == 3 else perm[s.first_slot:s.first_slot + s.rows]
        o, so = _seg_bytes(segs, out, sc, e, tag)
        o0, so0 = _seg_bytes(segs, out0, sc0, e, tag)
        o, o0 = o.reshape(s.rows, -1), o0.reshape(s.rows, -1)
        for row, t in enumerate(tokens):
            if t != bad_t:
                assert np.array_equal(o[row], o0[row]) and so[row] == so0[row], (e, row)
            elif tag == E8:
                assert not o[row].any() and so[row] == ref.NAN_SCALE, (e, row)
                seen += 1
    assert seen == 2  # its slot of an E4M3 routed expert and its shared row


# ------------------------------------------------------------------ layers

def _weights(g, E, H, N, Ns):
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)
    return [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)], [mk(H, N) for _ in range(E)] + [mk(H, Ns)]


def _routing(g, T, E, topk):
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    return ids, torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV), torch.rand(T, generator=g).to(DEV)


def _check_e4m3_batch(a, seg_rows, what):
    """An all-E4M3 ActBatch against the reference on the rows of each segment."""
    for e, rows in enumerate(seg_rows):
        codes, sbits = ref.quant(rows)
        assert np.array_equal(a.scale(e).cpu().numpy().view(np.uint16), sbits), (what, e, "scales")
        assert np.array_equal(a.A(e).cpu().numpy(), ref.pack(codes)), (what, e, "codes")


def _check_gemm(a, ws, C_of, what):
    """A GroupGEMM stage's outputs against the oracle on the device's own A operands and the prepared weights, within
    the project's bar for this tile (tests/_util.assert_f16_close)."""
    for e, w in enumerate(ws):
        rows = a.segs[e].rows
        if rows == 0:
            continue
        want = oracle.gg_e4m3(a.A(e).cpu().numpy(), w.B.cpu().numpy(), a.scale(e).cpu().numpy(), w.scale_b.cpu().numpy(),
                              rows, w.N, w.K)
        try:
            assert_f16_close(C_of(e).cpu().numpy(), want, w.K)
        except AssertionError as err:
            raise AssertionError(f"{what}, expert {e}: {err}") from None


def _stage_check(ffn, h, ids, wts, sw, E):
    """``MoEFFN.forward`` of an all-E4M3 layer stage by stage up to y: a1 and a2 bit for bit against the reference, h1
    and y against the oracle on the device's own operands. Returns (out, the intermediates, the routing)."""
    out, mid = ffn.forward(h, ids, wts, sw, return_intermediates=True)
    torch.cuda.synchronize()
    r = mid["routing"]
    perm = r.perm_token.cpu().numpy()
    h16 = h.to(torch.float16).cpu().numpy()
    first = r.first_slot
    seg = lambda t, e: t[first[e]:first[e] + r.counts[e]]
    _check_e4m3_batch(mid["a1"], _rows_by_segment(h16[perm], h16, r), "a1")
    _check_gemm(mid["a1"], ffn.w1, lambda e: mid["h1s"] if e == E else seg(mid["h1"], e), "h1")
    # a2: the device's own h1 through the same pass with FP16 tags, then the reference
    fp = [F] * (E + 1)
    if ffn.biased_or_gated:
        act = moe.glu_quant(mid["h1"], mid["h1s"], r, fp, ffn.activation, ffn.b1, ffn.b1s)
    else:
        act = moe.silu_mul_quant(mid["h1"], mid["h1s"], r, fp)
    torch.cuda.synchronize()
    _check_e4m3_batch(mid["a2"], [act.A(e).cpu().numpy() for e in range(E + 1)], "a2")
    _check_gemm(mid["a2"], ffn.w2, lambda e: mid["ys"] if e == E else seg(mid["y"], e), "y")
    return out, mid, r


def test_all_e4m3_layer_stage_by_stage():
    """★ The test that fails without the feature: on the parent commit a1 holds int8 codes."""
    E, topk, T, H, N, Ns = 4, 2, 33, 256, 128, 256
    g = torch.Generator().manual_seed(21)
    gu, dn = _weights(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gu, dn, [(W8A8_E4M3, W8A8_E4M3)] * (E + 1), num_routed=E)
    assert ffn.tag1 == ffn.tag2 == [E8] * 5 and not ffn.fuse_silu
    h = torch.randn(T, H, generator=g).half().to(DEV)
    ids, wts, sw = _routing(g, T, E, topk)
    out, mid, r = _stage_check(ffn, h, ids, wts, sw, E)
    assert tuple(mid["h1"].shape) == (T * topk, 2 * N)  # the plain layout
    want = gref.combine_bias(mid["y"].cpu().numpy(), r.inv_slot.cpu().numpy(), r.sorted_expert.cpu().numpy(),
                             wts.cpu().numpy(), topk, None, E, mid["ys"].cpu().numpy(), sw.cpu().numpy())
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_biased_layer():
    """An all-E4M3 layer with the four biases and the clamped SwiGLU, eager: a2 through glu_quant, out against
    combine_bias's chain."""
    E, topk, T, H, N, Ns = 4, 2, 33, 256, 128, 256
    g = torch.Generator().manual_seed(22)
    gu, dn = _weights(g, E, H, N, Ns)
    mk = lambda n: (torch.rand(n, generator=g) - 0.5).half().to(DEV)
    b1 = [mk(2 * N) for _ in range(E)] + [mk(2 * Ns)]
    b2 = [mk(H) for _ in range(E + 1)]
    ffn = moe.MoEFFN(gu, dn, [(W8A8_E4M3, W8A8_E4M3)] * (E + 1), num_routed=E, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    h = torch.randn(T, H, generator=g).half().to(DEV)
    ids, wts, sw = _routing(g, T, E, topk)
    out, mid, r = _stage_check(ffn, h, ids, wts, sw, E)
    want = gref.combine_bias(mid["y"].cpu().numpy(), r.inv_slot.cpu().numpy(), r.sorted_expert.cpu().numpy(),
                             wts.cpu().numpy(), topk, ffn.b2.cpu().numpy(), E, mid["ys"].cpu().numpy(), sw.cpu().numpy(),
                             ffn.b2s.cpu().numpy())
    assert np.array_equal(out.cpu().numpy().view(np.uint16), want.view(np.uint16))


def test_mixed_layer_eager_planned_graph():
    """E4M3 beside w8a8, fp16, w4a4 and w4a8_g32_sym_MXFP8, per expert and per linear (both activation passes run
    the builds that carry the MX tags and the E4M3 tag): the three forwards agree within the fp16 tolerance — the
    types sum in f32 in an order the plan decides, as tests/test_dynamic_plan_gpu.py compares them."""
    E, topk, T, H, N, Ns = 4, 2, 33, 256, 128, 256
    g = torch.Generator().manual_seed(23)
    gu, dn = _weights(g, E, H, N, Ns)
    E4 = W8A8_E4M3
    qcfg = [(E4, E4), (W8A8, E4), (FP16, W4A4), (W4A8_MXFP8, E4), (E4, E4)]
    ffn = moe.MoEFFN(gu, dn, qcfg, num_routed=E)
    assert ffn.tag1 == [E8, I8, F, M8, E8] and ffn.tag2 == [E8, E8, moe.ACT_INT4, E8, E8] and not ffn.fuse_silu
    gf = moe.GraphForward(ffn, T, topk)
    assert gf.mode == "plain" and gf.mask1 & (1 << 8) and gf.mask2 & (1 << 8)
    for _ in range(2):
        h = torch.randn(T, H, generator=g).half().to(DEV)
        ids, wts, sw = _routing(g, T, E, topk)
        want = ffn.forward(h, ids, wts).cpu().numpy()
        planned = moe.PlannedForward(ffn, h, ids, wts)().cpu().numpy()
        graph = gf.launch(h, ids, wts).cpu().numpy()
        assert_f16_close(planned, want, H)
        assert_f16_close(graph, want, H)
        with_sw = gf.launch(h, ids, wts, sw).cpu().numpy()
        assert_f16_close(with_sw, ffn.forward(h, ids, wts, sw).cpu().numpy(), H)
    assert gf.status() == 0


def test_bf16_block_under_a_graph():
    """GraphForward of a bf16 MoEBlock with E4M3 experts, captured once and replayed under two routings, one of which
    leaves an E4M3 expert empty: each replay equals the uncaptured launch bit for bit."""
    E, topk, T, H, N, Ns = 4, 2, 33, 256, 128, 256
    g = torch.Generator().manual_seed(24)
    gu, dn = _weights(g, E, H, N, Ns)
    E4 = W8A8_E4M3
    ffn = moe.MoEFFN(gu, dn, [(E4, E4), (E4, E4), (W8A8, E4), (E4, W8A8), (E4, E4)], num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(torch.bfloat16).to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(torch.bfloat16).to(DEV)
    e_bias = torch.zeros(E, dtype=torch.float32, device=DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=w_sg, scoring="sigmoid", e_bias=e_bias)
    gf = moe.GraphForward(block, T)
    assert gf.dtype == torch.bfloat16
    hiddens = [torch.randn(T, H, generator=g).to(torch.bfloat16).to(DEV) for _ in range(2)]
    static = hiddens[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gf.launch(static)  # warm-up outside the capture (module loading)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gf.launch(static)
    torch.cuda.current_stream().wait_stream(side)
    for i, h in enumerate(hiddens):
        e_bias.zero_()
        if i == 1:
            e_bias[1] = -8.0  # sigmoid scores lie in (0, 1): the E4M3 expert 1 is never chosen
        static.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        got = gf.out.clone()
        counts = gf.route_bufs[3].cpu().tolist()
        assert (counts[1] == 0) == (i == 1) and sum(counts) == T * topk
        want = gf.launch(h).clone()
        torch.cuda.synchronize()
        assert got.dtype == torch.bfloat16 and torch.isfinite(got.float()).all()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16)), i
    assert gf.status() == 0
