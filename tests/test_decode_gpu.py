"""GPU tests of the decode forward (moe.DecodeForward; mxmoe_moe_decode_gate_up / mxmoe_moe_decode_down, DESIGN.md §4
"Decode forward"): a layer call of 1..16 tokens without a planner equals the eager layer (MoEFFN.forward /
MoEBlock.forward) — bit for bit for the integer experts, whose dot products are exact and whose every other step is the
eager path's arithmetic; within the fp16 tolerance for fp16 experts on random data (another f32 summation order), bit for
bit where the data make every partial sum exact.

The eager intermediates are in slot order (sorted by expert), the decode buffers in pair order: row p of ``act`` / ``y``
is row inv_slot[p] of the eager one. The stages are compared in order, so the first wrong one is named."""
from __future__ import annotations

import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4, W8A8
from tests._decode_util import DEV, GUARD, bits, check_stages, f16_weights, hidden, routing

pytestmark = pytest.mark.gpu
INT_QCFG = [(W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8)]


@pytest.mark.parametrize("fuse", [None, False], ids=["interleaved", "plain"])
@pytest.mark.parametrize("T", [1, 7, 16])
def test_int_experts_bit_for_bit(T, fuse):
    """★ 1. w8a8 / w4a4 experts, both gate_up layouts, with and without shared_w, two routings through one object:
    act, y and out equal the eager layer's bit for bit. The plain layer's act also equals the interleaved layer's
    (the layout changes only the row index)."""
    topk, E, H, N, Ns = 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(400 + T)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, INT_QCFG, num_routed=E, fuse_silu=fuse)
    df = moe.DecodeForward(ffn, T, topk)
    assert df.layout == (nat.DECODE_GU_PLAIN if fuse is False else nat.DECODE_GU_INTERLEAVED)
    other = moe.DecodeForward(moe.MoEFFN(gate_up, down, INT_QCFG, num_routed=E), T, topk) if fuse is False else None
    for _ in range(2):
        ids, wts, sw = routing(g, T, E, topk)
        h = hidden(g, T, H)
        check_stages(df, ffn, h, ids, wts, sw)
        check_stages(df, ffn, h, ids, wts, None)
        if other is not None:
            other.launch(h, ids, wts, sw)
            torch.cuda.synchronize()
            assert torch.equal(bits(df.act), bits(other.act)) and torch.equal(bits(df.act_shared), bits(other.act_shared))
    assert df.status() == 0
    with pytest.raises(ValueError):
        df.launch(h, ids.long(), wts, sw)  # nothing is converted: the dtypes are the caller's


def test_layer_without_a_shared_expert():
    """★ 1. The same without a shared expert (no shared tiles in the grid, no ys)."""
    T, topk, E, H, N = 7, 2, 4, 256, 128
    g = torch.Generator().manual_seed(431)
    gate_up, down = f16_weights(g, E, H, N, 0)
    ffn = moe.MoEFFN(gate_up, down, INT_QCFG[:E], num_routed=E)
    df = moe.DecodeForward(ffn, T, topk)
    assert df.ys is None and df.act_shared is None
    for _ in range(2):
        ids, wts, _ = routing(g, T, E, topk)
        check_stages(df, ffn, hidden(g, T, H), ids, wts, None)
    assert df.status() == 0


@pytest.mark.parametrize("topk", [1, 8])
def test_routing_extremes(topk):
    """★ 2. T = 16, E = 8. topk = 1 with every token on expert 5: 16 rows on one expert, seven experts empty;
    topk = 8: every expert holds every token. The bounds of the row loop."""
    T, E, H, N, Ns = 16, 8, 256, 128, 256
    g = torch.Generator().manual_seed(440 + topk)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    qcfg = [INT_QCFG[e % 2] for e in range(E)] + [(W8A8, W8A8)]
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    df = moe.DecodeForward(ffn, T, topk)
    ids, wts, sw = routing(g, T, E, topk)
    if topk == 1:
        ids.fill_(5)
    mid = check_stages(df, ffn, hidden(g, T, H), ids, wts, sw)
    assert mid["routing"].counts == ([0] * 5 + [16, 0, 0] if topk == 1 else [16] * 8)
    assert df.status() == 0


GRID_QCFG = [(FP16, W8A8), (W8A8, W4A4), (FP16, W8A8), (W4A4, W8A8), (FP16, W8A8)]
SWAP_QCFG = [(W8A8, W4A4), (W4A4, W8A8), (W8A8, W4A4), (W4A4, W8A8), (W4A4, W8A8)]


@pytest.mark.parametrize("case", ["int", "swapped", "fp16_gate_up"])
def test_width_tails(case):
    """★ 3. H = 384, N = 384, Ns = 640: multiples of 128 that are no powers of two, so the column tiles and the K loops
    (1024-byte groups of 256-byte steps) end inside a group. swapped: the two linears of an expert differ in type
    (w8a8 / w4a4). fp16_gate_up: fp16 gate_up over a w8a8 down, on data that make every f32 partial sum of the fp16
    dot products exact (hidden multiples of 1/8 in [-2, 2], weights multiples of 1/4 in [-1, 1]: products are
    multiples of 1/32 below 2, sums of 384 of them need 15 bits), so the whole layer is bit-exact."""
    T, topk, E, H, N, Ns = 7, 2, 4, 384, 384, 640
    grid = case == "fp16_gate_up"
    qcfg = {"int": INT_QCFG, "swapped": SWAP_QCFG, "fp16_gate_up": GRID_QCFG}[case]
    g = torch.Generator().manual_seed(450)
    gate_up, down = f16_weights(g, E, H, N, Ns, grid=grid)
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    df = moe.DecodeForward(ffn, T, topk)
    for _ in range(2):
        ids, wts, sw = routing(g, T, E, topk)
        check_stages(df, ffn, hidden(g, T, H, grid=grid), ids, wts, sw)
    assert df.status() == 0


def test_fp16_experts_exact_gate_up():
    """★ 4a. fp16 experts on the exact grid (as in test_width_tails): act equals the eager path's bit for bit,
    whatever the summation orders."""
    T, topk, E, H, N, Ns = 7, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(460)
    gate_up, down = f16_weights(g, E, H, N, Ns, grid=True)
    ffn = moe.MoEFFN(gate_up, down, [(FP16, FP16)] * (E + 1), num_routed=E)
    df = moe.DecodeForward(ffn, T, topk)
    ids, wts, sw = routing(g, T, E, topk)
    h = hidden(g, T, H, grid=True)
    df.launch(h, ids, wts, sw)
    _, mid = ffn.forward(h, ids, wts, sw, return_intermediates=True)
    torch.cuda.synchronize()
    inv = mid["routing"].inv_slot.long()
    assert mid["h1"].shape[1] == N, "the eager gate_up is expected to run its SiLU epilogue at this size"
    assert torch.equal(bits(df.act), bits(mid["h1"][inv]))
    assert torch.equal(bits(df.act_shared), bits(mid["h1s"]))


@pytest.mark.parametrize("qcfg", [[(FP16, FP16)] * 5, [(W8A8, FP16), (FP16, FP16), (W4A4, FP16), (W8A8, FP16), (FP16, FP16)]],
                         ids=["fp16", "mixed"])
def test_fp16_experts_random_data(qcfg):
    """★ 4b. fp16 experts (alone, and fp16 down projections behind integer gate_ups) on random data: out within the
    project's fp16 tolerance of the eager layer (the summation orders differ, so equality is not asked). An fp16
    gate_up in front of an integer down is tested on exact data instead (test_width_tails): on random data a last-bit
    difference in act can move a quantised code."""
    T, topk, E, H, N, Ns = 16, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(470)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    df = moe.DecodeForward(ffn, T, topk)
    ids, wts, sw = routing(g, T, E, topk)
    check_stages(df, ffn, hidden(g, T, H), ids, wts, sw, stages=("close",))
    assert df.status() == 0


def _block(qcfg, seed, T, dtype=torch.float16):
    """tests/test_dynamic_plan_gpu.py's _block at T tokens (sigmoid scores and a selection bias, so a test can starve
    an expert), optionally with bf16 ends."""
    topk, E, H, N, Ns = 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(seed)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, qcfg, num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(dtype).to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(dtype).to(DEV)
    e_bias = torch.zeros(E, dtype=torch.float32, device=DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=w_sg, scoring="sigmoid", e_bias=e_bias)
    hiddens = [torch.randn(T, H, generator=g).to(dtype).to(DEV) for _ in range(3)]
    return block, hiddens


def test_block_under_a_graph():
    """★ 5. The integer MoEBlock at T = 16 captured once (router, both decode kernels, combine) and replayed on three
    routings, one with a starved expert: every replay equals block.forward bit for bit."""
    T = 16
    block, hiddens = _block(INT_QCFG, 7, T)
    df = moe.DecodeForward(block, T)
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
    e_bias = block.routing["e_bias"]
    counts = []
    for i, h in enumerate(hiddens):
        e_bias.zero_()
        if i == 2:
            e_bias[1] = -8.0  # sigmoid scores lie in (0, 1): expert 1 is never chosen
        static_hidden.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        got = df.out.clone()
        want, mid = block.forward(h, return_intermediates=True)
        torch.cuda.synchronize()
        counts.append(mid["routing"].counts)
        assert torch.equal(df.gate_out[0], mid["topk_ids"])
        assert torch.equal(bits(got), bits(want)), i
    assert counts[2][1] == 0 and len({tuple(c) for c in counts}) == 3  # three routings, one starved expert
    assert df.status() == 0


def test_bf16_ends():
    """★ 6. bf16 hidden states, router weights and out: equal to the bf16 block.forward bit for bit, and y equals the
    fp16 layer's y on hidden.to(torch.float16) (the row is converted as it is loaded, nothing after differs)."""
    T = 16
    block, hiddens = _block(INT_QCFG, 9, T, dtype=torch.bfloat16)
    df = moe.DecodeForward(block, T, dtype=torch.bfloat16)
    assert df.out.dtype == torch.bfloat16
    h = hiddens[0]
    got = df.launch(h).clone()
    want, mid = block.forward(h, return_intermediates=True)
    torch.cuda.synchronize()
    assert got.dtype == torch.bfloat16 and torch.equal(bits(got), bits(want))
    df16 = moe.DecodeForward(block.ffn, T, block.topk)
    df16.launch(h.to(torch.float16), mid["topk_ids"], mid["topk_weights"], mid["shared_w"])
    torch.cuda.synchronize()
    assert torch.equal(bits(df.y), bits(df16.y)) and torch.equal(bits(df.ys), bits(df16.ys))
    assert torch.equal(bits(df.y), bits(mid["y"][mid["routing"].inv_slot.long()]))
    with pytest.raises(ValueError):
        df.launch(h.to(torch.float16))
    with pytest.raises(ValueError):
        moe.DecodeForward(block, T, dtype=torch.float16)


def test_rows_past_the_call_keep_their_guard():
    """★ 7. Capacity 16, a call of 5 tokens: the rows of act, act_shared, y, ys and out past the call's keep the guard
    pattern; every row inside is written."""
    cap, T, topk, E, H, N, Ns = 16, 5, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(480)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    ffn = moe.MoEFFN(gate_up, down, INT_QCFG, num_routed=E)
    df = moe.DecodeForward(ffn, cap, topk)
    bufs = [(df.act, T * topk), (df.act_shared, T), (df.y, T * topk), (df.ys, T), (df.out, T)]
    for t, _ in bufs:
        bits(t).fill_(GUARD)
    ids, wts, sw = routing(g, T, E, topk)
    h = hidden(g, T, H)
    out = df.launch(h, ids, wts, sw)
    want = ffn.forward(h, ids, wts, sw)
    torch.cuda.synchronize()
    assert out.shape[0] == T and torch.equal(bits(out), bits(want))
    for t, rows in bufs:
        assert (bits(t[rows:]) == GUARD).all()
        assert not (bits(t[:rows]) == GUARD).all(dim=1).any()
    assert df.status() == 0
