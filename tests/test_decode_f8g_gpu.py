"""GPU tests of the decode forward for block-scaled FP8 experts (moe.DecodeForwardF8g; mxmoe_moe_decode_gate_up_f8g /
mxmoe_moe_decode_down_f8g, DESIGN.md §4 "Decode forward: block-scaled FP8"): layers of w8a8_g128_sym_E4M3 experts in a
call of 1..16 tokens.

Every stage is held to the float64 reference of its own device input (tests/_f8g128_ref.py): act to ref.gemm on
quantize.quant_e4m3_g128(hidden) and the layer's own codes and block scales (g and u rounded to fp16, then the gated
activation: _decode_util.assert_act_close), y to ref.gemm on quant_e4m3_g128 of the device's own act, out to the
combine of the device's own y — within tests/_util.assert_f16_close, the figure MoEFFN.forward is held to for this type
(tests/test_f8g128_layer_gpu.py). The down entry alone is also checked bit for bit on operands whose sums are exact in
any order."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import W8A8_G128_E4M3 as QG
from mxmoe_amd.quantize import quant_e4m3_g128, unpack_wxax
from tests import _f8g128_ref as ref
from tests import _gptoss_ref as gref
from tests._decode_util import DEV, GUARD, assert_act_close, bits, eager_act, f16_weights, guard, hidden, routing
from tests._mxfp8_ref import e4m3
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu


def _linear(x, w):
    """fp16 rows through one linear of the layer: the type's contract in float64 [rows, N]."""
    codes, sa = quant_e4m3_g128(x.cpu())
    return ref.gemm(codes.numpy(), sa.numpy(), unpack_wxax(w.B.cpu(), 8, w.K).numpy().view(np.uint8), w.scale_b.cpu().numpy().T)


def _check(df, ffn, h, ids=None, wts=None, sw=None, skip=()):
    """One launch, stage by stage, the rows of an expert together; pairs in ``skip`` (ids outside [0, E)) are not
    compared. A MoEBlock routes itself: its ids and weights are read back."""
    got = (df.launch(h) if df.block is not None else df.launch(h, ids, wts, sw)).clone()
    torch.cuda.synchronize()
    if df.block is not None:
        ids, wts, sw = df.gate_out
    T, topk = ids.shape
    n, E = T * topk, ffn.E
    h16, flat = h.to(torch.float16).cpu(), ids.view(-1).tolist()
    jobs = [(e, [p for p, x in enumerate(flat) if x == e and p not in skip]) for e in range(E)]
    jobs = [(e, h16[[p // topk for p in ps]], df.act[ps], df.y[ps]) for e, ps in jobs if ps]
    if ffn.has_shared:
        jobs.append((E, h16[:T], df.act_shared[:T], df.ys[:T]))
    for e, x, act, y in jobs:
        w1, w2 = ffn.w1[e], ffn.w2[e]
        gu, act = _linear(x, w1).astype(np.float16), act.cpu()
        for r in range(len(gu)):
            assert_act_close(act[r:r + 1].numpy(), gu[r:r + 1], None, "silu", {})
        assert_f16_close(y.cpu().numpy(), _linear(act, w2), w2.K)
    y = df.y[:n].cpu().numpy().copy()
    for p in skip:
        y[p] = 0  # (whatever the row holds is weighted in; the test compares the tokens without a bad id)
    want = gref.combine_bias(y, np.arange(n), np.array(flat), wts.cpu().numpy(), topk, None, E,
                             df.ys[:T].cpu().numpy() if ffn.has_shared else None, None if sw is None else sw.cpu().numpy())
    ok = [t for t in range(T) if not any(t * topk + k in skip for k in range(topk))]
    out, want = got.float().cpu().numpy()[ok].astype(np.float64), want.astype(np.float64)[ok]
    if got.dtype == torch.bfloat16:  # the f32 sum rounded to bf16 (8 significant bits): half an ulp, up to 2^-8 |ref|
        rms = np.sqrt(np.mean(want * want))
        assert (np.abs(out - want) <= (1e-3 + 2.0 ** -8) * np.abs(want) + 1e-3 * rms + 1e-6).all()
    else:
        assert_f16_close(out, want, ffn.H)
    return got


def _layer(E, H, N, Ns, seed):
    g = torch.Generator().manual_seed(seed)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    return g, moe.MoEFFN(gate_up, down, [(QG, QG)] * (E + (1 if Ns else 0)), num_routed=E)


# (H, N): one K group (an empty K slice) and three scale blocks (gate and up in different blocks); five groups (an
# uneven split, the row ending inside the trip in flight); nine groups (a slice of more than one trip) — in both
# linears, as down's K is N
@pytest.mark.parametrize("H,N", [(128, 384), (640, 256), (1152, 128)])
@pytest.mark.parametrize("T", [1, 5, 16])
def test_against_f64(T, H, N):
    """★ fails without the feature (no class, no entries). E = 4, topk = 2, the shared expert with N_shared != N; act
    also against the eager layer's activation rows."""
    E, topk, Ns = 4, 2, 128 if N != 128 else 256
    g, ffn = _layer(E, H, N, Ns, 1100 + T + H)
    df = moe.DecodeForwardF8g(ffn, T, topk)
    bufs = guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    h = hidden(g, T, H)
    _check(df, ffn, h, ids, wts, sw)
    for t in bufs:
        assert not (bits(t) == GUARD).all(dim=1).any()
    _, mid = ffn.forward(h, ids, wts, sw, return_intermediates=True)
    act, act_s = eager_act(ffn, mid)
    assert_f16_close(df.act.cpu().numpy(), act[mid["routing"].inv_slot.long()].cpu().numpy(), H)
    assert_f16_close(df.act_shared.cpu().numpy(), act_s.cpu().numpy(), H)
    assert df.status() == 0


def _exact_operands(n, E, H, K, seed):
    """A rows [n, K] (fp16) whose in-kernel quantisation is known, the codes and scales it must give, and per expert the
    down weight's codes [H, K] and block scales: in every 128-group of a row one element is 448 * 2^e at a column
    where every weight code is zero (a 448 code beside small products is not what this test is about: DESIGN.md §4
    "Decode forward on MFMA"), the others c * 2^e with c in 0, +-1 .. +-4 — so the group scale is 2^e and the codes
    are c's. Every group sum is an integer below 2^11 and every fold fits 24 bits: the result is the same in any
    order."""
    a_codes, sa, _, _ = ref.operands(n, H, K, True, seed)
    hot = 128 * np.arange(K // 128) + (7 * np.arange(K // 128) + 3) % 128
    a_codes[:, hot] = 0x7E  # 448
    ws = []
    for e in range(E):
        _, _, b_codes, sb = ref.operands(1, H, K, True, seed + 1 + e)
        b_codes[:, hot] = 0
        ws.append((b_codes, sb))
    x = (e4m3(a_codes) * np.repeat(sa, 128, axis=1)).astype(np.float16)
    return x, a_codes, sa, ws


# K = N of 128 / 640 / 1152 on 32-column tiles (two K slices: none / uneven / more than one trip); E = 64 at H = 1024
# and 2048: the smallest shapes with 64- and 128-column tiles (one slice; two column passes at 128)
@pytest.mark.parametrize("E,topk,T,N,H", [(4, 2, 16, 128, 256), (4, 2, 16, 640, 256), (4, 2, 16, 1152, 256),
                                          (64, 4, 16, 128, 1024), (64, 4, 16, 128, 2048)])
def test_down_exact(E, topk, T, N, H):
    n = T * topk
    x, a_codes, sa, ws = _exact_operands(n, E, H, N, 1200 + N + H)
    ids = (torch.arange(n, dtype=torch.int32) % E).view(T, topk).to(DEV)
    flat = ids.view(-1).tolist()
    want = np.stack([ref.gemm_fold_f32(a_codes[p:p + 1], sa[p:p + 1], *ws[e])[0] for p, e in enumerate(flat)])
    exact = np.stack([ref.gemm(a_codes[p:p + 1], sa[p:p + 1], *ws[e])[0] for p, e in enumerate(flat)])
    assert np.array_equal(want, exact.astype(np.float16)) and np.abs(exact).max() > 0  # the fold is exact: any order
    zero = lambda rows, k: (torch.zeros(rows, k, dtype=torch.uint8), torch.ones((rows + 127) // 128, k // 128))
    w1 = [moe.prepare_weight_e4m3_g128(*(t.to(DEV) for t in zero(2 * N, H))) for _ in range(E)]
    w2 = [moe.prepare_weight_e4m3_g128(torch.from_numpy(b).to(DEV), torch.from_numpy(sb).to(DEV)) for b, sb in ws]
    ffn = moe.MoEFFN(w1, w2, [(QG, QG)] * E, num_routed=E)
    df = moe.DecodeForwardF8g(ffn, T, topk)
    guard(df)
    df.act.copy_(torch.from_numpy(x))
    p = lambda t: None if t is None else moe._ptr(t)
    nat.check(nat.symbol(df.ENTRIES[1])(T, topk, E, 0, p(ids), p(df.experts), df.mask2, H, N, 0, p(df.act), None, p(df.y), None,
                                        p(df.dev_status), None))
    torch.cuda.synchronize()
    assert np.array_equal(df.y.cpu().numpy().view(np.uint16), want.view(np.uint16)) and df.status() == 0


@pytest.mark.parametrize("T,H,N", [(16, 640, 256), (5, 640, 256), (16, 8192, 128)])
def test_batches(T, H, N):
    """topk = 4 on E = 4 with every id equal: T = 16 puts 64 rows on one expert (four batches), T = 5 puts 20 (the last
    batch partial); H = 8192: fewer than 16 rows fit the LDS budget."""
    E, topk = 4, 4
    g, ffn = _layer(E, H, N, 0, 1300 + T + H)
    df = moe.DecodeForwardF8g(ffn, T, topk)
    _, wts, _ = routing(g, T, E, topk)
    _check(df, ffn, hidden(g, T, H), torch.full((T, topk), T % E, dtype=torch.int32, device=DEV), wts, None)
    assert df.status() == 0


def test_bf16_block():
    """A bf16 MoEBlock call (the router in front): hidden converted as it is loaded (the reference: hidden.to(fp16)),
    out bf16."""
    T, E, topk, H = 5, 4, 2, 640
    g, ffn = _layer(E, H, 256, 128, 1400)
    w_gate = torch.randn(E, H, generator=g).to(torch.bfloat16).to(DEV)
    df = moe.DecodeForwardF8g(moe.MoEBlock(ffn, w_gate, topk), T)
    got = _check(df, ffn, hidden(g, T, H, dtype=torch.bfloat16))
    assert got.dtype == torch.bfloat16 and df.status() == 0


def test_bad_id_keeps_its_rows():
    T, E, topk = 5, 4, 2
    g, ffn = _layer(E, 128, 384, 256, 1410)
    df = moe.DecodeForwardF8g(ffn, T, topk)
    guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    ids[2, 1] = E
    _check(df, ffn, hidden(g, T, 128), ids, wts, sw, skip=(2 * topk + 1,))
    assert (bits(df.act[5]) == GUARD).all() and (bits(df.y[5]) == GUARD).all()
    assert df.status(reset=True) == nat.DECODE_BAD_ID and df.status() == 0


def test_under_a_graph():
    """Captured once, replayed with two routings: every replay equals the uncaptured launch bit for bit."""
    T, E, topk, H = 5, 4, 2, 640
    g, ffn = _layer(E, H, 256, 128, 1420)
    df, other = moe.DecodeForwardF8g(ffn, T, topk), moe.DecodeForwardF8g(ffn, T, topk)
    calls = [(hidden(g, T, H), *routing(g, T, E, topk)) for _ in range(2)]
    static = [t.clone() for t in calls[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.launch(*static)  # warm-up outside the capture (module loading)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        df.launch(*static)
    torch.cuda.current_stream().wait_stream(side)
    for call in calls + calls[:1]:
        for s, t in zip(static, call):
            s.copy_(t)
        graph.replay()
        torch.cuda.synchronize()
        want = other.launch(*call).clone()
        torch.cuda.synchronize()
        for a, b in ((df.act, other.act), (df.y, other.y), (df.out, want)):
            assert torch.equal(bits(a), bits(b))
    assert not torch.equal(calls[0][1], calls[1][1]) and df.status() == 0
