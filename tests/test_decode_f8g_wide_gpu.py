"""GPU tests of the wide decode forward for block-scaled FP8 experts (moe.DecodeForwardF8gWide; DESIGN.md §4 "Decode
forward: block-scaled FP8, wide"): calls of 1..64 tokens. The quantiser and the tile entries are held to bits
(quantize.quant_e4m3_g128, _f8g128_ref.gemm_fold_f32), the whole layer stage by stage to float64 of its own device input
(test_decode_f8g_gpu.py's scheme, restated), and the down stage to MoEFFN.forward's y rows bit for bit."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import W8A8_G128_E4M3 as QG
from mxmoe_amd.quantize import quant_e4m3_g128, unpack_wxax
from tests import _f8g128_edges as X
from tests import _f8g128_ref as ref
from tests import _gptoss_ref as gref
from tests._decode_util import DEV, GUARD, assert_act_close, bits, eager_act, f16_weights, guard, hidden, routing
from tests._mxfp8_ref import e4m3
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
P = lambda t: None if t is None else moe._ptr(t)  # noqa: E731


def _canon(codes):
    """Device codes (pack_wxax's 8-bit order) in K order."""
    return unpack_wxax(codes.cpu(), 8, codes.shape[1]).numpy().view(np.uint8)


def _quant(x, codes, scales):
    nat.check(nat.symbol("mxmoe_moe_decode_quant_f8g")(moe._DT[x.dtype], P(x), x.shape[0], x.shape[1], P(codes), P(scales),
                                                       None, 0, 0, None, None, None))


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("K", [128, 640])
def test_quantiser_bits(K, dtype):
    """Codes and scales against quantize.quant_e4m3_g128: random rows and rows whose first group is zero, -0, holds a
    65504 (fp16), an Inf or a NaN."""
    x = torch.randn(7, K, generator=torch.Generator().manual_seed(K)).to(dtype)
    x[1, :128] = 0.0
    x[2, :128] = -0.0
    x[3, 5] = 65504.0 if dtype == torch.float16 else 65280.0  # (the largest bf16 inside fp16)
    x[4, 7] = float("inf")
    x[5, K - 1] = float("nan")
    codes = torch.full((7, K), 0x7B, dtype=torch.uint8, device=DEV)
    scales = torch.full((7, K // 128), -1.0, device=DEV)
    _quant(x.to(DEV), codes, scales)
    torch.cuda.synchronize()
    want_c, want_s = quant_e4m3_g128(x.to(torch.float16) if dtype == torch.float16 else x.float().to(torch.float16))
    assert np.array_equal(_canon(codes), want_c.numpy().view(np.uint8))
    got_s, want_s = scales.cpu().numpy(), want_s.numpy()
    assert np.array_equal(np.isnan(got_s), np.isnan(want_s)) and np.isnan(want_s).sum() == 2
    assert np.array_equal(got_s[~np.isnan(want_s)].view(np.uint32), want_s[~np.isnan(want_s)].view(np.uint32))


def _layer_of(E, T, topk, N, H, w1=None, w2=None):
    def prep(ws, rows, k):
        if ws is None:
            return [moe.prepare_weight_e4m3_g128(torch.zeros(rows, k, dtype=torch.uint8, device=DEV),
                                                 torch.ones((rows + 127) // 128, k // 128, device=DEV))] * E
        return [moe.prepare_weight_e4m3_g128(torch.from_numpy(b).to(DEV), torch.from_numpy(sb).to(DEV)) for b, sb in ws]
    df = moe.DecodeForwardF8gWide(moe.MoEFFN(prep(w1, 2 * N, H), prep(w2, H, N), [(QG, QG)] * E, num_routed=E), T, topk)
    guard(df)
    return df


# (E, topk, T, K, C); pair p goes to expert p % E, so an expert has T * topk / E rows.
#   (4, 2, 5)   2 or 3 rows: MB = 1, partial;       RB = 16, KC = min(K, 1024) = 640: K in one chunk
#   (2, 2, 24)  24 rows:     MB = 2, last block 8;  RB = 32, KC = 512: 1152 = 512 + 512 + 128, three chunks, the last partial
#   (2, 2, 40)  40 rows:     MB = 3, last block 8;  RB = 48, KC = 256: 640 = 256 + 256 + 128
#   (2, 2, 56)  56 rows:     MB = 4, last block 8;  RB = 64, KC = 256
#   (64, 4, 24) 1 or 2 rows, C = 2048: 128-column tiles (two passes); every other case has 64-column tiles
CASES = [(4, 2, 5, 640, 256), (2, 2, 24, 1152, 256), (2, 2, 40, 640, 256), (2, 2, 56, 640, 256), (64, 4, 24, 640, 2048)]


def _exact_case(E, topk, T, K, C):
    """test_decode_f8g_gpu.py's exact operands in decode_case's form: integer codes, power-of-two scales, one 448 per A
    group at a column where every weight code is zero, so the quantiser's codes and scales are known and every fold is
    exact in any order."""
    n = T * topk
    a_codes, sa, _, _ = ref.operands(n, C, K, True, 3000 + K + T)
    hot = 128 * np.arange(K // 128) + (7 * np.arange(K // 128) + 3) % 128
    a_codes[:, hot] = 0x7E  # 448
    ws = [ref.operands(1, C, K, True, 3001 + K + T + e)[2:] for e in range(E)]
    for b_codes, _ in ws:
        b_codes[:, hot] = 0
    x = (e4m3(a_codes) * np.repeat(sa, 128, axis=1)).astype(np.float16)
    return x, a_codes, sa, ws, [p % E for p in range(n)]


@pytest.mark.parametrize("kind", ["", "cancel", "exact"])
@pytest.mark.parametrize("E,topk,T,K,C", CASES)
def test_tile_entries_bits(E, topk, T, K, C, kind):
    """The quantiser then the down entry alone, bit for bit against gemm_fold_f32 (one slice at every tile width) on
    _f8g128_edges' operands and on the exact ones, whose reference equals its own f64 value; the gate_up entry on the
    edge operands through assert_act_close."""
    case = (E, topk, T, K, C, 1, kind)
    x, a_codes, sa, ws, flat = _exact_case(E, topk, T, K, C) if kind == "exact" else X.decode_case(case)
    ids = (torch.arange(T * topk, dtype=torch.int32) % E).view(T, topk).to(DEV)
    want = np.stack([ref.gemm_fold_f32(a_codes[p:p + 1], sa[p:p + 1], *ws[e])[0] for p, e in enumerate(flat)])
    if kind == "exact":
        f64 = np.stack([ref.gemm(a_codes[p:p + 1], sa[p:p + 1], *ws[e])[0] for p, e in enumerate(flat)])
        assert np.array_equal(want, f64.astype(np.float16)) and np.abs(f64).max() > 0
    df = _layer_of(E, T, topk, K, C, w2=ws)
    _quant(torch.from_numpy(x).to(DEV), df.codes_act, df.scales_act)
    nat.check(nat.symbol(df.ENTRIES[1])(T, topk, E, 0, P(ids), P(df.experts), df.mask2, C, K, 0, P(df.codes_act),
                                        P(df.scales_act), None, None, P(df.y), None, P(df.dev_status), None))
    torch.cuda.synchronize()
    assert np.array_equal(_canon(df.codes_act), a_codes) and np.array_equal(df.scales_act.cpu().numpy(), sa)
    assert not X.mismatch(df.y.cpu().numpy(), want).any() and df.status() == 0
    if kind == "exact":
        return
    N = C // 2
    x, a_codes, sa, ws, flat = X.decode_case((E, topk, T, K, N, 1, kind), gate_up=True)
    tok = [p // topk for p in range(T * topk)]
    gu = np.stack([ref.gemm_fold_f32(a_codes[t:t + 1], sa[t:t + 1], *ws[e])[0] for t, e in zip(tok, flat)])
    df = _layer_of(E, T, topk, N, K, w1=ws)
    _quant(torch.from_numpy(x).to(DEV), df.codes_hidden, df.scales_hidden)
    nat.check(nat.symbol(df.ENTRIES[0])(None, P(df.codes_hidden), P(df.scales_hidden), T, topk, E, 0, P(ids), P(df.experts),
                                        df.mask1, K, N, 0, df.layout, P(df.act), None, P(df.dev_status), None))
    torch.cuda.synchronize()
    act = df.act.cpu().numpy()
    for r in range(len(gu)):
        assert_act_close(act[r:r + 1], gu[r:r + 1], None, "silu", {})
    assert df.status() == 0


def _linear(x, w):
    """fp16 rows through one linear of the layer: the type's contract in float64 [rows, N]."""
    codes, sa = quant_e4m3_g128(x.cpu())
    return ref.gemm(codes.numpy(), sa.numpy(), _canon(w.B), w.scale_b.cpu().numpy().T)


def _check(df, ffn, h, ids=None, wts=None, sw=None, skip=()):
    """One launch, every stage against float64 of its own device input (test_decode_f8g_gpu.py's scheme): act to the
    gated activation of the fp16-rounded g and u, y to the down linear of the device's act, out to the combine of the
    device's y. Pairs in ``skip`` (bad ids) are not compared."""
    got = (df.launch(h) if df.block is not None else df.launch(h, ids, wts, sw)).clone()
    torch.cuda.synchronize()
    if df.block is not None:
        ids, wts, sw = df.gate_out
    (T, topk), E = ids.shape, ffn.E
    h16, flat = h.to(torch.float16).cpu(), ids.view(-1).tolist()
    jobs = [(e, [p for p, x in enumerate(flat) if x == e and p not in skip]) for e in range(E)]
    jobs = [(e, h16[[p // topk for p in ps]], df.act[ps], df.y[ps]) for e, ps in jobs if ps]
    if ffn.has_shared:
        jobs.append((E, h16[:T], df.act_shared[:T], df.ys[:T]))
    for e, x, act, y in jobs:
        gu, act = _linear(x, ffn.w1[e]).astype(np.float16), act.cpu()
        for r in range(len(gu)):
            assert_act_close(act[r:r + 1].numpy(), gu[r:r + 1], None, "silu", {})
        assert_f16_close(y.cpu().numpy(), _linear(act, ffn.w2[e]), ffn.w2[e].K)
    y = df.y[:T * topk].cpu().numpy().copy()
    y[list(skip)] = 0  # (whatever a skipped row holds is weighted in; its token is not compared)
    want = gref.combine_bias(y, np.arange(T * topk), np.array(flat), wts.cpu().numpy(), topk, None, E,
                             df.ys[:T].cpu().numpy() if ffn.has_shared else None, None if sw is None else sw.cpu().numpy())
    ok = [t for t in range(T) if not any(t * topk + k in skip for k in range(topk))]
    out, want = got.float().cpu().numpy()[ok].astype(np.float64), want.astype(np.float64)[ok]
    if got.dtype == torch.bfloat16:  # the f32 sum rounded to bf16 (8 significant bits): half an ulp, up to 2^-8 |ref|
        assert (np.abs(out - want) <= (1e-3 + 2.0 ** -8) * np.abs(want) + 1e-3 * np.sqrt(np.mean(want * want)) + 1e-6).all()
    else:
        assert_f16_close(out, want, ffn.H)
    return got


def _layer(E, H, N, Ns, seed):
    g = torch.Generator().manual_seed(seed)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    return g, moe.MoEFFN(gate_up, down, [(QG, QG)] * (E + (1 if Ns else 0)), num_routed=E)


@pytest.mark.parametrize("H,N", [(128, 384), (640, 256), (1152, 128)])
@pytest.mark.parametrize("T", [1, 17, 40, 64])
def test_against_f64(T, H, N):
    """E = 4, topk = 2, the shared expert with N_shared != N; guard patterns around every buffer."""
    E, topk, Ns = 4, 2, 128 if N != 128 else 256
    g, ffn = _layer(E, H, N, Ns, 3100 + T + H)
    df = moe.DecodeForwardF8gWide(ffn, T, topk)
    bufs = guard(df)
    _check(df, ffn, hidden(g, T, H), *routing(g, T, E, topk))
    for t in bufs:
        assert not (bits(t) == GUARD).all(dim=1).any()
    assert df.status() == 0


@pytest.mark.parametrize("T,H,N", [(20, 640, 256), (26, 640, 256), (64, 8192, 128)])
def test_batches(T, H, N):
    """Every id equal with topk = 4 (RB = 32): T = 20 puts 80 rows on one expert, batches of 32 + 32 + 16; T = 26 puts
    104, 32 + 32 + 32 + 8: a ragged last block behind r0 > 0. H = 8192 at T = 64: KC = 256, the smallest of a row in
    chunks, 32 chunks in gate_up."""
    E, topk = 4, 4
    g, ffn = _layer(E, H, N, 0, 3300 + T + H)
    df = moe.DecodeForwardF8gWide(ffn, T, topk)
    _, wts, _ = routing(g, T, E, topk)
    _check(df, ffn, hidden(g, T, H), torch.full((T, topk), T % E, dtype=torch.int32, device=DEV), wts, None)
    assert df.status() == 0


def test_y_equals_the_eager_layer():
    """On a layer of exact-in-any-order weights (_f8g128_ref.operands(exact=True)), the down stage on the eager layer's
    own act rows gives MoEFFN.forward's y and ys rows bit for bit: one slice and the shared quantiser."""
    E, topk, T, H, N, Ns = 4, 2, 40, 256, 640, 384
    prep = lambda rows, k, seed: moe.prepare_weight_e4m3_g128(  # noqa: E731
        *(torch.from_numpy(t).to(DEV) for t in ref.operands(1, rows, k, True, seed)[2:]))
    w1 = [prep(2 * N, H, 3500 + e) for e in range(E)] + [prep(2 * Ns, H, 3510)]
    w2 = [prep(H, N, 3520 + e) for e in range(E)] + [prep(H, Ns, 3530)]
    ffn = moe.MoEFFN(w1, w2, [(QG, QG)] * (E + 1), num_routed=E)
    g = torch.Generator().manual_seed(3540)
    ids, wts, sw = routing(g, T, E, topk)
    _, mid = ffn.forward(hidden(g, T, H), ids, wts, sw, return_intermediates=True)
    act, act_s = eager_act(ffn, mid)
    inv = mid["routing"].inv_slot.long()
    df = moe.DecodeForwardF8gWide(ffn, T, topk)
    guard(df)
    df.act.copy_(act[inv])
    df.act_shared.copy_(act_s)
    nat.check(nat.symbol("mxmoe_moe_decode_quant_f8g")(nat.DT_FP16, P(df.act), T * topk, N, P(df.codes_act), P(df.scales_act),
                                                       P(df.act_shared), T, Ns, P(df.codes_act_shared),
                                                       P(df.scales_act_shared), None))
    nat.check(nat.symbol(df.ENTRIES[1])(T, topk, E, 1, P(ids), P(df.experts), df.mask2, H, N, Ns, P(df.codes_act),
                                        P(df.scales_act), P(df.codes_act_shared), P(df.scales_act_shared), P(df.y), P(df.ys),
                                        P(df.dev_status), None))
    torch.cuda.synchronize()
    assert mid["y"].abs().max() > 0 and torch.equal(bits(df.y), bits(mid["y"][inv])) and torch.equal(bits(df.ys), bits(mid["ys"]))
    assert df.status() == 0


def test_bf16_block():
    T, E, topk, H = 21, 4, 2, 640
    g, ffn = _layer(E, H, 256, 128, 3400)
    w_gate = torch.randn(E, H, generator=g).to(torch.bfloat16).to(DEV)
    df = moe.DecodeForwardF8gWide(moe.MoEBlock(ffn, w_gate, topk), T)
    got = _check(df, ffn, hidden(g, T, H, dtype=torch.bfloat16))
    assert got.dtype == torch.bfloat16 and df.status() == 0


def test_bad_id_keeps_its_rows():
    T, E, topk = 21, 4, 2
    g, ffn = _layer(E, 128, 384, 256, 3410)
    df = moe.DecodeForwardF8gWide(ffn, T, topk)
    guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    ids[18, 1] = E
    _check(df, ffn, hidden(g, T, 128), ids, wts, sw, skip=(18 * topk + 1,))
    assert (bits(df.act[37]) == GUARD).all() and (bits(df.y[37]) == GUARD).all()
    assert df.status(reset=True) == nat.DECODE_BAD_ID and df.status() == 0


def test_under_a_graph():
    """Captured once, replayed with two routings: every replay equals the uncaptured launch bit for bit."""
    T, E, topk, H = 21, 4, 2, 640
    g, ffn = _layer(E, H, 256, 128, 3420)
    df, other = moe.DecodeForwardF8gWide(ffn, T, topk), moe.DecodeForwardF8gWide(ffn, T, topk)
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
