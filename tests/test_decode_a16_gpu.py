"""GPU tests of the decode forward on the fp16 MFMA (moe.DecodeForwardA16; mxmoe_moe_decode_gate_up_a16 /
mxmoe_moe_decode_down_a16, DESIGN.md §4 "Decode forward: fp16 activations on MFMA"). The reference is the contract in
float64, v(r) = fp16(sum_k x[k] * b[r][k]), with b read back from the layer's own prepared tensors (``_deq``). On grid
data (multiples of 1/4 in [-1, 1], power-of-two scales) every f32 partial sum is exact in any order: down, run alone on
grid activations, equals DecodeForwardWo's y and the float64 value bit for bit; the gated activation's rcp / exp2 have no
float64 restatement, so gate_up is held to DecodeForwardWo's act bit for bit (itself held to the eager layer)."""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe, quantize
from mxmoe_amd.groupgemm import FP16, W4A16_ASYM, W4A16_G128_ASYM, W4A16_MXFP4, W8A8, QParams
from tests import _gptoss_ref as gref
from tests._decode_util import DEV, GUARD, biases, bits, f16_weights, guard, hidden, routing
from tests._util import assert_f16_close
from tests.test_decode_wo_gpu import _grid_weight

pytestmark = pytest.mark.gpu
KINDS = {"fp16": FP16, "mx": W4A16_MXFP4, "w4a16": QParams(16, 4, -1, True), "w8a16_g128": QParams(16, 8, 128, True),
         "w4a16_g128_asym": W4A16_G128_ASYM, "scheme": None}
SCHEME = [(W4A16_ASYM, W8A8), (W8A8, W4A16_ASYM), (W4A16_ASYM, W4A16_ASYM), (W8A8, W8A8), (W4A16_ASYM, W4A16_ASYM)]
E, H, N, NS = 4, 384, 128, 256  # H = 384: three K groups of 128, a second g128 scale group


def _deq(w):
    """b[r][k] of a prepared weight as fp16 [rows, K] (host), rows as stored"""
    q = w.q
    if not q.is_quant:
        return w.B.cpu()
    if q.fmt:
        return quantize.dequant_mxfp4(w.B.cpu(), quantize.unpack_mxfp4_scales(w.scale_b.cpu(), w.K)).half()
    return quantize.dequant_weightonly(quantize.unpack_weightonly_mi355x(w.B.cpu(), q.w_bits, w.K), w.scale_b.cpu(), q.w_bits,
                                       q.gsize, q.sym)


@functools.lru_cache(maxsize=None)
def _layer(kind, grid=True, fuse=False, e=E, h=H, n=N, ns=NS):
    """grid: every weight a value its quantiser reproduces, every product a multiple of 2^-8 (asserted exact below)"""
    g = torch.Generator().manual_seed(900 + sum(map(ord, kind)) + h)
    nexp = e + (1 if ns else 0)
    qcfg = SCHEME[:nexp] if kind == "scheme" else [(KINDS[kind],) * 2] * nexp
    if grid and kind not in ("fp16", "mx"):
        shapes = [(2 * n, h)] * e + [(2 * ns, h)] * (nexp - e) + [(h, n)] * e + [(h, ns)] * (nexp - e)
        qs = [p[0] for p in qcfg] + [p[1] for p in qcfg]  # (a w8a8 linear quantises the w4a16 grid's weights)
        ws = [_grid_weight(g, r, k, q if q.is_weight_only else W4A16_ASYM) for (r, k), q in zip(shapes, qs)]
        assert max(h, n, ns) * 4 * max(b for _, b in ws) < 2 ** 24  # K * (max|x| / (1/4)) * (max|b| / 2^-6)
        ws = [w for w, _ in ws]
    else:
        ws = sum(f16_weights(g, e, h, n, ns, grid=grid), [])
    return moe.MoEFFN(ws[:nexp], ws[nexp:], qcfg, num_routed=e, fuse_silu=fuse)


def _down(df, T, ids, act, act_s):
    """the class's down entry alone, on the caller's activations"""
    f, p = df.ffn, lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
    nat.check(nat.symbol(df.ENTRIES[1])(T, df.topk, f.E, int(f.has_shared), p(ids), p(df.experts), df.mask2, f.H, f.N, f.Ns,
                                        p(act), p(act_s), p(df.y), p(df.ys), p(df.dev_status), None))
    torch.cuda.synchronize()


def _down_f64(ffn, ids, act, act_s):
    """y and ys of the contract in float64, unrounded; the rows of experts with quantised activations are None"""
    ws = [None if w.q.a_bits != 16 else _deq(w).double() for w in ffn.w2]
    y = [None if ws[e] is None else act[p].cpu().double() @ ws[e].T for p, e in enumerate(ids.view(-1).tolist())]
    return y, (act_s.cpu().double() @ ws[ffn.E].T if ffn.has_shared else None)


def _exact(ffn, T, topk, ids, seed):
    g = torch.Generator().manual_seed(seed)
    a16, wo = moe.DecodeForwardA16(ffn, T, topk), moe.DecodeForwardWo(ffn, T, topk)
    guard(a16), guard(wo)
    wts, sw = routing(g, T, ffn.E, topk)[1:]
    h = hidden(g, T, ffn.H, grid=True, step=4, bound=1)
    a16.launch(h, ids, wts, sw if ffn.has_shared else None), wo.launch(h, ids, wts, sw if ffn.has_shared else None)
    torch.cuda.synchronize()
    assert torch.equal(bits(a16.act), bits(wo.act)), "gate_up (routed act)"
    assert not ffn.has_shared or torch.equal(bits(a16.act_shared), bits(wo.act_shared)), "gate_up (shared act)"
    n = T * topk
    act = hidden(g, n, ffn.N, grid=True, step=4, bound=1)
    act_s = hidden(g, T, ffn.Ns, grid=True, step=4, bound=1) if ffn.has_shared else None
    _down(a16, T, ids, act, act_s), _down(wo, T, ids, act, act_s)
    assert torch.equal(bits(a16.y), bits(wo.y)), "down (routed y)"
    y64, ys64 = _down_f64(ffn, ids, act, act_s)
    for p, want in enumerate(y64):
        assert want is None or torch.equal(bits(a16.y[p].cpu()), bits(want.float().half())), f"down (y[{p}] against float64)"
    if ffn.has_shared:
        assert torch.equal(bits(a16.ys), bits(wo.ys)) and torch.equal(bits(a16.ys.cpu()), bits(ys64.float().half())), "down (ys)"
    assert a16.status() == 0 == wo.status()
    return a16


def _ids(T, topk):
    """expert 0 takes every token (more than the VALU form's 5-row batch from T = 6), expert 3 none"""
    return torch.tensor([[0, 1 + (t & 1)][:topk] for t in range(T)], dtype=torch.int32, device=DEV)


@pytest.mark.parametrize("T", [1, 5, 16])
@pytest.mark.parametrize("fuse", [False, True], ids=["plain", "interleaved"])
@pytest.mark.parametrize("kind", list(KINDS))
def test_exact_stage_by_stage(kind, fuse, T):
    """1. E = 4 and the shared expert, topk = 2, H = 384, N = 128, Ns = 256: 32-column tiles, two K slices. The scheme's
    w8a8 experts run the carried-over integer path in the same launch and are held to DecodeForwardWo's bytes."""
    _exact(_layer(kind, fuse=fuse), T, 2, _ids(T, 2), 910 + T)


def test_sixteen_rows_on_one_expert():
    _exact(_layer("w4a16"), 16, 1, torch.full((16, 1), 2, dtype=torch.int32, device=DEV), 920)


@pytest.mark.parametrize("kind,h,ns", [("w4a16", 128, 5632), ("fp16", 8192, 0), ("fp16", 16384, 0)])
def test_k_chunks_and_wide_tiles(kind, h, ns):
    """2. Rows that do not fit LDS whole at T = 16. Ns = 5632 (44 K groups): the shared down runs 11 chunks of 4 groups,
    each split over two K slices (H = 128: 32-column tiles). H = 8192 / 16384 with E = 8: gate_up runs 16 / 32 chunks,
    and down has 64- / 128-column tiles (one slice; two column groups per wave at 128)."""
    e = 8 if ns == 0 else 2
    ffn = _layer(kind, e=e, h=h, ns=ns)
    ids = torch.arange(16 * 2, dtype=torch.int32, device=DEV).view(16, 2) % e
    _exact(ffn, 16, 2, ids, 930 + h)


@pytest.mark.parametrize("kind", ["fp16", "mx", "w4a16_g128_asym"])
def test_random_data(kind):
    """3. randn hidden states, weights uniform in +-0.2, T = 16: y against the float64 down of the kernel's own act, out
    against the whole layer in float64 (every stage rounded to fp16 once), with the suite's fp16 tolerance."""
    ffn, T, topk = _layer(kind, grid=False), 16, 2
    g = torch.Generator().manual_seed(940)
    df = moe.DecodeForwardA16(ffn, T, topk)
    ids, wts, sw = routing(g, T, E, topk)
    h = hidden(g, T, H)
    out = df.launch(h, ids, wts, sw).clone()
    torch.cuda.synchronize()
    y64, ys64 = _down_f64(ffn, ids, df.act, df.act_shared)
    assert_f16_close(df.y.float().cpu().numpy(), torch.stack(y64).numpy(), N)
    assert_f16_close(df.ys.float().cpu().numpy(), ys64.numpy(), NS)
    f16 = lambda t: t.numpy().astype(np.float16)
    flat, h64 = ids.view(-1).tolist(), h.cpu().double()
    act = np.concatenate([gref.glu(f16(h64[p // topk:p // topk + 1] @ _deq(ffn.w1[e]).double().T)) for p, e in enumerate(flat)])
    act_s = gref.glu(f16(h64 @ _deq(ffn.w1[E]).double().T))
    y = np.stack([f16(torch.from_numpy(act[p]).double() @ _deq(ffn.w2[e]).double().T) for p, e in enumerate(flat)])
    ys = f16(torch.from_numpy(act_s).double() @ _deq(ffn.w2[E]).double().T)
    want = (wts.cpu().double().numpy()[:, :, None] * y.reshape(T, topk, H).astype(np.float64)).sum(1) + \
        sw.cpu().double().numpy()[:, None] * ys.astype(np.float64)
    assert_f16_close(out.float().cpu().numpy(), want, H)
    assert df.status() == 0


def test_bf16_block_with_biases_and_clamp():
    """4a. test_decode_wo_gpu.py::test_bf16_ends's construction: a bf16 MoEBlock over exact w4a16 gate_ups and w8a8 downs
    with biases and the clamped SwiGLU — every stage exact or integer, so out equals block.forward bit for bit."""
    T, topk, bf = 16, 2, torch.bfloat16
    g = torch.Generator().manual_seed(950)
    _, down = f16_weights(g, E, H, N, NS)
    gate_up = [_grid_weight(g, 2 * n, H, W4A16_ASYM)[0] for n in [N] * E + [NS]]
    b1, b2 = biases(g, E, H, N, NS)
    ffn = moe.MoEFFN(gate_up, down, [(W4A16_ASYM, W8A8)] * (E + 1), num_routed=E, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(bf).to(DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=(torch.randn(H, generator=g) * H ** -0.5).to(bf).to(DEV))
    df = moe.DecodeForwardA16(block, T, dtype=bf)
    h = hidden(g, T, H, grid=True, dtype=bf, step=4, bound=1)
    got = df.launch(h).clone()
    want = block.forward(h)
    torch.cuda.synchronize()
    assert got.dtype == bf and torch.equal(bits(got), bits(want)) and df.status() == 0


def test_block_under_a_graph():
    """4b. A MoEBlock over the scheme captured once and replayed on two hidden states with different routings: each
    replay equals the uncaptured launch bit for bit."""
    T, topk = 7, 2
    g = torch.Generator().manual_seed(960)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).half().to(DEV)
    block = moe.MoEBlock(_layer("scheme", grid=False), w_gate, topk, renormalize=True)
    df, ref = moe.DecodeForwardA16(block, T), moe.DecodeForwardA16(block, T)
    static_hidden, side, graph, seen = hidden(g, T, H), torch.cuda.Stream(), torch.cuda.CUDAGraph(), []
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        df.launch(static_hidden)  # warm-up outside the capture (module loading)
    side.synchronize()
    with torch.cuda.graph(graph, stream=side):
        df.launch(static_hidden)
    torch.cuda.current_stream().wait_stream(side)
    for h in [hidden(g, T, H) for _ in range(2)]:
        static_hidden.copy_(h)
        graph.replay()
        ref.launch(h)
        torch.cuda.synchronize()
        for a, b in ((df.gate_out[0], ref.gate_out[0]), (df.act, ref.act), (df.y, ref.y), (df.out, ref.out)):
            assert torch.equal(a, b)
        seen.append(df.gate_out[0].clone())
    assert not torch.equal(seen[0], seen[1]) and df.status() == 0


def test_bad_id_and_kind_outside_the_mask():
    """5. An id of E and an id of -1: their pairs' rows keep the guard and status() is DECODE_BAD_ID. A mask that names
    w8a8 only on the scheme's layer: the other records set DECODE_BAD_KIND and their rows keep the guard."""
    ffn, T, topk = _layer("scheme", grid=False), 7, 2
    g = torch.Generator().manual_seed(970)
    df = moe.DecodeForwardA16(ffn, T, topk)
    guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    ids[2, 0], ids[5, 1] = E, -1
    df.launch(hidden(g, T, H), ids, wts, sw)
    torch.cuda.synchronize()
    bad = [2 * topk, 5 * topk + 1]
    for t in (df.act, df.y):
        assert (bits(t[bad]) == GUARD).all() and not (bits(t[[p for p in range(T * topk) if p not in bad]]) == GUARD).all(dim=1).any()
    assert df.status(reset=True) == nat.DECODE_BAD_ID
    df.mask1 = df.mask2 = 1 << nat.DECODE_W8A8
    guard(df)
    ids = routing(g, T, E, topk)[0]
    df.launch(hidden(g, T, H), ids, wts, sw)
    torch.cuda.synchronize()
    for buf, lin in ((df.act, 0), (df.y, 1)):
        for p, e in enumerate(ids.view(-1).tolist()):
            assert (not (bits(buf[p]) == GUARD).all()) == (SCHEME[e][lin] is W8A8), (p, e, lin)
    assert (bits(df.act_shared) == GUARD).all() and df.status() == nat.DECODE_BAD_KIND
