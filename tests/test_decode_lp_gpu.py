"""GPU tests of the decode forward on MFMA (moe.DecodeForwardLp; mxmoe_moe_decode_gate_up_lp / mxmoe_moe_decode_down_lp,
DESIGN.md §4 "Decode forward on MFMA"): E4M3, MXFP8 and MXFP4 activation experts in a layer call of 1..16 tokens.

Every stage is held to a float64 reference of its own input: act to the layer's dequantised gate_up weights on
hidden quantised by quantize.quant_e4m3 / quant_mxfp8 / quant_mxfp4 (g and u rounded to fp16, then the gated
activation), y to the dequantised down weights on the device's own act quantised the same way, out to the combine of
the device's own y — within tests/_util.assert_f16_close, the figure MoEFFN.forward is held to for these types
(tests/test_e4m3_layer_gpu.py, test_mxfp8_a8_gpu.py, test_mxfp4_gpu.py; for act, which lies behind the activation, that
figure on g and u carried through it: _assert_act_close). act is also compared with the eager layer's
own activation rows: the A codes are the activation pass's."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import W4A4_MXFP4, W4A8_MXFP8, W4A16_ASYM, W8A8, W8A8_E4M3
from tests import _gptoss_ref as gref
from tests._decode_util import DEV, GUARD, assert_act_close as _assert_act_close, biases, bits, eager_act, f16_weights, guard, hidden, \
    mx_codes, routing
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
MIXED = [(W8A8_E4M3, W4A8_MXFP8), (W4A8_MXFP8, W4A4_MXFP4), (W4A4_MXFP4, W8A8_E4M3), (W8A8, W4A16_ASYM), (W4A16_ASYM, W8A8)]
KINDS = {"e4m3": [(W8A8_E4M3, W8A8_E4M3)], "mxfp8": [(W4A8_MXFP8, W4A8_MXFP8)], "mxfp4": [(W4A4_MXFP4, W4A4_MXFP4)],
         "mixed": MIXED}


def _a64(x, q):
    """The A operand the type's activation tag defines, float64 (the per-row types: codes, and the row scales apart)."""
    if q.fmt == "E4M3":
        c, s = qz.quant_e4m3(x)
        return c.view(torch.float8_e4m3fn).double(), s
    if q.fmt in ("MXFP8", "MXFP4") and q.a_bits < 16:
        return (qz.dequant_mxfp8(*qz.quant_mxfp8(x)) if q.a_bits == 8 else qz.dequant_mxfp4(*qz.quant_mxfp4(x))), None
    if q.a_bits == 16:
        return x.double(), None
    c, s = qz.quant_rtn_sym(x, q.a_bits)
    return c.double(), s


def _w64(w):
    """The layer's own weight dequantised, float64 [rows, K] (the per-row types: codes, and the row scales apart)."""
    B, q = w.B.cpu(), w.q
    sb = None if w.scale_b is None else w.scale_b.cpu()
    if not q.is_quant:
        return B.double(), None
    if q.fmt in ("MXFP4", "MXFP8"):
        return qz.dequant_mxfp4(B, qz.unpack_mxfp4_scales(sb, w.K)), None
    if q.is_weight_only:
        return qz.dequant_weightonly(qz.unpack_weightonly_mi355x(B, q.w_bits, w.K), sb, q.w_bits, q.gsize, q.sym).double(), None
    c = qz.unpack_wxax(B, q.w_bits, w.K)
    return (c.view(torch.uint8).view(torch.float8_e4m3fn) if q.is_fp8 else c).double(), sb


def _linear(x, w):
    """fp16 rows through one linear of the layer: the type's contract in float64, one rounding to fp16."""
    (a, sa), (b, sb) = _a64(x.cpu(), w.q), _w64(w)
    c = a @ b.t()
    if sa is not None:
        c = c * (sa[:, None] * sb[None, :]).double()  # fp16_rn(scale_a * scale_b), as the epilogue forms it
    return c.half()


def _check(df, ffn, h, ids, wts, sw, skip=()):
    """One launch, stage by stage; pairs in ``skip`` (ids outside [0, E)) are not compared."""
    T, topk = ids.shape
    n, E = T * topk, ffn.E
    got = df.launch(h, ids, wts, sw).clone()
    torch.cuda.synchronize()
    h16, flat = h.to(torch.float16), ids.view(-1).tolist()
    act_fn = "silu" if ffn.activation == "silu" else "clamp"
    glu = {} if act_fn == "silu" else dict(alpha=ffn.activation.alpha, limit=ffn.activation.limit)
    rows = [(p, e, h16[p // topk:p // topk + 1], df.act[p:p + 1], df.y[p]) for p, e in enumerate(flat) if p not in skip]
    if ffn.has_shared:
        rows += [(None, E, h16[t:t + 1], df.act_shared[t:t + 1], df.ys[t]) for t in range(T)]
    for p, e, x, act, y in rows:
        w1, w2 = ffn.w1[e], ffn.w2[e]
        gu = _linear(x, w1)
        N = w2.K
        if ffn.fuse_silu:  # gate row n at 32 (n / 16) + n % 16, its up row 16 further
            idx = torch.arange(N)
            idx = 32 * (idx // 16) + idx % 16
            gu = torch.cat([gu[:, idx], gu[:, idx + 16]], dim=1)
        b1 = None if ffn.b1 is None else (ffn.b1s if e == E else ffn.b1[e]).cpu().numpy()
        _assert_act_close(act.cpu().numpy(), gu.numpy(), b1, act_fn, glu)
        assert_f16_close(y.cpu().numpy()[None], _linear(act, w2).numpy(), w2.K)
    y = df.y[:n].cpu().numpy().copy()
    for p in skip:
        y[p] = 0  # (whatever the row holds is weighted in; the test compares the tokens without a bad id)
    b2 = None if ffn.b2 is None else ffn.b2.cpu().numpy()
    want = gref.combine_bias(y, np.arange(n), np.array(flat), wts.cpu().numpy(), topk, b2, E,
                             df.ys[:T].cpu().numpy() if ffn.has_shared else None, None if sw is None else sw.cpu().numpy(),
                             None if ffn.b2 is None or not ffn.has_shared else ffn.b2s.cpu().numpy())
    ok = [t for t in range(T) if not any(t * topk + k in skip for k in range(topk))]
    out, ref = got.float().cpu().numpy()[ok].astype(np.float64), want.astype(np.float64)[ok]
    if got.dtype == torch.bfloat16:  # the f32 sum rounded to bf16 (8 significant bits): half an ulp, up to 2^-8 |ref|
        rms = np.sqrt(np.mean(ref * ref))
        assert (np.abs(out - ref) <= (1e-3 + 2.0 ** -8) * np.abs(ref) + 1e-3 * rms + 1e-6).all()
    else:
        assert_f16_close(out, ref, ffn.H)
    return got


def _layer(name, E, H, N, Ns, seed, fuse=None, **kw):
    g = torch.Generator().manual_seed(seed)
    gate_up, down = f16_weights(g, E, H, N, Ns)
    qcfg = [KINDS[name][e % len(KINDS[name])] for e in range(E + (1 if Ns else 0))]
    return g, moe.MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=fuse, **kw)


# (H, N): one K step and a column count that is no multiple of 128; five K steps (the row ends inside the group of
# steps in flight) — in both linears, as down's K is N
@pytest.mark.parametrize("H,N", [(128, 384), (640, 256)])
@pytest.mark.parametrize("T", [1, 5, 16])
@pytest.mark.parametrize("name,fuse", [("e4m3", False), ("mxfp8", True), ("mxfp8", False), ("mxfp4", False), ("mixed", False)])
def test_against_f64(name, fuse, T, H, N):
    """★ fails without the feature (no class, no entries). E = 4, topk = 2, the shared expert with N_shared != N; the
    routed act also against the eager layer's activation rows."""
    E, topk, Ns = 4, 2, 128 if N != 128 else 256
    g, ffn = _layer(name, E, H, N, Ns, 900 + T + H, fuse)
    assert ffn.fuse_silu == fuse
    df = moe.DecodeForwardLp(ffn, T, topk)
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


@pytest.mark.parametrize("name", list(KINDS))
def test_more_than_one_batch(name):
    """topk = 4 on E = 4 (the entries need topk <= E) with every id equal: T = 16 puts 64 rows on one expert, four
    batches; T = 5 puts 20, the last batch partial."""
    E, topk = 4, 4
    for T, e in ((16, 1), (5, 3)):
        g, ffn = _layer(name, E, 640, 256, 0, 930 + T)
        df = moe.DecodeForwardLp(ffn, T, topk)
        _, wts, _ = routing(g, T, E, topk)
        _check(df, ffn, hidden(g, T, 640), torch.full((T, topk), e, dtype=torch.int32, device=DEV), wts, None)
        assert df.status() == 0


def test_bf16_ends():
    """A bf16 call of the mixed layer: hidden converted as it is loaded (the reference: hidden.to(fp16)), out bf16."""
    T, E, topk = 5, 4, 2
    g, ffn = _layer("mixed", E, 640, 256, 128, 940)
    df = moe.DecodeForwardLp(ffn, T, topk, dtype=torch.bfloat16)
    ids, wts, sw = routing(g, T, E, topk)
    got = _check(df, ffn, hidden(g, T, 640, dtype=torch.bfloat16), ids, wts, sw)
    assert got.dtype == torch.bfloat16 and df.status() == 0


def test_gptoss_style_mxfp8_layer():
    """Checkpoint-style MXFP4 tensors (random codes, scale bytes 118..126) with the four biases and the clamped SwiGLU,
    MXFP8 activations: prepare_weight_mx's operands read in place, the bias and the clamp in the gate_up epilogue."""
    T, E, topk, H, N = 5, 4, 2, 640, 256
    g = torch.Generator().manual_seed(950)
    ws = [[moe.prepare_weight_mx(*(t.to(DEV) for t in mx_codes(g, rows, K, 118, 126)), W4A8_MXFP8) for _ in range(E)]
          for rows, K in ((2 * N, H), (H, N))]
    b1, b2 = biases(g, E, H, N, 0)
    ffn = moe.MoEFFN(ws[0], ws[1], [(W4A8_MXFP8, W4A8_MXFP8)] * E, num_routed=E, gate_up_bias=b1, down_bias=b2,
                     activation=moe.SwigluClamp())
    df = moe.DecodeForwardLp(ffn, T, topk)
    assert df._glu is not None and df.mask1 == 1 << nat.DECODE_W4A8_MXFP8
    ids, wts, _ = routing(g, T, E, topk)
    _check(df, ffn, hidden(g, T, H), ids, wts, None)
    assert df.status() == 0


def test_bad_id_keeps_its_rows():
    T, E, topk = 5, 4, 2
    g, ffn = _layer("mixed", E, 128, 384, 256, 960)
    df = moe.DecodeForwardLp(ffn, T, topk)
    guard(df)
    ids, wts, sw = routing(g, T, E, topk)
    ids[2, 1] = E
    _check(df, ffn, hidden(g, T, 128), ids, wts, sw, skip=(2 * topk + 1,))
    assert (bits(df.act[5]) == GUARD).all() and (bits(df.y[5]) == GUARD).all()
    assert df.status(reset=True) == nat.DECODE_BAD_ID and df.status() == 0


def test_under_a_graph():
    """Captured once, replayed with two routings: every replay equals the uncaptured launch bit for bit."""
    T, E, topk, H = 5, 4, 2, 640
    g, ffn = _layer("mixed", E, H, 256, 128, 970)
    df, ref = moe.DecodeForwardLp(ffn, T, topk), moe.DecodeForwardLp(ffn, T, topk)
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
        want = ref.launch(*call).clone()
        torch.cuda.synchronize()
        for a, b in ((df.act, ref.act), (df.y, ref.y), (df.out, want)):
            assert torch.equal(bits(a), bits(b))
    assert not torch.equal(calls[0][1], calls[1][1]) and df.status() == 0
