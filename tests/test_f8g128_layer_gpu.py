"""GPU tests of the MXMOE_ACT_E4M3_G128 activation tag (bit for bit against quantize.quant_e4m3_g128, through the
gather and through mxmoe_moe_glu_quant) and of MoE layers with w8a8_g128_sym_E4M3 experts: eager stage by stage against
the f64 reference of tests/_f8g128_ref.py, PlannedForward and a replayed GraphForward bit for bit against eager."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W8A8_E4M3, W8A8_G128_E4M3
from mxmoe_amd.quantize import pack_e4m3, quant_e4m3_g128, unpack_wxax
from tests import _f8g128_ref as ref
from tests._util import assert_f16_close
from tests.test_f8g128 import _special_groups

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
G8, F = moe.ACT_E4M3_G128, moe.ACT_FP16
QG = W8A8_G128_E4M3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _check_batch(a, seg_rows, what):
    """Every E4M3_G128 segment of an ActBatch against quant_e4m3_g128 of its fp16 rows: codes and f32 scales, bit for bit."""
    for e, rows in enumerate(seg_rows):
        if a.qtags[e] != G8 or len(rows) == 0:
            continue
        codes, sc = quant_e4m3_g128(torch.as_tensor(rows))
        assert torch.equal(a.A(e).cpu(), pack_e4m3(codes)), (what, e, "codes")
        assert np.array_equal(a.scale(e).cpu().numpy(), sc.t().reshape(-1).numpy(), equal_nan=True), (what, e, "scales")


def _segments(t, r):
    return [t[r.first_slot[e]:r.first_slot[e] + r.counts[e]] for e in range(r.E)]


@pytest.mark.parametrize("W", [128, 384, 2944])
def test_tag_against_quant_e4m3_g128(W):
    T, E, topk = 12, 3, 2
    g = torch.Generator().manual_seed(W)
    h = torch.randn(T, W, generator=g).half() * 3
    sp = torch.from_numpy(_special_groups())  # [6, 256]: zero, 65504, ties, subnormals, Inf and NaN groups
    h[:6, :128], h[6:, W - 128:] = sp[:, :128], sp[:, 128:]
    ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
    r = moe.route(ids, E)
    perm = r.perm_token.cpu()
    a = moe.quant_act(h.to(DEV), r, [G8] * E, False)
    torch.cuda.synchronize()
    _check_batch(a, _segments(h[perm].numpy(), r), "gather")
    # through mxmoe_moe_glu_quant: [gate | up] rows with a bias, the same pass with fp16 tags as the input of the rule
    gu = torch.cat([h[perm], torch.randn(T * topk, W, generator=g).half()], dim=1).to(DEV)
    bias = (torch.rand(E, 2 * W, generator=g) - 0.5).half().to(DEV)
    got = moe.glu_quant(gu, None, r, [G8] * E, moe.SwigluClamp(), bias)
    act = moe.glu_quant(gu, None, r, [F] * E, moe.SwigluClamp(), bias)
    torch.cuda.synchronize()
    _check_batch(got, [act.A(e).cpu().numpy() for e in range(E)], "glu_quant")


def _check_gemm(a, ws, C_of, what):
    """The new type's GroupGEMM outputs against the f64 reference on the device's own A operands."""
    for e, w in enumerate(ws):
        rows = a.segs[e].rows
        if rows == 0 or w.q != QG:
            continue
        G = w.K // 128
        dec = lambda t: unpack_wxax(t.cpu(), 8, w.K).numpy().view(np.uint8)  # noqa: E731
        want = ref.gemm(dec(a.A(e)), a.scale(e).cpu().numpy().reshape(G, rows).T, dec(w.B), w.scale_b.cpu().numpy().T)
        assert_f16_close(C_of(e).cpu().numpy(), want, w.K)


MIX = [(QG, QG), (W8A8_E4M3, QG), (FP16, FP16), (QG, W8A8_E4M3), (QG, FP16), (FP16, QG), (QG, QG), (W8A8_E4M3, W8A8_E4M3)]


@pytest.mark.parametrize("T", [3, 64])
@pytest.mark.parametrize("qcfg", [[(QG, QG)] * 8, MIX], ids=["all", "mix"])
def test_layer_eager_planned_graph(qcfg, T):
    E, topk, H, N = 8, 2, 256, 128
    g = torch.Generator().manual_seed(5 + T)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)  # noqa: E731
    ffn = moe.MoEFFN([mk(2 * N, H) for _ in range(E)], [mk(H, N) for _ in range(E)], qcfg, num_routed=E)
    assert not ffn.fuse_silu and ffn.tag1 == [moe.act_tag(q[0]) for q in qcfg]
    gf = moe.GraphForward(ffn, T, topk)
    for rep in range(2):
        h = torch.randn(T, H, generator=g).half().to(DEV)
        ids = torch.stack([torch.randperm(E, generator=g)[:topk] for _ in range(T)]).to(torch.int32).to(DEV)
        wts = torch.softmax(torch.rand(T, topk, generator=g), dim=1).to(DEV)
        out, mid = ffn.forward(h, ids, wts, return_intermediates=True)
        torch.cuda.synchronize()
        r = mid["routing"]
        _check_batch(mid["a1"], _segments(h.cpu().numpy()[r.perm_token.cpu().numpy()], r), "a1")
        _check_gemm(mid["a1"], ffn.w1, lambda e: _segments(mid["h1"], r)[e], "h1")
        act = moe.silu_mul_quant(mid["h1"], None, r, [F] * E)
        torch.cuda.synchronize()
        _check_batch(mid["a2"], [act.A(e).cpu().numpy() for e in range(E)], "a2")
        _check_gemm(mid["a2"], ffn.w2, lambda e: _segments(mid["y"], r)[e], "y")
        assert torch.equal(moe.PlannedForward(ffn, h, ids, wts)(), out)
        assert torch.equal(gf.launch(h, ids, wts), out), rep  # (the second pass replays the plan on another routing)
    assert gf.status() == 0
