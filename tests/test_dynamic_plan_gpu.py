"""GPU tests of device planning (DESIGN.md §4 "Device planning / graph forward"): one DynamicGroupGemm planned
once and launched with several device row tables equals the host-planned GroupGemm of the same rows bit for bit;
a MoE layer captured once into a graph (GraphForward) equals the eager layer for every routing it is replayed on.

Why bit for bit: a dynamic launch runs the host plan's kernel on the same tiles (tests/test_dynamic_plan.py), and
every output element's K order is the same in every tile class. The integer types are exact whatever the tiles;
for the float and MX types the shapes here are ones the host planner does not split along K (asserted), and the
quant-type mixes keep both sides on the same kernel build.
"""
from __future__ import annotations

import types

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd import quantize as qz
from mxmoe_amd.groupgemm import (BF16, FP16, W4A4, W4A4_MXFP4, W4A8_MXFP8, W4A16_MXFP4, W8A8, W8A8_E4M3, DynamicGroupGemm,
                                 GroupGemm, Problem, QParams)
from tests._util import assert_f16_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 0x7B7B  # fp16 bit pattern of the guard rows (a finite value no product here produces in bulk)
W4A16 = QParams(16, 4, 128, False)
V2X, V3, WO3 = "v2x_256x256_w8_b3_buf_spread_edma", "v3_256x128_w4_dma_ring3_2wg", "wo3_64x256_w8_3wg"


def variant_index(name: str) -> int:
    for ln in nat.list_variants():
        if ln.split()[1] == name:
            return int(ln.split()[0])
    raise AssertionError(f"variant {name} not compiled")


class Operands:
    """One problem at capacity: A (and its scales) for `cap` rows, the weight, and how many bytes a row takes."""

    def __init__(self, q: QParams, cap: int, N: int, K: int, seed: int, silu: bool):
        g = torch.Generator().manual_seed(seed)
        a = ((torch.rand(cap, K, generator=g) * 2 - 1)).half()
        w = ((torch.rand(N, K, generator=g) * 2 - 1) * 0.2).half()
        self.q, self.cap, self.N, self.K, self.silu = q, cap, N, K, silu
        self.sa = None
        if q.is_fp8:  # (moe.prepare_weight has neither E4M3 nor bf16: B and scale_b built here; no SiLU epilogue)
            qb, sb = qz.quant_e4m3(w)
            self.w = types.SimpleNamespace(B=qz.pack_e4m3(qb).to(DEV), scale_b=sb.to(DEV))
        elif q.fmt == "bf16":
            self.w = types.SimpleNamespace(B=w.bfloat16().to(DEV), scale_b=None)
        else:
            self.w = moe.prepare_weight(w.to(DEV), q, interleave=silu)
        if q.is_fp8:
            qa, sa = qz.quant_e4m3(a)
            self.A, self.sa = qz.pack_e4m3(qa).to(DEV), sa.to(DEV)
        elif q.fmt == "bf16":
            self.A = a.bfloat16().to(DEV)
        elif q.fmt == "MXFP4" and not q.is_weight_only:
            codes, sc = qz.quant_mxfp4(a)
            self.A, self.sa = codes.to(DEV), qz.pack_mxfp4_scales(sc).to(DEV)
        elif q.fmt == "MXFP8":
            codes, sc = qz.quant_mxfp8(a)
            self.A, self.sa = codes.to(DEV), qz.pack_mxfp4_scales(sc).to(DEV)
        elif q.is_quant and not q.is_weight_only:
            qa, sa = qz.quant_rtn_sym(a, q.a_bits)
            self.A, self.sa = qz.pack_wxax(qa, q.a_bits).to(DEV), sa.to(DEV)
        else:
            self.A = a.to(DEV)
        self.a_row = self.A.shape[1] * self.A.element_size()
        self.sa_row = 0 if self.sa is None else (self.sa.numel() // cap) * self.sa.element_size()
        self.cols = N // 2 if silu else N

    def problem(self, C: torch.Tensor, M: int, start: int = 0) -> Problem:
        """The problem on rows [start, start + M) of the operands, writing C."""
        sa = None if self.sa is None else self.sa[start:start + M]
        return Problem(A=self.A[start:start + M], B=self.w.B, C=C, M=M, N=self.N, K=self.K, q=self.q, scale_a=sa,
                       scale_b=self.w.scale_b, silu=self.silu)


# (variant, routed experts' types, shared expert's type, K, SiLU epilogue)
GG_CASES = {
    "wo3_fp16_w8a8_w4a4": (WO3, [FP16, W8A8, W4A4, W8A8], FP16, 256, False),
    "wo3_w4a16_w8a8": (WO3, [W4A16, W8A8, W4A16, W8A8], W8A8, 256, False),
    "wo3_mxfp8": (WO3, [W4A8_MXFP8] * 4, W4A8_MXFP8, 416, False),
    "v2x_mxfp4_w8a8_fp16": (V2X, [W4A4_MXFP4, W8A8, FP16, W4A4_MXFP4], W8A8, 256, False),
    "v3_w4a4": (V3, [W4A4] * 4, W4A4, 256, False),
    "wo3_silu": (WO3, [W8A8, FP16, W4A4, W8A8], FP16, 256, True),
    "v2x_silu": (V2X, [W8A8, FP16, W8A8, FP16], W8A8, 256, True),
    "v2x_e4m3_w8a8": (V2X, [W8A8_E4M3, W8A8, W8A8_E4M3, W8A8], W8A8_E4M3, 256, False),
    "v2x_bf16_fp16": (V2X, [BF16, FP16, BF16, FP16], BF16, 256, False),
}
# rows of the 4 routed experts (sum <= R = 600) and of the shared expert (<= T = 513): tile-boundary values, one
# expert holding all of R, two experts empty
ROW_TABLES = [([64, 65, 127, 257], 129), ([600, 0, 0, 0], 256), ([0, 128, 0, 255], 1), ([1, 63, 129, 256], 513)]
R, T, E = 600, 513, 4


@pytest.mark.parametrize("N", [128, 384])
@pytest.mark.parametrize("case", list(GG_CASES))
def test_one_plan_many_row_tables(case, N):
    """★ Planned once; each row table's launch equals the host-planned GroupGemm of those rows bit for bit and
    leaves the rows past them untouched. The routed experts share one C buffer (rows in slot order, as a MoE
    layer's), their A rows start at a per-launch offset inside each operand store."""
    vname, kinds, shared_kind, K, silu = GG_CASES[case]
    v = variant_index(vname)
    Nw = 2 * N if silu else N  # the SiLU epilogue halves the columns: keep C at N columns
    ops = [Operands(q, R, Nw, K, 100 + i, silu) for i, q in enumerate(kinds)] + [Operands(shared_kind, T, Nw, K, 199, silu)]
    C = torch.empty(R, N, dtype=torch.float16, device=DEV)
    Cs = torch.empty(T, N, dtype=torch.float16, device=DEV)
    dyn = DynamicGroupGemm([o.problem(Cs if i == E else C, o.cap) for i, o in enumerate(ops)], joint=range(E),
                           rows_total=R, variant=v)
    assert dyn.variant == v and dyn.info.splitk_slabs == 0 and dyn.tile_slots == dyn.info.grid
    guard = torch.full((1,), GUARD, dtype=torch.int16, device=DEV).view(torch.float16)
    for rows, rows_shared in ROW_TABLES:
        all_rows = rows + [rows_shared]
        first = np.concatenate([[0], np.cumsum(rows)[:-1]]).tolist() + [0]
        # rows taken from the END of each odd problem's store, from the start of the others: offsets at work
        start = [o.cap - r if i % 2 else 0 for i, (o, r) in enumerate(zip(ops, all_rows))]
        table = [(r, s * o.a_row, s * o.sa_row, 0 if i == E else f * N * 2)
                 for i, (o, r, s, f) in enumerate(zip(ops, all_rows, start, first))]
        C.copy_(guard.expand_as(C))
        Cs.copy_(guard.expand_as(Cs))
        dyn.launch(DynamicGroupGemm.row_table(table, DEV))
        torch.cuda.synchronize()
        got, got_s = C.clone(), Cs.clone()
        C.copy_(guard.expand_as(C))
        Cs.copy_(guard.expand_as(Cs))
        host = GroupGemm([o.problem(Cs[:r] if i == E else C[f:f + r], r, s)
                          for i, (o, r, s, f) in enumerate(zip(ops, all_rows, start, first)) if r], variant=v)
        assert host.info.splitk_slabs == 0  # the bit-identity claim: no K split on the host side either
        host.launch()
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), C.view(torch.int16)), (case, rows)
        assert torch.equal(got_s.view(torch.int16), Cs.view(torch.int16)), (case, rows)
        used = sum(rows)
        assert (got[used:].view(torch.int16) == GUARD).all() and (got_s[rows_shared:].view(torch.int16) == GUARD).all()
        assert not (got[:used].view(torch.int16) == GUARD).all(dim=1).any()  # every planned row was written
    assert dyn.status() == 0


def _block(qcfg, seed, scoring="sigmoid"):
    T_, topk, E_, H, N, Ns = 60, 2, 4, 256, 128, 256
    g = torch.Generator().manual_seed(seed)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half()
    gate_up = [mk(2 * N, H) for _ in range(E_)] + [mk(2 * Ns, H)]
    down = [mk(H, N) for _ in range(E_)] + [mk(H, Ns)]
    ffn = moe.MoEFFN([w.to(DEV) for w in gate_up], [w.to(DEV) for w in down], qcfg, num_routed=E_)
    w_gate = (torch.randn(E_, H, generator=g) * H ** -0.5).half().to(DEV)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).half().to(DEV)
    e_bias = torch.zeros(E_, dtype=torch.float32, device=DEV)
    block = moe.MoEBlock(ffn, w_gate, topk, renormalize=True, w_shared_gate=w_sg, scoring=scoring, e_bias=e_bias)
    hiddens = [torch.randn(T_, H, generator=g).half().to(DEV) for _ in range(3)]
    return block, hiddens, T_


def _captured(gf, static_hidden):
    """GraphForward.launch captured once on a side stream, as one linear chain."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        gf.launch(static_hidden)  # warm-up outside the capture (module loading)
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        gf.launch(static_hidden)
    torch.cuda.current_stream().wait_stream(side)
    return graph


def _replay_against_eager(block, hiddens, T_, exact):
    gf = moe.GraphForward(block, T_)
    static_hidden = torch.zeros_like(hiddens[0])
    static_hidden.copy_(hiddens[0])
    graph = _captured(gf, static_hidden)
    e_bias = block.routing["e_bias"]
    counts_seen = []
    for i, h in enumerate(hiddens):
        e_bias.zero_()
        if i == 2:
            e_bias[1] = -8.0  # sigmoid scores lie in (0, 1): expert 1 is never chosen
        static_hidden.copy_(h)
        graph.replay()
        torch.cuda.synchronize()
        got = gf.out.clone()
        counts_seen.append(gf.route_bufs[3].cpu().tolist())
        want, mid = block.forward(h, return_intermediates=True)
        torch.cuda.synchronize()
        assert counts_seen[-1] == mid["routing"].counts
        if exact:
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), i
        else:
            assert_f16_close(got.cpu().numpy(), want.cpu().numpy(), block.ffn.H)
    assert counts_seen[2][1] == 0 and len({tuple(c) for c in counts_seen}) == 3  # three routings, one starved expert
    assert gf.status() == 0
    return gf


def test_layer_under_a_graph_int_experts():
    """★ A MoEBlock with w8a8 / w4a4 experts, captured once, replayed on three routings (one with an expert at
    zero rows): every replay equals the eager forward bit for bit."""
    qcfg = [(W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8)]
    block, hiddens, T_ = _block(qcfg, 7)
    gf = _replay_against_eager(block, hiddens, T_, exact=True)
    assert gf.mode in ("fused", "interleaved")


def test_layer_under_a_graph_float_experts():
    """The same with fp16, w4a4_g32_sym_MXFP4 and w4a16_g32_sym_MXFP4 experts, within the fp16 tolerance (the
    eager plans may split K or take another kernel build than the capacity plan)."""
    qcfg = [(FP16, FP16), (W4A4_MXFP4, W4A4_MXFP4), (W4A16_MXFP4, W4A16_MXFP4), (FP16, FP16), (W4A4_MXFP4, W4A4_MXFP4)]
    block, hiddens, T_ = _block(qcfg, 11)
    _replay_against_eager(block, hiddens, T_, exact=False)


# the gate_up layouts: (MoEFFN's fuse_silu, its gate_up_mode override, the modes GraphForward may end in)
LAYOUTS = {"default": (None, None, ("fused", "interleaved")), "plain": (False, None, ("plain",)),
           "interleaved": (None, "interleaved", ("interleaved",))}


@pytest.mark.parametrize("T_, layout", [pytest.param(1, "default", id="1"), pytest.param(7, "default", id="7"),
                                        pytest.param(7, "plain", id="7-plain"),
                                        pytest.param(7, "interleaved", id="7-interleaved")])
def test_ffn_with_caller_routing_at_decode_sizes(T_, layout):
    """GraphForward on a plain MoEFFN with the caller's ids and weights (most experts empty), for every gate_up
    layout: the three forwards (eager, planned, graph) give the same bits. The routed rows (N = 128) and the shared
    rows (Ns = 256) differ in width, so the activation pass takes its routed / shared split."""
    topk, E_, H, N, Ns = 2, 4, 256, 128, 256
    fuse, override, modes = LAYOUTS[layout]
    g = torch.Generator().manual_seed(300 + T_)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half().to(DEV)
    qcfg = [(W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8), (W4A4, W4A4), (W8A8, W8A8)]
    ffn = moe.MoEFFN([mk(2 * N, H) for _ in range(E_)] + [mk(2 * Ns, H)], [mk(H, N) for _ in range(E_)] + [mk(H, Ns)],
                     qcfg, num_routed=E_, fuse_silu=fuse)
    ffn.gate_up_mode = override
    gf = moe.GraphForward(ffn, T_, topk)
    assert gf.mode in modes
    for _ in range(2):  # two routings through the same plan
        ids = torch.stack([torch.randperm(E_, generator=g)[:topk] for _ in range(T_)]).to(torch.int32).to(DEV)
        wts = torch.softmax(torch.rand(T_, topk, generator=g), dim=1).to(DEV)
        sw = torch.rand(T_, generator=g).to(DEV)
        h = torch.randn(T_, H, generator=g).half().to(DEV)
        got = gf.launch(h, ids, wts, sw).clone()
        want = ffn.forward(h, ids, wts, sw)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        # a PlannedForward takes no shared_w (the shared expert at weight 1): the three forwards without it
        pf = moe.PlannedForward(ffn, h, ids, wts)
        assert pf.mode in modes
        planned = pf().clone()
        got = gf.launch(h, ids, wts).clone()
        want = ffn.forward(h, ids, wts)
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        assert torch.equal(planned.view(torch.int16), want.view(torch.int16))
    assert gf.status() == 0
    with pytest.raises(ValueError):
        gf.launch(h, ids.long(), wts, sw)  # nothing may be converted under capture: the dtypes are the caller's
