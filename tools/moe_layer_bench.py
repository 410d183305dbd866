"""One qwen2_moe layer-11 MoE FFN step at bs=8192 (LP-1 mixed w4a4 + w8a8 qconfig, routed histogram of
the committed workload, random weights) on the device, unfused (silu_mul_quant) against the fused
SiLU epilogue (MXMOE_GG_EPI_SILU_MUL + quant_slots): moe_bench.qwen2_layer_bench — per-stage and step
times, outputs checked bit-identical.

python tools/moe_layer_bench.py [--rounds 4] [--iters 30] > gpurun_out/moe_layer.json

--dtype bf16 [--bs 128 8192]: bf16_layer_bench (below) instead — the bf16 MoEBlock against the cast wrap around the fp16
block (hidden.to(fp16) -> layer -> out.to(bf16)), eager GraphForward launches and captured-graph replays, one JSON
line per batch size.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from mxmoe_amd import moe_bench  # noqa: E402


def bf16_layer_bench(batches=(128, 8192), rounds: int = 4, iters: int = 20):
    """A bf16 model's qwen2_moe layer 11 (LP-1 mixed w4a4 + w8a8 qconfig, random weights, the router with its shared
    gate) at every batch size of ``batches`` (yields one dict each), two ways in one process with the sides alternating
    over rounds:
      native  the bf16 ``MoEBlock``: GraphForward.launch(hidden bf16) -> out bf16;
      wrap    what a bf16 caller had to do around the fp16 layer: hidden.to(fp16) -> the fp16 block -> out.to(bf16)
              (two cast kernels on preallocated buffers, so both sides can be captured).
    Each as eager ``GraphForward.launch`` calls and as a captured-graph replay: device time (events around ``iters``
    back-to-back runs) and wall time per run with a synchronise. Per side the median of the rounds' medians with
    min / max (us), and native / wrap ratios."""
    from mxmoe_amd.groupgemm import QParams
    from mxmoe_amd.moe import GraphForward, MoEBlock, MoEFFN
    from mxmoe_amd.moe_bench import _captured, _device, _rounds, _stat, _wall
    from mxmoe_amd.workload import load_workload, mixed_qconfig_lp1, qwen2_layer11_workload

    shapes, topk = load_workload(qwen2_layer11_workload(8192, qconfig=mixed_qconfig_lp1()))["layer-11"], 4
    E = len(shapes["gate_up"]) - 1
    H = shapes["gate_up"][0].K
    N, Ns = shapes["down"][0].K, shapes["down"][-1].K
    qcfg = [(QParams(a.a_bits, a.w_bits, a.gsize, a.sym), QParams(b.a_bits, b.w_bits, b.gsize, b.sym))
            for a, b in zip(shapes["gate_up"], shapes["down"])]
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.05).half().to(dev)
    ffn = MoEFFN([mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)], [mk(H, N) for _ in range(E)] + [mk(H, Ns)], qcfg,
                 num_routed=E)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(torch.bfloat16).to(dev)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(torch.bfloat16).to(dev)
    blk_b = MoEBlock(ffn, w_gate, topk, w_shared_gate=w_sg)
    blk_h = MoEBlock(ffn, w_gate.half(), topk, w_shared_gate=w_sg.half())

    def one(bs: int) -> dict:
        hidden = torch.randn(bs, H, generator=g).to(torch.bfloat16).to(dev)
        gf_b, gf_h = GraphForward(blk_b, bs), GraphForward(blk_h, bs)
        h16 = torch.empty(bs, H, dtype=torch.float16, device=dev)
        out_b = torch.empty(bs, H, dtype=torch.bfloat16, device=dev)

        def native():
            gf_b.launch(hidden)

        def wrap():
            h16.copy_(hidden)
            gf_h.launch(h16)
            out_b.copy_(gf_h.out)

        g_native, g_wrap = _captured(native), _captured(wrap)
        torch.cuda.synchronize()

        wall, device = (lambda fn: _wall(fn, iters)), (lambda fn: _device(fn, iters))
        sides = {"native_eager_device": lambda: device(native), "wrap_eager_device": lambda: device(wrap),
                 "native_graph_device": lambda: device(g_native.replay), "wrap_graph_device": lambda: device(g_wrap.replay),
                 "native_eager_wall": lambda: wall(native), "wrap_eager_wall": lambda: wall(wrap),
                 "native_graph_wall": lambda: wall(g_native.replay), "wrap_graph_wall": lambda: wall(g_wrap.replay)}
        out = {"model": "qwen2_moe layer 11, bf16 ends", "bs": bs, "E": E, "topk": topk, "H": H}
        out.update({k: _stat(v) for k, v in _rounds(sides, rounds).items()})
        m = lambda k: out[k]["median_us"]
        for form in ("eager_device", "graph_device", "eager_wall", "graph_wall"):
            out[f"native_over_wrap_{form}"] = round(m(f"native_{form}") / m(f"wrap_{form}"), 4)
            out[f"saved_us_{form}"] = round(m(f"wrap_{form}") - m(f"native_{form}"), 1)
        out["cast_bytes"] = 2 * bs * H * 4  # each cast pass reads and writes bs * H 16-bit elements
        out["same_routing"] = bool(torch.equal(gf_b.gate_out[0], gf_h.gate_out[0]))
        out["status"] = gf_b.status() | gf_h.status()
        return out

    for bs in batches:  # (a generator: a caller can print each size as it completes)
        yield one(bs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--model", default="qwen2_moe", choices=["qwen2_moe", "ds2"])
    ap.add_argument("--dtype", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--bs", type=int, nargs="+", default=[128, 8192], help="batch sizes of the bf16 comparison")
    args = ap.parse_args()
    if args.dtype == "bf16":
        for r in bf16_layer_bench(args.bs, args.rounds, args.iters):
            print(json.dumps(r), flush=True)
            if r["status"]:
                sys.exit(1)
        return
    r = moe_bench.qwen2_layer_bench(args.rounds, args.iters, model=args.model)
    r["model"] = args.model
    print(json.dumps(r), flush=True)
    if not r["bit_identical"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
