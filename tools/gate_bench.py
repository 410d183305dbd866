"""Print mxmoe_amd.moe_bench.gate_bench (the router kernel against the torch composite) as JSON lines:
    python tools/gate_bench.py [--bs 8192 128] [--models qwen2_moe ds2 ds3 ds2_full kimi_k2 qwen3_next]
                               [--dtype fp16 bf16] [--out FILE]"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxmoe_amd.moe_bench import gate_bench  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--bs", type=int, nargs="+", default=[8192, 128])
    ap.add_argument("--models", nargs="+", default=["qwen2_moe", "ds2"],
                    help="qwen2_moe ds2 ds3 ds2_full kimi_k2 qwen3_next (mxmoe_amd.moe_bench.GATE_MODELS)")
    ap.add_argument("--dtype", nargs="+", default=["fp16"], choices=["fp16", "bf16"],
                    help="the operands' element type; both: each shape with the two dtypes back to back")
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None, help="also write the list of results to this JSON file")
    a = ap.parse_args()
    results = []
    for model in a.models:
        for bs in a.bs:
            for dtype in a.dtype:
                r = gate_bench(bs=bs, model=model, rounds=a.rounds, iters=a.iters, dtype=dtype)
                results.append(r)
                print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
