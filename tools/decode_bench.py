"""The decode forward against the graph forward: qwen2_moe layer 11 (LP-1 mixed w4a4 + w8a8) at T = 1 / 4 / 16, run as
  (a) GraphForward replayed from a captured graph (route, segments, device planner, two GroupGEMMs, ...);
  (b) DecodeForward replayed from a captured graph (decode_gate_up, decode_down, combine; no planner),
in one process with the sides alternating over rounds (moe_bench.decode_forward_bench): device and wall time of both,
the two decode kernels alone, the plain-layout variant and the combine. One JSON line per T; --out also writes the
list to a file (profiles/<round>/decode/bench.json). Exits 1 when an output is not bit-identical to the eager layer.

--model gpt-oss: a synthetic gpt-oss layer instead (moe_bench.decode_forward_gptoss_bench: gptoss_layer of E = 32,
topk = 4, H = N = 2880, random codes, scale bytes in [118, 126]), DecodeForwardEx against GraphForward of the same layer,
with the two _ex kernels and the bias combine alone, the weight bytes read and the TB/s they imply. Exits 1 when an
output is not within the fp16 tolerance of the eager layer (MXFP4 sums depend on their order).

--model qwen2_moe --scheme w4a16_w8a8: layer 11 with the reference's small-batch scheme instead of LP-1
(workload.w4a16_w8a8_qconfig: w4a16_g-1_asym + w8a8 per linear, the shared expert included;
moe_bench.decode_forward_wo_bench), DecodeForwardWo against GraphForward of the same layer, with the two _wo kernels and
the combine alone, the weight bytes read and the TB/s they imply. Exits 1 when an output is not within the fp16
tolerance of the eager layer (weight-only sums depend on their order).

--model qwen2_moe --scheme e4m3: layer 11 with every expert w8a8_g-1_sym_E4M3 (moe_bench.decode_forward_e4m3_bench),
and --model gpt-oss --act-bits 8: the gpt-oss layer with MXFP8 activations (w4a8_g32_sym_MXFP8): DecodeForwardLp (the
MFMA decode kernels) against GraphForward of the same layer, compared within the fp16 tolerance.

--model qwen2_moe --scheme f8g128: layer 11 with every expert w8a8_g128_sym_E4M3 (moe_bench.decode_forward_f8g_bench):
DecodeForwardF8g against GraphForward of the same layer, on the rows --scheme e4m3 draws; --scheme f8g128_ds: a
DeepSeek-V3-shaped layer of that type (H = 7168, N = 2048, top-8, E reduced to 16). Compared within the fp16 tolerance.

--form a16: DecodeForwardA16 (fp16 activations on the fp16 MFMA) as a further side of the same rounds, beside the VALU
form and GraphForward, on the layers it takes: --scheme w4a16_w8a8, --scheme fp16 (layer 11 with every expert fp16) and
--model gpt-oss with fp16 activations. Reported with its two entries alone, its device median over the VALU form's and
over GraphForward's, and GraphForward's own (max - min) / median over the rounds.

--form f8g_wide: DecodeForwardF8gWide (block-scaled FP8 at up to 64 tokens) beside GraphForward and, up to 16 tokens,
DecodeForwardF8g, on --scheme f8g128 and f8g128_ds: device time per side and the wide form's ratios to the other two.

python tools/decode_bench.py [--model qwen2_moe|gpt-oss] [--scheme lp1|w4a16_w8a8|fp16|e4m3|f8g128|f8g128_ds] [--act-bits 16|8]
                             [--form valu|a16|f8g_wide] [--rounds 4] [--iters 30] [--batches 1,4,16] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from mxmoe_amd import moe_bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--batches", default="1,4,16")
    ap.add_argument("--out", default="")
    ap.add_argument("--model", default="qwen2_moe", choices=["qwen2_moe", "gpt-oss"])
    ap.add_argument("--scheme", default="lp1", choices=["lp1", "w4a16_w8a8", "fp16", "e4m3", "f8g128", "f8g128_ds"],
                    help="qwen2_moe: the layer's qconfig")
    ap.add_argument("--act-bits", type=int, default=16, choices=[16, 8], help="gpt-oss: fp16 or MXFP8 activations")
    ap.add_argument("--form", default="valu", choices=["valu", "a16", "f8g_wide"],
                    help="a16: DecodeForwardA16 as a further side; f8g_wide: DecodeForwardF8gWide")
    args = ap.parse_args()
    if args.model == "gpt-oss" and args.scheme != "lp1":
        ap.error("--scheme belongs to --model qwen2_moe")
    if args.model != "gpt-oss" and args.act_bits != 16:
        ap.error("--act-bits belongs to --model gpt-oss")
    a16 = args.form == "a16"
    if a16 and not (args.scheme in ("w4a16_w8a8", "fp16") or (args.model == "gpt-oss" and args.act_bits == 16)):
        ap.error("--form a16 takes --scheme w4a16_w8a8 or fp16, or --model gpt-oss with fp16 activations")
    wide = args.form == "f8g_wide"
    if wide and args.scheme not in ("f8g128", "f8g128_ds"):
        ap.error("--form f8g_wide takes --scheme f8g128 or f8g128_ds")
    results = []
    wo = args.scheme != "lp1"
    kw = {"act_bits": args.act_bits} if args.model == "gpt-oss" else {}
    if a16 or args.scheme == "fp16":
        kw["a16"] = a16
    bench = moe_bench.decode_forward_gptoss_bench if args.model == "gpt-oss" else \
        {"lp1": moe_bench.decode_forward_bench, "w4a16_w8a8": moe_bench.decode_forward_wo_bench,
         "fp16": lambda *a, **k: moe_bench.decode_forward_wo_bench(*a, fp16=True, **k),
         "e4m3": moe_bench.decode_forward_e4m3_bench, "f8g128": lambda *a: moe_bench.decode_forward_f8g_bench(*a, wide=wide),
         "f8g128_ds": lambda *a: moe_bench.decode_forward_f8g_bench(*a, deepseek=True, wide=wide)}[args.scheme]
    for r in bench([int(b) for b in args.batches.split(",") if b], args.rounds, args.iters, **kw):
        print(json.dumps(r), flush=True)
        results.append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)
    same = "close_to_eager" if args.model == "gpt-oss" or wo else "bit_identical_to_eager"
    if not all(all(r[same].values()) and not any(r["status"].values()) for r in results):
        sys.exit(1)


if __name__ == "__main__":
    main()
