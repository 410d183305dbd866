"""Benchmarks of the MoE layer and its plumbing (mxmoe_amd/moe.py), and the torch composite the router is timed
against: what tools/moe_layer_bench.py, graph_bench.py, gptoss_bench.py, fp8_layer_bench.py and gate_bench.py print, and bench.py's MoE
layer extras (through ``moe.qwen2_layer_bench``). Nothing here is on a layer's path."""
from __future__ import annotations

import ctypes
import time
from typing import Optional, Sequence

import torch

from . import _native as nat
from .groupgemm import W4A8_MXFP8, W4A16_MXFP4, QParams
from .harness import time_launches
from .moe import (_BITS, DecodeForward, DecodeForwardEx, DecodeForwardWo, GraphForward, MoEBlock, MoEFFN, PlannedForward, SwigluClamp, _launch_combine,
                  _ptr, _stream, combine_into, gate, gptoss_layer, prepare_weight_mx, silu_mul_quant)
from .workload import (ds2_mixed_qconfig, ds2_workload, load_workload, mixed_qconfig_lp1, qwen2_layer11_workload,
                       w4a16_w8a8_qconfig)


def _wall(fn, iters: int) -> float:
    """Median wall time of a call with a synchronise (µs), after 3 warm-up calls."""
    ts = []
    for i in range(iters + 3):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= 3:
            ts.append((time.perf_counter() - t0) * 1e6)
    return sorted(ts)[len(ts) // 2]


def _device(fn, iters: int) -> float:
    """Median device time of a launch sequence (µs)."""
    return time_launches(fn, 3, iters)["median_ms"] * 1e3


def _stat(values, digits: int = 1) -> dict:
    """A side's rounds: the median of the rounds' medians with min / max (µs) and (max - min) / median."""
    med = sorted(values)[len(values) // 2]
    return {"median_us": round(med, digits), "min_us": round(min(values), digits), "max_us": round(max(values), digits),
            "spread": round((max(values) - min(values)) / med, 4)}


def _captured(fn) -> torch.cuda.CUDAGraph:
    """``fn`` (launches only, e.g. a GraphForward's) run once on a side stream, then captured there: its graph."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    side.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    return graph


def _rounds(sides: dict, rounds: int) -> dict:
    """Every side measured once per round, the sides alternating: {side: its rounds' values}."""
    res = {k: [] for k in sides}
    for _ in range(rounds):
        for k, fn in sides.items():
            res[k].append(fn())
    return res


def qwen2_layer_bench(rounds: int = 4, iters: int = 30, bs: int = 8192, model: str = "qwen2_moe",
                      interleaved: bool = False, scheme: str = "lp1") -> dict:
    """qwen2_moe layer 11 (LP-1 mixed w4a4 + w8a8 qconfig, the committed routing histogram) — or
    model="ds2": the DeepSeek-V2-Lite mixed layer of the bench (64 routed experts, top-6, the two
    shared experts as one of twice the width) — with random weights, as planned MoE FFN steps,
    unfused vs the fused SiLU epilogue: per-stage and step device times (median over alternating
    rounds, µs) and whether the two outputs are bit-identical. interleaved: a third step, the fused
    layout through the plain epilogue + the interleaved-input SiLU pass (the small-batch form before
    round 6), with each step's gate_up mode. scheme (qwen2_moe): "lp1" (the LP-1 mixed w4a4 + w8a8
    qconfig) or "w4a16_w8a8" (the reference's small-batch scheme, hz_fused.cuh:14-125)."""
    if model == "ds2":
        layer = load_workload(ds2_workload(bs, qconfig=ds2_mixed_qconfig()))["layer-1"]
    else:
        qc = w4a16_w8a8_qconfig() if scheme == "w4a16_w8a8" else mixed_qconfig_lp1()
        layer = load_workload(qwen2_layer11_workload(bs, qconfig=qc))["layer-11"]
    E = len(layer["gate_up"]) - 1
    H = layer["gate_up"][0].K
    N, Ns = layer["down"][0].K, layer["down"][-1].K
    topk = max(1, round(sum(s.M for s in layer["gate_up"][:E]) / bs))
    qcfg = [(QParams(a.a_bits, a.w_bits, a.gsize, a.sym), QParams(b.a_bits, b.w_bits, b.gsize, b.sym))
            for a, b in zip(layer["gate_up"], layer["down"])]
    counts = [s.M for s in layer["gate_up"][:E]]
    counts[0] += bs * topk - sum(counts)  # the histogram's int() truncation
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    ids = torch.repeat_interleave(torch.arange(E, dtype=torch.int32), torch.tensor(counts))
    ids = ids[torch.randperm(ids.numel(), generator=g)].view(bs, topk).contiguous().to(dev)
    gate_up = [((torch.rand(2 * N, H, generator=g) * 2 - 1) * 0.05).half().to(dev) for _ in range(E)]
    gate_up.append(((torch.rand(2 * Ns, H, generator=g) * 2 - 1) * 0.05).half().to(dev))
    down = [((torch.rand(H, N, generator=g) * 2 - 1) * 0.05).half().to(dev) for _ in range(E)]
    down.append(((torch.rand(H, Ns, generator=g) * 2 - 1) * 0.05).half().to(dev))
    hidden = ((torch.rand(bs, H, generator=g) * 2 - 1)).half().to(dev)
    wts = torch.softmax(torch.rand(bs, topk, generator=g), dim=1).to(dev)
    modes = [("unfused", False, None), ("fused", True, None)] + ([("interleaved", True, "interleaved")] if interleaved else [])
    steps = {}
    for name, fuse, override in modes:
        layer_ = MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=fuse)
        layer_.gate_up_mode = override
        steps[name] = PlannedForward(layer_, hidden, ids, wts)
    del gate_up, down, layer_
    for st in steps.values():
        st()
    torch.cuda.synchronize()
    same = all(torch.equal(steps["unfused"].out.view(torch.int16), st.out.view(torch.int16)) for st in steps.values())
    res = {n: {"step": []} | {k: [] for k in st.stages} for n, st in steps.items()}
    for _ in range(rounds):
        for n, st in steps.items():
            res[n]["step"].append(time_launches(st, 5, iters)["median_ms"])
            for k, fn in st.stages.items():
                res[n][k].append(time_launches(fn, 3, iters)["median_ms"])
    out = {n: {k: round(sorted(v)[len(v) // 2] * 1e3, 1) for k, v in d.items()} for n, d in res.items()}
    out["bit_identical"] = bool(same)
    out["speedup"] = round(out["unfused"]["step"] / out["fused"]["step"], 4)
    out["gate_up_mode"] = {n: st.mode for n, st in steps.items()}
    names = [ln.split()[1] for ln in nat.list_variants()]
    out["gate_up_variant"] = {n: names[st.g1.variant] for n, st in steps.items()}
    return out


def graph_forward_bench(batches: Sequence[int] = (128,), model: str = "qwen2_moe", rounds: int = 4,
                        iters: int = 20):
    """One MoE FFN layer (qwen2_moe layer 11 with the LP-1 mixed w4a4 + w8a8 qconfig, or model="ds2": the
    DeepSeek-V2-Lite mixed layer) at every batch size of ``batches`` (yields one dict each), random weights,
    routing drawn from the committed histogram (top-4 / top-6 distinct experts per token), three ways in one process, the sides alternating over rounds:
      eager    MoEFFN.forward, wall time per call with a synchronise per call (host round trip, two host plans);
      planned  PlannedForward, device time (host-planned for this very routing: XCD-packed, split-K allowed);
      graph    GraphForward replayed from a captured graph, wall time (with a synchronise) and device time.
    Per side the median of the rounds' medians with min / max (µs); the two GroupGEMMs alone on both plans, the
    planner + GEMM pair against the GEMM at the capacity grid (their difference is the planner kernel), the
    segment kernel, and the tile slots launched against the tiles the routing uses."""
    if model == "ds2":
        shapes, topk = load_workload(ds2_workload(8192, qconfig=ds2_mixed_qconfig()))["layer-1"], 6
    else:
        shapes, topk = load_workload(qwen2_layer11_workload(8192, qconfig=mixed_qconfig_lp1()))["layer-11"], 4
    E = len(shapes["gate_up"]) - 1
    H = shapes["gate_up"][0].K
    N, Ns = shapes["down"][0].K, shapes["down"][-1].K
    qcfg = [(QParams(a.a_bits, a.w_bits, a.gsize, a.sym), QParams(b.a_bits, b.w_bits, b.gsize, b.sym))
            for a, b in zip(shapes["gate_up"], shapes["down"])]
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    hist = torch.tensor([max(s.M, 1) for s in shapes["gate_up"][:E]], dtype=torch.float64)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.05).half().to(dev)
    layer = MoEFFN([mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)], [mk(H, N) for _ in range(E)] + [mk(H, Ns)], qcfg,
                   num_routed=E)

    def one(bs: int) -> dict:
        ids = torch.multinomial((hist / hist.sum()).expand(bs, E), topk, replacement=False, generator=g).to(torch.int32).to(dev)
        hidden = ((torch.rand(bs, H, generator=g) * 2 - 1)).half().to(dev)
        wts = torch.softmax(torch.rand(bs, topk, generator=g), dim=1).to(dev)

        want = layer.forward(hidden, ids, wts)
        pf = PlannedForward(layer, hidden, ids, wts)
        gf = GraphForward(layer, bs, topk)
        graph = _captured(lambda: gf.launch(hidden, ids, wts))
        graph.replay()
        pf()
        torch.cuda.synchronize()
        same = bool(torch.equal(gf.out.view(torch.int16), want.view(torch.int16)))
        same_planned = bool(torch.equal(gf.out.view(torch.int16), pf.out.view(torch.int16)))
        wall, device = (lambda fn: _wall(fn, iters)), (lambda fn: _device(fn, iters))
        lib = nat.lib()
        st = _stream(None)
        sides = {
            "eager_wall": lambda: wall(lambda: layer.forward(hidden, ids, wts)),
            "planned_device": lambda: device(pf),
            "graph_wall": lambda: wall(graph.replay),
            "graph_device": lambda: device(graph.replay),
            "planned_gate_up": lambda: device(pf.g1.launch),
            "planned_down": lambda: device(pf.g2.launch),
            "dynamic_gate_up": lambda: device(lambda: gf.g1.launch(gf.dyn[0])),
            "dynamic_down": lambda: device(lambda: gf.g2.launch(gf.dyn[1])),
            "capacity_gemm_gate_up": lambda: device(lambda: nat.check(lib.mxmoe_gg_launch(ctypes.byref(gf.g1.info), st))),
            "capacity_gemm_down": lambda: device(lambda: nat.check(lib.mxmoe_gg_launch(ctypes.byref(gf.g2.info), st))),
            "segments": lambda: device(lambda: nat.check(lib.mxmoe_moe_segments(
                _ptr(gf.route_bufs[3]), E, bs, topk, 1, gf._tables, 2, _ptr(gf.seg_status), st))),
        }
        out = {"model": model, "bs": bs, "E": E, "topk": topk, "gate_up_mode": {"planned": pf.mode, "graph": gf.mode}}
        out.update({k: _stat(v) for k, v in _rounds(sides, rounds).items()})
        names = [ln.split()[1] for ln in nat.list_variants()]
        counts = gf.route_bufs[3].cpu().tolist() + [bs]
        out["plans"] = {}
        for name, dyn, host in (("gate_up", gf.g1, pf.g1), ("down", gf.g2, pf.g2)):
            tiles = nat.dynamic_tiles(list(dyn._c_problems), dyn.variant, dyn.joint, dyn.rows_total,
                                      [(c, 0, 0, 0) for c in counts])[0]
            out["plans"][name] = {"graph_variant": names[dyn.variant], "planned_variant": names[host.variant],
                                  "tile_slots": dyn.tile_slots, "tiles_used": int((tiles[:, 0] >= 0).sum()),
                                  "planned_tiles": host.total_tiles, "planned_splitk_slabs": int(host.info.splitk_slabs)}
        m = lambda k: out[k]["median_us"]
        out["planner_kernel_us"] = {"gate_up": round(m("dynamic_gate_up") - m("capacity_gemm_gate_up"), 1),
                                    "down": round(m("dynamic_down") - m("capacity_gemm_down"), 1)}
        out["graph_wall_over_eager_wall"] = round(m("graph_wall") / m("eager_wall"), 4)
        out["graph_device_over_planned_device"] = round(m("graph_device") / m("planned_device"), 4)
        out["bit_identical_to_eager"], out["bit_identical_to_planned"] = same, same_planned
        out["status"] = gf.status()
        return out

    for bs in batches:  # (a generator: a caller can print each size as it completes)
        yield one(bs)


def fp8_layer_bench(batches: Sequence[int] = (128, 512, 2048, 8192), rounds: int = 4, iters: int = 30):
    """FP8 layers: the qwen2_moe layer-11 shape (60 routed experts, top-4, the shared expert; routing drawn from the
    committed histogram, random weights) at every batch size of ``batches`` (yields one dict each) with every expert
    w8a8_g-1_sym_E4M3 ("e4m3"), w8a8_g-1_sym ("w8a8") or fp16, each side a ``PlannedForward`` step on the same
    weights, hidden states and routing, in one process with the sides alternating over rounds. All three run the
    plain gate_up layout (fuse_silu=False: the E4M3 tile has no SiLU epilogue), so the two activation passes of the
    e4m3 and w8a8 sides are the same launches on the same bytes but for the tag. Per side and stage the median of the
    rounds' medians with min / max (us), the gate_up / down variants, and per activation pass whether the e4m3 median
    lies inside the w8a8 side's own min - max over the rounds ("parity") with the ratio of the medians."""
    from .groupgemm import FP16, W8A8, W8A8_E4M3

    shapes, topk = load_workload(qwen2_layer11_workload(8192))["layer-11"], 4
    E = len(shapes["gate_up"]) - 1
    H = shapes["gate_up"][0].K
    N, Ns = shapes["down"][0].K, shapes["down"][-1].K
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    hist = torch.tensor([max(s.M, 1) for s in shapes["gate_up"][:E]], dtype=torch.float64)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.05).half().to(dev)
    gate_up = [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)]
    down = [mk(H, N) for _ in range(E)] + [mk(H, Ns)]
    layers = {name: MoEFFN(gate_up, down, [(q, q)] * (E + 1), num_routed=E, fuse_silu=False)
              for name, q in (("e4m3", W8A8_E4M3), ("w8a8", W8A8), ("fp16", FP16))}
    names = [ln.split()[1] for ln in nat.list_variants()]

    def one(bs: int) -> dict:
        ids = torch.multinomial((hist / hist.sum()).expand(bs, E), topk, replacement=False, generator=g).to(torch.int32).to(dev)
        hidden = ((torch.rand(bs, H, generator=g) * 2 - 1)).half().to(dev)
        wts = torch.softmax(torch.rand(bs, topk, generator=g), dim=1).to(dev)
        steps = {n: PlannedForward(layer, hidden, ids, wts) for n, layer in layers.items()}
        for st in steps.values():
            st()
        torch.cuda.synchronize()
        ref = steps["fp16"].out.float()
        sides = {}
        for n, st in steps.items():
            sides[(n, "step")] = lambda st=st: time_launches(st, 5, iters)["median_ms"] * 1e3
            for k, fn in st.stages.items():
                sides[(n, k)] = lambda fn=fn: _device(fn, iters)
        res = _rounds(sides, rounds)
        out = {"bs": bs, "E": E, "topk": topk, "H": H, "N": N, "N_shared": Ns}
        for n, st in steps.items():
            out[n] = {k: _stat(res[(n, k)]) for k in ["step", *st.stages]}
            out[n]["gate_up_mode"] = st.mode
            out[n]["variants"] = {"gate_up": names[st.g1.variant], "down": names[st.g2.variant]}
            out[n]["splitk_slabs"] = [int(st.g1.info.splitk_slabs), int(st.g2.info.splitk_slabs)]
            err = (st.out.float() - ref).norm() / ref.norm()
            out[n]["rel_err_to_fp16"] = round(float(err), 5)
        out["act_passes_vs_w8a8"] = {}
        for k in ("quant_act", "act_quant"):
            e, w = out["e4m3"][k], out["w8a8"][k]
            out["act_passes_vs_w8a8"][k] = {"parity": bool(w["min_us"] <= e["median_us"] <= w["max_us"]),
                                            "ratio": round(e["median_us"] / w["median_us"], 4)}
        for k in ("gate_up", "down", "step"):
            out["act_passes_vs_w8a8"][k] = {"ratio": round(out["e4m3"][k]["median_us"] / out["w8a8"][k]["median_us"], 4)}
        return out

    for bs in batches:  # (a generator: a caller can print each size as it completes)
        yield one(bs)


def _decode_bench(layer: MoEFFN, cls, call, rounds: int, iters: int, head: dict, compare: str, weight_bytes,
                  plain: Optional[MoEFFN] = None, report_used: bool = True) -> dict:
    """One batch size of a decode bench: ``cls(layer)`` against ``GraphForward(layer)`` on ``call`` = (hidden, ids,
    wts), both captured and replayed, the sides alternating over rounds. Compared with the eager layer bit for bit
    (``compare`` = "bit_identical_to_eager") or within the fp16 GroupGEMM tolerance 1e-3 |ref| + 1e-3 rms(ref)
    ("close_to_eager": sums that depend on their order). Timed: device and wall time of each graph, the class's two
    entries alone and its combine; ``plain``: the same layer in the plain gate_up layout as a third side (LP-1).
    Reported: ``weight_bytes(weights, experts)`` of the experts the ids name (and the shared one), with ``report_used``
    also their number and the TB/s the two entries imply; ``faster`` — the decode graph's device median, max over
    rounds, below GraphForward's min over rounds — and the status words."""
    hidden, ids, wts = call
    bs, topk = ids.shape
    E, shared = layer.E, int(layer.has_shared)
    want = layer.forward(hidden, ids, wts)
    objs = {"graph": GraphForward(layer, bs, topk), "decode": cls(layer, bs, topk)}
    if plain is not None:
        objs["decode_plain"] = cls(plain, bs, topk)
    gf, df = objs["graph"], objs["decode"]
    graphs = {k: _captured(lambda o=o: o.launch(hidden, ids, wts)) for k, o in objs.items()}
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    if compare == "bit_identical_to_eager":
        same = {k: bool(torch.equal(o.out.view(torch.int16), want.view(torch.int16))) for k, o in objs.items()}
    else:
        want = want.float()
        tol = 1e-3 * want.abs() + 1e-3 * want.square().mean().sqrt() + 1e-6
        same = {k: bool(((o.out.float() - want).abs() <= tol).all()) for k, o in objs.items()}
    wall, device = (lambda fn: _wall(fn, iters)), (lambda fn: _device(fn, iters))
    st, glu = _stream(None), ((df._glu,) if df.TAKES_GLU else ())
    gate_up_k = lambda: nat.check(nat.symbol(df.ENTRIES[0])(
        *glu, nat.DT_FP16, _ptr(hidden), bs, topk, E, shared, _ptr(ids), _ptr(df.experts), df.mask1, layer.H, layer.N,
        layer.Ns, df.layout, _ptr(df.act), _ptr(df.act_shared), _ptr(df.dev_status), st))
    down_k = lambda: nat.check(nat.symbol(df.ENTRIES[1])(
        bs, topk, E, shared, _ptr(ids), _ptr(df.experts), df.mask2, layer.H, layer.N, layer.Ns, _ptr(df.act),
        _ptr(df.act_shared), _ptr(df.y), _ptr(df.ys), _ptr(df.dev_status), st))
    if df._glu is not None:  # the bias combine, as DecodeForwardEx.launch calls it
        combine = {"combine_bias": lambda: device(lambda: _launch_combine(df.out, df.y, df.inv_slot, ids.view(-1), wts, None, None,
                                                                          topk, None, layer.down_bias))}
    else:
        combine = {"combine": lambda: device(lambda: combine_into(df.out, df.y, df.inv_slot, wts, df.ys, topk))}
    sides = {k + "_device": (lambda gr=gr: device(gr.replay)) for k, gr in graphs.items()}
    sides.update({"graph_wall": lambda: wall(graphs["graph"].replay), "decode_wall": lambda: wall(graphs["decode"].replay),
                  "decode_gate_up": lambda: device(gate_up_k), "decode_down": lambda: device(down_k)}, **combine)
    out = dict(head, graph_gate_up_mode=gf.mode)
    out.update({k: _stat(v) for k, v in _rounds(sides, rounds).items()})
    used = sorted(set(ids.flatten().tolist())) + ([E] if shared else [])
    mb = {"gate_up": weight_bytes(layer.w1, used) / 1e6, "down": weight_bytes(layer.w2, used) / 1e6}
    if report_used:
        out["experts_used"] = len(used) - shared
    out["weight_mb"] = {k: round(v, 2) for k, v in mb.items()}
    if report_used:
        out["implied_tb_s"] = {k: round(mb[k] / out["decode_" + k]["median_us"], 3) for k in mb}  # MB / µs = TB/s
    out["decode_over_graph_device"] = round(out["decode_device"]["median_us"] / out["graph_device"]["median_us"], 4)
    out["faster"] = bool(out["decode_device"]["max_us"] < out["graph_device"]["min_us"])
    out[compare] = same
    out["status"] = {"graph": gf.status(), "decode": df.status() | (objs["decode_plain"].status() if plain is not None else 0)}
    return out


def _qwen2_decode_layer(qconfig, g, dev: str):
    """qwen2_moe layer 11 under ``qconfig`` with random weights: (gate_up, down, qcfg, routing histogram, E, H, N, Ns)"""
    shapes = load_workload(qwen2_layer11_workload(8192, qconfig=qconfig))["layer-11"]
    E = len(shapes["gate_up"]) - 1
    H = shapes["gate_up"][0].K
    N, Ns = shapes["down"][0].K, shapes["down"][-1].K
    qcfg = [(QParams(a.a_bits, a.w_bits, a.gsize, a.sym), QParams(b.a_bits, b.w_bits, b.gsize, b.sym))
            for a, b in zip(shapes["gate_up"], shapes["down"])]
    hist = torch.tensor([max(s.M, 1) for s in shapes["gate_up"][:E]], dtype=torch.float64)
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.05).half().to(dev)
    gate_up, down = [mk(2 * N, H) for _ in range(E)] + [mk(2 * Ns, H)], [mk(H, N) for _ in range(E)] + [mk(H, Ns)]
    return gate_up, down, qcfg, hist, E, H, N, Ns


def _qwen2_decode_call(g, hist, bs: int, E: int, topk: int, H: int, dev: str):
    ids = torch.multinomial((hist / hist.sum()).expand(bs, E), topk, replacement=False, generator=g).to(torch.int32).to(dev)
    hidden = ((torch.rand(bs, H, generator=g) * 2 - 1)).half().to(dev)
    wts = torch.softmax(torch.rand(bs, topk, generator=g), dim=1).to(dev)
    return hidden, ids, wts


def decode_forward_bench(batches: Sequence[int] = (1, 4, 16), rounds: int = 4, iters: int = 30):
    """qwen2_moe layer 11 (LP-1 mixed w4a4 + w8a8, random weights, routing drawn from the committed histogram) at
    decode sizes, ``DecodeForward`` against ``GraphForward``, both replayed from captured graphs in one process with
    the sides alternating over rounds (yields one dict per batch size): device and wall time of each graph, the two
    decode kernels alone, the plain-layout DecodeForward (the same kernels on [gate; up] rows), and the combine. Per
    side the median of the rounds' medians with min / max (µs). ``faster``: the bar — DecodeForward's device median,
    max over rounds, below GraphForward's min over rounds."""
    dev, topk, g = "cuda", 4, torch.Generator().manual_seed(0)
    gate_up, down, qcfg, hist, E, H, N, Ns = _qwen2_decode_layer(mixed_qconfig_lp1(), g, dev)
    layer = MoEFFN(gate_up, down, qcfg, num_routed=E)
    plain = MoEFFN(gate_up, down, qcfg, num_routed=E, fuse_silu=False)
    del gate_up, down
    weight_bytes = lambda ws, es: sum(ws[e].B.numel() * ws[e].B.element_size() for e in es)
    for bs in batches:  # (a generator: a caller can print each size as it completes)
        head = {"model": "qwen2_moe", "bs": bs, "E": E, "topk": topk, "H": H, "N": N, "N_shared": Ns}
        yield _decode_bench(layer, DecodeForward, _qwen2_decode_call(g, hist, bs, E, topk, H, dev), rounds, iters, head,
                            "bit_identical_to_eager", weight_bytes, plain=plain, report_used=False)


def decode_forward_wo_bench(batches: Sequence[int] = (1, 4, 16), rounds: int = 4, iters: int = 30):
    """qwen2_moe layer 11 with the reference's small-batch scheme (``w4a16_w8a8_qconfig``: w4a16_g-1_asym + w8a8 per
    linear, the shared expert included; random weights, routing drawn from the committed histogram) at decode sizes,
    ``DecodeForwardWo`` against ``GraphForward`` of the same layer, as ``decode_forward_bench`` measures the LP-1 layer
    (yields one dict per batch size). Also the weight bytes (codes and scale buffers of the experts the ids name, and
    the shared expert's), the TB/s they imply and the kinds among them. Weight-only sums depend on their order, so the
    outputs are compared with the eager layer's within the fp16 GroupGEMM tolerance, not bit for bit."""
    dev, topk, g = "cuda", 4, torch.Generator().manual_seed(0)
    gate_up, down, qcfg, hist, E, H, N, Ns = _qwen2_decode_layer(w4a16_w8a8_qconfig(), g, dev)
    layer = MoEFFN(gate_up, down, qcfg, num_routed=E)
    del gate_up, down
    weight_bytes = lambda ws, es: sum(ws[e].B.numel() * ws[e].B.element_size() +
                                      ws[e].scale_b.numel() * ws[e].scale_b.element_size() for e in es)
    for bs in batches:
        head = {"model": "qwen2_moe", "scheme": "w4a16_w8a8", "bs": bs, "E": E, "topk": topk, "H": H, "N": N, "N_shared": Ns}
        call = _qwen2_decode_call(g, hist, bs, E, topk, H, dev)
        out = _decode_bench(layer, DecodeForwardWo, call, rounds, iters, head, "close_to_eager", weight_bytes)
        used = sorted(set(call[1].flatten().tolist())) + [E]
        out["kinds"] = {"gate_up": sorted({layer.w1[e].q.qcfg for e in used}), "down": sorted({layer.w2[e].q.qcfg for e in used})}
        yield out


def decode_forward_gptoss_bench(batches: Sequence[int] = (1, 4, 16), rounds: int = 4, iters: int = 30, E: int = 32,
                                topk: int = 4, H: int = 2880, N: int = 2880):
    """A synthetic gpt-oss layer (``gptoss_layer``: E = 32, top-4, H = N = 2880 padded to 2944, random e2m1 codes, scale
    bytes in [118, 126], biases in +-0.5, the clamped SwiGLU) at decode sizes, ``DecodeForwardEx`` against
    ``GraphForward`` of the same layer, as ``decode_forward_bench`` measures the qwen2_moe layer (yields one dict per
    batch size), with the bias combine alone. Also the weight bytes (codes and scale bytes of the experts the ids
    name) and the TB/s they imply. MXFP4 sums depend on their order, so the outputs are compared with the eager
    layer's within the fp16 GroupGEMM tolerance, not bit for bit."""
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    u8 = lambda *shape, lo=0, hi=256: torch.randint(lo, hi, shape, generator=g, device=dev, dtype=torch.uint8)
    bias = lambda *shape: torch.rand(*shape, generator=g, device=dev) - 0.5
    layer = gptoss_layer(u8(E, 2 * N, H // 32, 16), u8(E, 2 * N, H // 32, lo=118, hi=127), bias(E, 2 * N),
                         u8(E, H, N // 32, 16), u8(E, H, N // 32, lo=118, hi=127), bias(E, H))
    weight_bytes = lambda ws, es: sum(ws[e].B.numel() + ws[e].scale_b.numel() for e in es)
    for bs in batches:
        ids = torch.stack([torch.randperm(E, generator=g, device=dev)[:topk] for _ in range(bs)]).to(torch.int32)
        hidden = torch.zeros(bs, layer.H, dtype=torch.float16, device=dev)
        hidden[:, :H] = (torch.randn(bs, H, generator=g, device=dev) * 0.5).half()
        wts = torch.softmax(torch.rand(bs, topk, generator=g, device=dev), dim=1)
        head = {"model": "gpt-oss layer (synthetic)", "bs": bs, "E": E, "topk": topk, "H": layer.H, "N": layer.N}
        yield _decode_bench(layer, DecodeForwardEx, (hidden, ids, wts), rounds, iters, head, "close_to_eager", weight_bytes)


def gptoss_bench(batches: Sequence[int] = (1, 16, 128, 512, 2048), act_bits: int = 16, rounds: int = 4, iters: int = 20,
                 E: int = 32, topk: int = 4, H: int = 2944, N: int = 2944):
    """One gpt-oss-20b-shaped MoE block (E = 32 experts, top-4, H = N = 2880 padded to 2944, MXFP4 weights with random
    codes, biases, the clamped SwiGLU, the router with its logit bias) at every batch size of ``batches`` (yields one
    dict each), three ways in one process with the sides alternating over rounds, as ``graph_forward_bench``: eager
    ``MoEBlock.forward`` (wall, a synchronise per call), ``PlannedForward`` (device), ``GraphForward`` replayed from a
    captured graph (wall and device); and the two new plumbing kernels against the ones they stand in for at the
    same shape: the biased clamped activation pass against the SiLU pass, combine_bias against combine, with the
    extra bias bytes each reads. Per side the median of the rounds' medians with min / max (µs). act_bits: 16 or 8."""
    dev = "cuda"
    q = {16: W4A16_MXFP4, 8: W4A8_MXFP8}[act_bits]
    g = torch.Generator(device=dev).manual_seed(0)

    def weight(rows, K):  # random e2m1 codes, scales 2^-6 .. 2^-4 (|w| <= 0.375)
        codes = torch.randint(0, 256, (rows, K // 2), generator=g, device=dev, dtype=torch.uint8)
        scales = torch.randint(121, 124, (rows, K // 32), generator=g, device=dev, dtype=torch.uint8)
        return prepare_weight_mx(codes, scales, q)

    rnd = lambda *shape: torch.rand(*shape, generator=g, device=dev) * 2 - 1
    ffn = MoEFFN([weight(2 * N, H) for _ in range(E)], [weight(H, N) for _ in range(E)], [(q, q)] * E, num_routed=E,
                 gate_up_bias=list(rnd(E, 2 * N) * 0.5), down_bias=list(rnd(E, H) * 0.5), activation=SwigluClamp())
    block = MoEBlock(ffn, (torch.randn(E, H, generator=g, device=dev) * H ** -0.5).half(), topk, renormalize=True,
                     logit_bias=torch.randn(E, generator=g, device=dev))

    def one(bs: int) -> dict:
        hidden = (torch.randn(bs, H, generator=g, device=dev) * 0.5).half()
        want, mid = block.forward(hidden, return_intermediates=True)
        ids, wts, r = mid["topk_ids"], mid["topk_weights"], mid["routing"]
        pf = PlannedForward(ffn, hidden, ids, wts)
        gf = GraphForward(block, bs)
        graph = _captured(lambda: gf.launch(hidden))
        graph.replay()
        pf()
        torch.cuda.synchronize()
        same = bool(torch.equal(gf.out.view(torch.int16), want.view(torch.int16)))
        same_planned = bool(torch.equal(pf.out.view(torch.int16), want.view(torch.int16)))
        # the plumbing kernels alone, old against new, on the planned step's buffers
        silu = silu_mul_quant(pf.h1, None, r, ffn.tag2)
        out2 = torch.empty_like(pf.out)
        w32 = wts.to(torch.float32).contiguous()
        wall, device = (lambda fn: _wall(fn, iters)), (lambda fn: _device(fn, iters))
        sides = {
            "eager_wall": lambda: wall(lambda: block.forward(hidden)),
            "planned_device": lambda: device(pf),
            "graph_wall": lambda: wall(graph.replay),
            "graph_device": lambda: device(graph.replay),
            "act_silu": lambda: device(silu.relaunch),
            "act_glu_bias": lambda: device(pf.a2.relaunch),
            "combine": lambda: device(lambda: combine_into(out2, pf.y, r.inv_slot, w32, None, topk)),
            "combine_bias": lambda: device(pf.stages["combine"]),
        }
        out = {"model": "gpt-oss-20b layer", "act_bits": act_bits, "bs": bs, "E": E, "topk": topk, "H": H, "N": N}
        out.update({k: _stat(v) for k, v in _rounds(sides, rounds).items()})
        m = lambda k: out[k]["median_us"]
        n = bs * topk
        abits = _BITS[ffn.tag2[0]]
        out["act_bytes"] = {"silu": n * 2 * N * 2 + n * N * abits // 8, "extra_bias_read": n * 2 * N * 2,
                            "distinct_bias": E * 2 * N * 2}
        out["combine_bytes"] = {"combine": n * H * 2 + bs * H * 2, "extra_bias_read": n * H * 2 + n * 4,
                                "distinct_bias": E * H * 2}
        out["act_glu_bias_over_silu"] = round(m("act_glu_bias") / m("act_silu"), 4)
        out["combine_bias_over_combine"] = round(m("combine_bias") / m("combine"), 4)
        out["graph_wall_over_eager_wall"] = round(m("graph_wall") / m("eager_wall"), 4)
        out["graph_device_over_planned_device"] = round(m("graph_device") / m("planned_device"), 4)
        names = [ln.split()[1] for ln in nat.list_variants()]
        out["variants"] = {"planned": [names[pf.g1.variant], names[pf.g2.variant]],
                           "graph": [names[gf.g1.variant], names[gf.g2.variant]]}
        # the host plans (eager, planned) may split K, the device-planned graph never does: with float accumulation
        # (fp16 or MXFP8 activations) the two then differ in summation order, so bit identity is expected only
        # where no host plan split K
        out["host_splitk_slabs"] = [int(pf.g1.info.splitk_slabs), int(pf.g2.info.splitk_slabs)]
        out["graph_max_abs_diff_to_eager"] = float((gf.out.float() - want.float()).abs().max())
        out["eager_max_abs"] = float(want.float().abs().max())
        out["bit_identical_to_eager"], out["planned_bit_identical_to_eager"] = same, same_planned
        out["status"] = gf.status()
        return out

    for bs in batches:  # (a generator: a caller can print each size as it completes)
        yield one(bs)


GATE_MODELS = {"qwen2_moe": dict(H=2048, E=60, topk=4, shared_gate=True),
               "ds2": dict(H=2048, E=64, topk=6, shared_gate=False),
               # DeepSeek-V3 / R1 (noaux_tc) and the full DeepSeek-V2 (group_limited_greedy)
               "ds3": dict(H=7168, E=256, topk=8, shared_gate=False, renormalize=True, bias=True,
                           routing=dict(scoring="sigmoid", n_group=8, topk_group=4, routed_scaling_factor=2.5)),
               "ds2_full": dict(H=5120, E=160, topk=6, shared_gate=False,
                                routing=dict(scoring="softmax", n_group=8, topk_group=3, group_top=1,
                                             routed_scaling_factor=16.0)),
               # more than 256 experts (mxmoe_moe_gate_wide): Kimi-K2 (sigmoid + bias, one group) and Qwen3-Next
               # (softmax over the chosen ones, shared-expert gate: 513 columns)
               "kimi_k2": dict(H=7168, E=384, topk=8, shared_gate=False, renormalize=True, bias=True,
                               routing=dict(scoring="sigmoid", routed_scaling_factor=2.827)),
               "qwen3_next": dict(H=2048, E=512, topk=10, shared_gate=True, renormalize=True,
                                  routing=dict(scoring="softmax"))}
HBM_ROOF_BYTES_PER_S = 8e12  # MI355X


def _group_mask(group_scores: torch.Tensor, topk_group: int, gs: int) -> torch.Tensor:
    """The published group stage (DeepSeek-V2 / V3 MoEGate.forward): bool [T, E], the kept groups' experts."""
    T, n_group = group_scores.shape
    group_idx = torch.topk(group_scores, k=topk_group, dim=-1, sorted=False)[1]
    group_mask = torch.zeros_like(group_scores)
    group_mask.scatter_(1, group_idx, 1)
    return group_mask.unsqueeze(-1).expand(T, n_group, gs).reshape(T, -1).bool()


def gate_composite(logits: torch.Tensor, topk: int, renormalize: bool = False, e_bias: Optional[torch.Tensor] = None,
                   scoring: str = "softmax", n_group: int = 1, topk_group: int = 1, group_top: Optional[int] = None,
                   routed_scaling_factor: float = 1.0):
    """The models' public routing code on f32 logits, in torch: softmax -> topk (qwen2_moe,
    DeepSeek-V2-Lite), DeepSeek-V2's group_limited_greedy, DeepSeek-V3's noaux_tc (masked_fill 0.0 as
    published). Returns (int32 ids, f32 weights)."""
    T, E = logits.shape
    if scoring == "softmax":
        scores = torch.softmax(logits, dim=-1)
        choice = scores
        if n_group > 1:
            group_scores = scores.view(T, n_group, -1).max(dim=-1).values
            choice = scores.masked_fill(~_group_mask(group_scores, topk_group, E // n_group), 0.0)
        wts, ids = torch.topk(choice, topk, dim=-1)
    else:
        scores = logits.sigmoid()
        choice = scores if e_bias is None else scores + e_bias.unsqueeze(0)
        if n_group > 1:
            group_scores = choice.view(T, n_group, -1).topk(2, dim=-1)[0].sum(dim=-1)
            choice = choice.masked_fill(~_group_mask(group_scores, topk_group, E // n_group), 0.0)
        ids = torch.topk(choice, topk, dim=-1)[1]
        wts = scores.gather(1, ids)
    if renormalize:
        wts = wts / (wts.sum(dim=-1, keepdim=True) + 1e-20)
    if routed_scaling_factor != 1.0:
        wts = wts * routed_scaling_factor
    return ids.to(torch.int32), wts


def gate_bench(bs: int = 8192, model: str = "qwen2_moe", rounds: int = 4, iters: int = 30, dtype: str = "fp16") -> dict:
    """The router kernel against the torch composite it replaces (fp16 matmul -> f32 softmax -> topk
    -> int32 ids, + sigmoid(hidden @ w_sg) for qwen2_moe; for ds3 / ds2_full the public group-limited
    routing code, ``gate_composite``), same process, interleaved round by round:
    per side the median of the rounds' medians with min / max (µs) and the composite's run-to-run
    spread (max - min) / median; the kernel's algorithmic bytes and fraction of the HBM roof.
    model: "qwen2_moe" (H 2048, E 60, top-4, shared gate), "ds2" (DeepSeek-V2-Lite: E 64, top-6),
    "ds3" (DeepSeek-V3: H 7168, E 256, top-8, 8 groups / 4 kept, sigmoid + bias, renormalised, factor
    2.5), "ds2_full" (DeepSeek-V2: H 5120, E 160, top-6, 8 groups / 3 kept, softmax, factor 16), "kimi_k2"
    (H 7168, E 384, top-8, sigmoid + bias, renormalised, factor 2.827) or "qwen3_next" (H 2048, E 512, top-10,
    softmax renormalised, shared gate). dtype: "fp16" or "bf16" — the operands of the kernel and of the composite's
    matmul (the same random values rounded to that format)."""
    if dtype not in ("fp16", "bf16"):
        raise ValueError(f"dtype must be 'fp16' or 'bf16', got {dtype!r}")
    dt = torch.bfloat16 if dtype == "bf16" else torch.float16
    m = GATE_MODELS[model]
    H, E, topk = m["H"], m["E"], m["topk"]
    routing = dict(m.get("routing", {}))
    renorm = bool(m.get("renormalize", False))
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    hidden = torch.randn(bs, H, generator=g).to(dt).to(dev)
    w_gate = (torch.randn(E, H, generator=g) * H ** -0.5).to(dt).to(dev)
    w_sg = (torch.randn(H, generator=g) * H ** -0.5).to(dt).to(dev) if m["shared_gate"] else None
    if m.get("bias"):
        routing["e_bias"] = (torch.randint(-64, 65, (E,), generator=g).float() / 256).to(dev)
    bufs = gate(hidden, w_gate, topk, renormalize=renorm, w_shared_gate=w_sg, **routing)

    def kernel():
        gate(hidden, w_gate, topk, renormalize=renorm, w_shared_gate=w_sg, out=bufs, **routing)

    def composite():
        logits = (hidden @ w_gate.T).float()
        if routing:
            ids, wts = gate_composite(logits, topk, renorm, **routing)
        else:
            wts, ids = torch.topk(torch.softmax(logits, dim=-1), topk, dim=-1)
            ids = ids.to(torch.int32)
        sw = torch.sigmoid(hidden @ w_sg) if w_sg is not None else None
        return ids, wts, sw

    ref_ids = composite()[0]
    torch.cuda.synchronize()
    agree = float((bufs[0] == ref_ids).all(dim=1).float().mean())  # fp16-rounded logits can reorder near-ties
    res = {"kernel": [], "torch": []}
    for _ in range(rounds):
        res["kernel"].append(time_launches(kernel, 5, iters)["median_ms"] * 1e3)
        res["torch"].append(time_launches(composite, 5, iters)["median_ms"] * 1e3)

    out = {"model": model, "bs": bs, "H": H, "E": E, "topk": topk, "dtype": dtype, "shared_gate": w_sg is not None,
           "kernel": _stat(res["kernel"], 2), "torch": _stat(res["torch"], 2)}
    nbytes = bs * H * 2 + (E + 1) * H * 2 + bs * topk * 8 + (bs * 4 if w_sg is not None else 0)
    if routing:
        nbytes += E * 4 if "e_bias" in routing else 0
        out["routing"] = {k: v for k, v in routing.items() if k != "e_bias"}
        out["routing"].update(renormalize=renorm, e_bias="e_bias" in routing)
    out["bytes"] = nbytes
    out["hbm_fraction"] = round(nbytes / (out["kernel"]["median_us"] * 1e-6) / HBM_ROOF_BYTES_PER_S, 4)
    out["speedup"] = round(out["torch"]["median_us"] / out["kernel"]["median_us"], 3)
    # the bar: the kernel's median no slower than the composite's, within the composite's own spread
    out["meets_bar"] = bool(out["kernel"]["median_us"] <= out["torch"]["median_us"] * (1 + out["torch"]["spread"]))
    out["rows_same_ids_as_torch"] = round(agree, 4)
    return out
