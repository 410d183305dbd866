"""CPU tests of the host tile planner (gg_plan.cpp:plan_host) through mxmoe_gg_plan_tiles: every
output tile of every problem is planned exactly once (split-K slices partition its K stages), and
the placement rules hold — the shared expert of a bs=8192 layer is cut into one rectangle per XCD at
the end (or, switched, the head) of that XCD's queue, and routed experts are not split across XCDs by chunk boundaries.
(The reference's TileScheduler, tile_scheduler.cuh:5-50, walks problems in order on the device; the
placement is ours and affects speed and HBM traffic only, never results.)
The planner is a host-only unit: tests/cpp/plan_host_check.cpp runs it without the library, under the host
compiler's sanitizers (test_host_planner_under_host_sanitizers).
"""
from __future__ import annotations

import collections
import ctypes
import os

import numpy as np
import pytest

from mxmoe_amd import _native as nat
from mxmoe_amd.workload import load_workload, mixed_qconfig_lp1, model_workload, qwen2_layer11_workload

FMT = {"": nat.FMT_DEFAULT, "E4M3": nat.FMT_E4M3, "bf16": nat.FMT_BF16}


def _probs(shapes):
    return [nat.GGProblemC(A=0, B=0, scale_a=0, scale_b=0, C=0, M=s.M, N=s.N, K=s.K, a_bits=s.a_bits,
                           w_bits=s.w_bits, gsize=s.gsize, sym=int(s.sym), fmt=FMT[s.fmt], lda=0, ldb=0, ldc=0)
            for s in shapes]


def _bn(variant, s):
    bm, bn, bk, th = (ctypes.c_int32() for _ in range(4))
    nat.check(nat.lib().mxmoe_gg_variant_tile(variant, s.a_bits, s.w_bits, *(ctypes.byref(x) for x in (bm, bn, bk, th))))
    return bm.value, bn.value


def _layer(bs=8192, **kw):
    return load_workload(qwen2_layer11_workload(bs, **kw))["layer-11"]


def check_coverage(shapes, variant=nat.VARIANT_AUTO):
    probs = _probs(shapes)
    v = nat.resolve_variant((nat.GGProblemC * len(probs))(*probs), len(probs), variant)
    tiles, rows = nat.plan_tiles(probs, v)
    live = tiles[tiles[:, 0] >= 0]
    assert len({tuple(t) for t in live.tolist()}) == len(live), "a tile slot is planned twice"
    by_prob = collections.defaultdict(list)
    for t in live:
        by_prob[int(rows[t[0]])].append(t)
    for i, s in enumerate(shapes):
        if s.M == 0 or s.N == 0:
            assert i not in by_prob
            continue
        ts = np.array(by_prob[i])
        bm, bn = _bn(v, s)
        m0s = np.unique(ts[:, 1])
        n0s = np.unique(ts[:, 2])
        assert m0s[0] == 0 and m0s[-1] < s.M and (np.diff(m0s) <= bm).all() and (np.diff(m0s) > 0).all()
        assert (n0s == np.arange(0, s.N, bn)).all(), f"problem {i}: n-tiles {n0s}"
        ks_end = None
        for m0 in m0s:
            for n0 in n0s:
                sl = ts[(ts[:, 1] == m0) & (ts[:, 2] == n0)]
                assert len(sl) >= 1, f"problem {i}: tile ({m0}, {n0}) missing"
                sl = sl[np.argsort(sl[:, 4])]
                assert sl[0, 4] == 0 and (sl[1:, 4] == sl[:-1, 5]).all()
                assert ks_end is None or sl[-1, 5] == ks_end
                ks_end = sl[-1, 5]
                if len(sl) > 1:  # split-K: one slab group, slice index / count in cls
                    assert len(set(sl[:, 7].tolist())) == 1 and ((sl[:, 3] >> 16) & 0xFF == len(sl)).all()
                    assert sorted(((sl[:, 3] >> 8) & 0xFF).tolist()) == list(range(len(sl)))
                else:
                    assert sl[0, 6] == -1 and sl[0, 7] == -1
        assert len(ts) == sum(len(ts[(ts[:, 1] == m0) & (ts[:, 2] == n0)]) for m0 in m0s for n0 in n0s)
    return tiles, rows, v


@pytest.mark.parametrize("cfg", ["fp16", "w8a8", "w4a4", "mixed", "e4m3", "w4a16", "w4a16_w8a8", "w2a16", "w8a16"])
@pytest.mark.parametrize("bs", [8192, 512, 128])
def test_every_tile_planned_once(cfg, bs):
    from mxmoe_amd.workload import w4a16_w8a8_qconfig

    kw = {"fp16": {}, "w8a8": dict(qstr="w8a8_g-1_sym"), "w4a4": dict(qstr="w4a4_g-1_sym"),
          "mixed": dict(qconfig=mixed_qconfig_lp1()), "e4m3": dict(qstr="w8a8_g-1_sym_E4M3"),
          "w4a16": dict(qstr="w4a16_g128_asym"), "w4a16_w8a8": dict(qconfig=w4a16_w8a8_qconfig()),
          "w2a16": dict(qstr="w2a16_g128_asym"), "w8a16": dict(qstr="w8a16_g-1_asym")}[cfg]
    layer = _layer(bs, **kw)
    names = [ln.split()[1] for ln in nat.list_variants()]
    for gg in ("gate_up", "down"):
        _, _, v = check_coverage(layer[gg])
        # (small-batch weight-only calls, w8a8 riding along, and fp16 / w8a8 calls at bs <= 512 plan
        # for the 3-WG/CU kernel)
        small = (cfg in ("w4a16", "w4a16_w8a8", "w2a16", "w8a16") and bs < 8192) or (cfg in ("fp16", "w8a8", "w4a4", "mixed") and bs <= 512)
        assert (names[v] == "wo3_64x256_w8_3wg") == small, (cfg, bs, gg)


def test_other_models_and_every_v2_variant():
    for model in ("ds2", "mixtral", "qwen2_moe_57b"):
        layer = next(iter(load_workload(model_workload(model, 4096)).values()))
        for gg in ("gate_up", "down"):
            check_coverage(layer[gg])
    shapes = _layer(8192)["gate_up"]
    for v in nat.production_variants():
        check_coverage(shapes, v)


def _xcd_queues(tiles):
    q = [[] for _ in range(8)]
    for b, t in enumerate(tiles):
        if t[0] >= 0:
            q[b % 8].append(t)
    return q


def _queue_parts(shapes):
    tiles, rows, v = check_coverage(shapes, nat.default_variant())
    shared = len(shapes) - 1
    return tiles, rows, shared, _xcd_queues(tiles)


@pytest.mark.parametrize("cfg", ["fp16", "w8a8", "mixed"])
@pytest.mark.parametrize("gg", ["gate_up", "down"])
def test_xcd_packing_shared_pieces(cfg, gg):
    """XCD packing (gg_plan.cpp plan_host): the shared expert's tiles are cut into
    8 consecutive pieces of its rectangle order, one per XCD queue — at the queue HEAD when its tiles
    are the long ones (down: 4x the routed K) or the call is 16-bit (fp16: low arithmetic intensity),
    at the TAIL otherwise — each piece a compact block of the tile grid (panel reuse in one L2), and the
    per-XCD piece sizes differ (they level the XCDs' modelled loads)."""
    kw = {"fp16": {}, "w8a8": dict(qstr="w8a8_g-1_sym"), "mixed": dict(qconfig=mixed_qconfig_lp1())}[cfg]
    shapes = _layer(8192, **kw)[gg]
    tiles, rows, shared, q = _queue_parts(shapes)
    head = gg == "down" or cfg == "fp16"
    mt, nt = -(-shapes[shared].M // 256), -(-shapes[shared].N // 256)
    total = 0
    for x in range(8):
        is_shared = [int(rows[t[0]]) == shared for t in q[x]]
        n = sum(is_shared)
        total += n
        assert n > 0
        if head:
            assert all(is_shared[:n]) and not any(is_shared[n:]), f"XCD {x}: shared tiles must open the queue"
        else:
            assert all(is_shared[-n:]) and not any(is_shared[:-n]), f"XCD {x}: shared tiles must close the queue"
        st = np.array([t for t, s in zip(q[x], is_shared) if s])
        m_panels, n_panels = len(np.unique(st[:, 1])), len(np.unique(st[:, 2]))
        # compact: its own rectangle plus the surplus tails it takes over (each a few columns of
        # another rectangle's band) — not the whole grid's rows (32 + 44 panels on gate_up)
        assert m_panels + n_panels <= 64 and (m_panels <= 16 or n_panels <= 16), (x, m_panels, n_panels, n)
    assert total == mt * nt


@pytest.mark.parametrize("cfg", ["fp16", "w8a8", "mixed"])
@pytest.mark.parametrize("gg", ["gate_up", "down"])
def test_routed_experts_stay_on_one_xcd(cfg, gg):
    """Every routed expert of a bs 8192 layer call runs on ONE XCD (its A / B panels in one L2): the
    packing assigns experts whole by LPT over their modelled loads; before it, the
    last 16 chunks' worth of tiles were cut into 16-tile chunks and ~15 experts spanned 2-3 XCDs."""
    kw = {"fp16": {}, "w8a8": dict(qstr="w8a8_g-1_sym"), "mixed": dict(qconfig=mixed_qconfig_lp1())}[cfg]
    shapes = _layer(8192, **kw)[gg]
    tiles, rows, _ = check_coverage(shapes, nat.default_variant())
    homes = collections.defaultdict(set)
    for b, t in enumerate(tiles):
        if t[0] >= 0:
            homes[int(rows[t[0]])].add(b % 8)
    routed = [i for i in range(len(shapes) - 1) if shapes[i].M > 0]
    assert all(len(homes[i]) == 1 for i in routed), [len(homes[i]) for i in routed]


def test_xcd_packing_levels_the_modelled_finish():
    """The planner's own tile-time model (tools/plan_model.py) on the packed plans: the down calls'
    modelled makespan over the mean per-slot load drops from 1.087-1.097 (round 5's chunked placement:
    fp16 / w8a8 / mixed) to <= 1.07, and no gate_up call gets worse than round 5's 1.054-1.059."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("plan_model", os.path.join(os.path.dirname(__file__), "..", "tools",
                                                                             "plan_model.py"))
    pm = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pm)
    for cfg, kw in (("fp16", {}), ("w8a8", dict(qstr="w8a8_g-1_sym")), ("mixed", dict(qconfig=mixed_qconfig_lp1()))):
        for gg, bound in (("gate_up", 1.06), ("down", 1.07)):
            shapes = _layer(8192, **kw)[gg]
            tiles, rows, _ = check_coverage(shapes, nat.default_variant())
            m = pm.model(shapes, tiles, rows)
            assert m["makespan_over_mean"] <= bound, (cfg, gg, m)


KNOBS = {"MXMOE_GG_BAND": "8", "MXMOE_GG_REGION": "1", "MXMOE_GG_REGION_ROT": "1", "MXMOE_GG_ALIGN": "0",
         "MXMOE_GG_TAIL_CHUNK": "4", "MXMOE_GG_XCD_RR": "1", "MXMOE_GG_NGROUP": "4"}


@pytest.mark.parametrize("cfg", ["fp16", "w8a8"])
def test_product_plan_ignores_planner_ab_switches(monkeypatch, cfg):
    """The planner's A/B switches are read only by the tools-only lab library: the product
    library's tile table does not depend on the caller's environment."""
    kw = {"fp16": {}, "w8a8": dict(qstr="w8a8_g-1_sym")}[cfg]
    for gg in ("gate_up", "down"):
        shapes = _layer(8192, **kw)[gg] + _layer(512, **kw)[gg]
        probs = _probs(shapes)
        v = nat.resolve_variant((nat.GGProblemC * len(probs))(*probs), len(probs), nat.VARIANT_AUTO)
        base, rows = nat.plan_tiles(probs, v)
        for k, val in KNOBS.items():
            monkeypatch.setenv(k, val)
        knobbed, rows2 = nat.plan_tiles(probs, v)
        for k in KNOBS:
            monkeypatch.delenv(k)
        assert np.array_equal(base, knobbed) and np.array_equal(rows, rows2)


def test_product_library_lists_only_correct_variants():
    names = [ln.split()[1] for ln in nat.list_variants()]
    assert names and not any(n.startswith(("abl_", "x_")) for n in names)
    assert nat.production_variants(None) == list(range(len(names)))


def cross_xcd_split_groups(tiles) -> int:
    """Split-K groups whose slices sit on more than one XCD queue (blockIdx % 8)."""
    homes = collections.defaultdict(set)
    for b, t in enumerate(tiles):
        if t[0] >= 0 and t[7] >= 0:
            homes[int(t[7])].add(b % 8)
    return sum(len(x) > 1 for x in homes.values())


@pytest.mark.parametrize("wa,K", [((8, 8), 4224), ((4, 4), 4224), ((16, 16), 1408)], ids=["w8a8", "w4a4", "fp16"])
def test_tail_chunks_scatter_split_slices_across_xcds(wa, K):
    """A split group with 5 or 8 slices straddles the 16-entry tail chunks, so its slices land on
    different XCDs (different L2s). tests/test_gg_gpu.py::test_splitk_slices_on_different_xcds runs
    these shapes on the GPU; this pins that they keep exercising the cross-L2 hand-off."""
    from mxmoe_amd.workload import QShape

    shapes = [QShape([128, 2048, K], *wa), QShape([40, 256, 1408], *wa)]
    tiles, _, _ = check_coverage(shapes)
    assert cross_xcd_split_groups(tiles) > 0


def test_lab_planner_knobs_plan_the_small_batch_kernel():
    """The lab library's planner A/B switches on the 3-WG/CU small-batch kernel, whose XCD chunk is 96
    slots: plain round-robin or unaligned chunks take a whole chunk at once (a fixed 64-entry buffer
    overflowed there until round 6). Runs the lab library in a subprocess (CPU: planning only); skips
    when the lab library is absent or older than its sources."""
    import subprocess
    import sys

    from mxmoe_amd import build

    if not build.LAB_LIB.exists() or build.needs_build(build.LAB_LIB):
        pytest.skip("lab library absent or stale")
    code = (
        "import numpy as np\n"
        "from mxmoe_amd import _native as nat\n"
        "from mxmoe_amd.workload import load_workload, qwen2_layer11_workload, w4a16_w8a8_qconfig\n"
        "from tests.test_planner import _probs\n"
        "names = [l.split()[1] for l in nat.list_variants()]\n"
        "v = names.index('x_wo3_pch')\n"
        "for gg in ('gate_up', 'down'):\n"
        "    probs = _probs(load_workload(qwen2_layer11_workload(512, qconfig=w4a16_w8a8_qconfig()))['layer-11'][gg])\n"
        "    tiles, rows = nat.plan_tiles(probs, v)\n"
        "    assert (tiles[:, 0] >= 0).sum() > 0\n"
        "print('ok')\n")
    for knob in ("MXMOE_GG_XCD_RR=1", "MXMOE_GG_ALIGN=0", "MXMOE_GG_TAIL_CHUNK=96"):
        k, val = knob.split("=")
        env = dict(os.environ, MXMOE_GG_LIB=str(build.LAB_LIB), **{k: val})
        r = subprocess.run([sys.executable, "-c", code], cwd=str(build.ROOT),
                           env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "ok" in r.stdout, (knob, r.returncode, r.stderr[-800:])


def test_host_planner_under_host_sanitizers(tmp_path):
    """tests/cpp/plan_host_check.cpp: the host planner (gg_plan.cpp) with the product's three variants, built
    with the host compiler alone and -fsanitize=address,undefined, run as a program of its own: the coverage
    check_coverage asserts, on the Plan itself, over the tile classes, split-K, XCD regions, the packed MoE call
    shape and every validation error."""
    import shutil
    import subprocess

    from mxmoe_amd import build

    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "plan_host_check"
    r = subprocess.run([cxx, *flags, "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                        str(build.ROOT / "tests" / "cpp" / "plan_host_check.cpp"), str(build.CSRC / "gg_plan.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("plan_host_check ok")
