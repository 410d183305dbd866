"""CPU tests of device planning (DESIGN.md §4 "Device planning / graph forward"): the tile planner the GPU
runs (mxmoe_amd/csrc/gg_dyn.h), executed on the host through mxmoe_gg_dynamic_tiles, against the host planner
(mxmoe_gg_plan_tiles) — the same tile set for the same rows, the capacity bound never exceeded, bad row tables
only ever clamped and flagged; the device segment table (mxmoe_moe_segments_host) against moe._make_segments; and
the planner's functions under the host compiler's sanitizers (tests/cpp/dyn_plan_check.cpp, a program of its own).
"""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from mxmoe_amd import _native as nat
from tests._dynamic_ref import BITS, m_tiles_ref, segments_ref

ROOT = Path(__file__).resolve().parent.parent
BOUNDARY_ROWS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 513]
N, K = 384, 512

# (a_bits, w_bits, gsize, sym, fmt)
TYPES = {
    "fp16": (16, 16, -1, 1, nat.FMT_DEFAULT),
    "w8a8": (8, 8, -1, 1, nat.FMT_DEFAULT),
    "w4a4": (4, 4, -1, 1, nat.FMT_DEFAULT),
    "w4a16": (16, 4, 128, 0, nat.FMT_DEFAULT),
    "mxfp4": (4, 4, 32, 1, nat.FMT_MXFP4),
    "mxfp4_a16": (16, 4, 32, 1, nat.FMT_MXFP4),
    "mxfp8": (8, 4, 32, 1, nat.FMT_MXFP8),
    "g128": (4, 4, 128, 1, nat.FMT_DEFAULT),
}
VARIANT_TYPES = {
    "v2x_256x256_w8_b3_buf_spread_edma": ["fp16", "w8a8", "w4a4", "w4a16", "mxfp4", "mxfp4_a16", "mxfp8", "g128"],
    "v3_256x128_w4_dma_ring3_2wg": ["fp16", "w8a8", "w4a4"],
    "wo3_64x256_w8_3wg": ["fp16", "w8a8", "w4a4", "w4a16", "mxfp4_a16", "mxfp8"],
}
CASES = [(v, t) for v, ts in VARIANT_TYPES.items() for t in ts]


def variant_index(name: str) -> int:
    for ln in nat.list_variants():
        if ln.split()[1] == name:
            return int(ln.split()[0])
    raise AssertionError(f"variant {name} not compiled")


def prob(kind: str, M: int, n: int = N, k: int = K) -> nat.GGProblemC:
    a, w, g, sym, fmt = TYPES[kind]
    return nat.GGProblemC(A=0, B=0, scale_a=0, scale_b=0, C=0, M=M, N=n, K=k, a_bits=a, w_bits=w, gsize=g, sym=sym,
                          fmt=fmt, lda=0, ldb=0, ldc=0)


def host_tile_set(kinds, rows, v, n=N):
    """{(problem, m0, n0, class)} of the host plan of these rows (split-K slices merged by the set)."""
    tiles, order = nat.plan_tiles([prob(k, r, n) for k, r in zip(kinds, rows)], v)
    live = tiles[tiles[:, 0] >= 0]
    return {(int(order[t[0]]), int(t[1]), int(t[2]), int(t[3]) & 0xFF) for t in live}


def dyn_tiles(kinds, caps, joint, rows_total, rows, v, n=N, **kw):
    tiles, planned, status = nat.dynamic_tiles([prob(k, c, n) for k, c in zip(kinds, caps)], v, joint, rows_total,
                                               [(r, 0, 0, 0) for r in rows], **kw)
    live = tiles[tiles[:, 0] >= 0]
    assert len(live) == 0 or (np.flatnonzero(tiles[:, 0] >= 0).max() == len(live) - 1), "planned tiles are not a prefix"
    assert (live[:, 4] == 0).all() and (live[:, 6] == -1).all() and (live[:, 7] == -1).all()  # no split-K
    keys = [(int(t[0]), int(t[1]), int(t[2]), int(t[3])) for t in live]
    assert len(set(keys)) == len(keys), "a tile is planned twice"
    return set(keys), planned, status, len(tiles)


@pytest.mark.parametrize("variant,kind", CASES)
def test_tile_set_matches_host_planner_at_boundaries(variant, kind):
    """★ One problem per boundary row count, all routed: the device rule plans the host planner's tile set."""
    v = variant_index(variant)
    rows = BOUNDARY_ROWS
    R = sum(rows)
    kinds = [kind] * len(rows)
    got, planned, status, slots = dyn_tiles(kinds, [R] * len(rows), range(len(rows)), R, rows, v)
    assert status == 0 and planned.tolist() == rows
    assert got == host_tile_set(kinds, rows, v)
    assert len(got) <= slots


@pytest.mark.parametrize("variant", list(VARIANT_TYPES))
def test_tile_set_matches_host_planner_random_counts(variant):
    """A few hundred seeded count vectors (E <= 64, R <= 4096) of mixed types, with a shared problem: the same
    tile set as the host planner, inside the capacity bound, nothing clamped."""
    v = variant_index(variant)
    rng = np.random.default_rng(20260101)
    kinds_ok = VARIANT_TYPES[variant]
    for it in range(120):
        E = int(rng.integers(1, 65))
        R = int(rng.integers(1, 4097))
        T = int(rng.integers(1, 600))
        hot = rng.integers(0, E, size=max(1, E // 4))  # a skewed routing: a quarter of the experts take most rows
        ids = np.where(rng.random(R) < 0.7, rng.choice(hot, R), rng.integers(0, E, R))
        counts = np.bincount(ids, minlength=E).tolist()
        kinds = [kinds_ok[int(j)] for j in rng.integers(0, len(kinds_ok), E + 1)]
        n = int(rng.choice([128, 384, 1408]))
        got, planned, status, slots = dyn_tiles(kinds, [R] * E + [T], range(E), R, counts + [T], v, n=n)
        assert status == 0 and planned.tolist() == counts + [T]
        assert got == host_tile_set(kinds, counts + [T], v, n=n), (it, E, R, T)
        assert len(got) <= slots


def _geom(v, kind):
    a, w = TYPES[kind][0], TYPES[kind][1]
    t = nat.variant_tile(v, a, w)
    return t["BM"], t["BN"]


@pytest.mark.parametrize("variant", list(VARIANT_TYPES))
@pytest.mark.parametrize("E,T,topk", [(4, 60, 2), (60, 1, 4), (60, 7, 4), (64, 300, 6), (8, 1024, 2)])
def test_capacity_bound_holds_and_is_tight(variant, E, T, topk):
    """Adversarial routings never need more than tile_slots: all rows on one expert, one row on each, every
    expert one past a tile boundary. The bound is attained by one of them (it is not loose by construction)."""
    v = variant_index(variant)
    kind = "w8a8"
    bm, bn = _geom(v, kind)
    R = T * topk
    kinds = [kind] * (E + 1)
    caps = [R] * E + [T]
    tables = [[R] + [0] * (E - 1), [0] * (E - 1) + [R]]
    one_each = [1] * min(E, R) + [0] * (E - min(E, R))
    one_each[0] += R - sum(one_each)
    tables.append(one_each)
    for step in (bm, 128, 64):
        t, left = [], R
        for _ in range(E):
            t.append(min(step + 1, left))
            left -= t[-1]
        tables.append(t)
    used = []
    for t in tables:
        got, planned, status, slots = dyn_tiles(kinds, caps, range(E), R, t + [T], v)
        assert status == 0 and planned.tolist() == t + [T]
        assert len(got) <= slots
        want = sum(-(-N // bn) * len(m_tiles_ref(r, bm, 0, 0)) for r in t + [T])
        assert len(got) == want
        used.append(len(got))
    tn = -(-N // bn)
    shared = tn * -(-T // bm)
    n = min(E, R)  # non-empty experts: their first rows open a tile each, the other R - n rows fill tiles
    assert slots == shared + min(E * tn * -(-R // bm), n * tn + tn * ((R - n) // bm))
    assert max(used) == slots, (used, slots)


def test_classes_follow_the_host_rule():
    """The class bits against a restatement of the rule: 256-row tiles while more than 128 rows remain, then one
    128-row tile, or one 64-row tile for the types that take it (fp16 on v2x; w8a8 has no 64-row class)."""
    v = variant_index("v2x_256x256_w8_b3_buf_spread_edma")
    for kind, tail2 in (("fp16", 64), ("w8a8", 0), ("w4a16", 64), ("mxfp4", 0)):
        for rows in BOUNDARY_ROWS + [300, 384, 385, 512, 640, 641]:
            got, _, status, _ = dyn_tiles([kind], [1024], [0], 1024, [rows], v, n=128)
            assert status == 0
            assert sorted((m0, c) for _, m0, _, c in got) == m_tiles_ref(rows, 256, 128, tail2), (kind, rows)


@pytest.mark.parametrize("variant", list(VARIANT_TYPES))
def test_bad_row_tables_are_clamped_and_flagged(variant):
    """Rows above a capacity, a joint sum above rows_total, a slot table cut short, offsets outside the extents:
    the planned tiles stay inside the capacities and the matching status bit is set. (CPU only: a GPU test must
    not feed the planner bad counts.)"""
    v = variant_index(variant)
    E, T, R = 4, 60, 120
    kinds = ["w8a8", "w4a4", "fp16", "w8a8", "fp16"]
    caps = [100, 100, 100, 100, T]
    bm = _geom(v, "w8a8")[0]

    def inside(got, planned):
        assert (planned >= 0).all() and (planned <= np.array(caps)).all() and planned[:E].sum() <= R
        for p, m0, n0, _ in got:
            assert 0 <= m0 < planned[p] and 0 <= n0 < N

    got, planned, status, _ = dyn_tiles(kinds, caps, range(E), R, [500, 0, -4, 0, T + 9], v)
    assert status == nat.DYN_ROWS_CLAMPED and planned.tolist() == [100, 0, 0, 0, T]
    inside(got, planned)
    got, planned, status, _ = dyn_tiles(kinds, caps, range(E), R, [90, 90, 90, 90, T], v)
    assert status == nat.DYN_JOINT_CLAMPED and planned.tolist() == [90, 30, 0, 0, T]
    inside(got, planned)
    full, _, _, slots = dyn_tiles(kinds, caps, range(E), R, [30, 30, 30, 30, T], v)
    got, planned, status, n = dyn_tiles(kinds, caps, range(E), R, [30, 30, 30, 30, T], v, slot_limit=len(full) - 1)
    assert n == len(full) - 1 and status == nat.DYN_SLOTS_CUT and len(got) < len(full) and got < full
    inside(got, planned)
    # offsets: extents of exactly the capacities, so any positive offset on a full problem leaves the buffer
    P = [prob(k, c) for k, c in zip(kinds, caps)]
    for field, bad in ((1, 16), (3, 16), (1, -16), (3, 8), (2, 1), (1, 1 << 62)):
        rows = [[100, 0, 0, 0] for _ in range(E)] + [[T, 0, 0, 0]]
        rows[0][0] = 100 if field != 2 else 100
        rows[0][field] = bad
        tiles, planned, status = nat.dynamic_tiles(P, v, range(E), 1000, rows)
        assert status == nat.DYN_BAD_OFFSET and planned.tolist() == [0, 100, 100, 100, T], (field, bad)
        assert not (tiles[:, 0] == 0).any()
    rows = [[40, 60 * K, 0, 60 * 2 * N]] + [[0, 0, 0, 0]] * (E - 1) + [[T, 0, 0, 0]]  # an offset that fits: accepted
    tiles, planned, status = nat.dynamic_tiles(P, v, range(E), 1000, rows)
    assert status == 0 and planned[0] == 40 and bm > 0


def test_validation_matches_the_host_plan():
    """The same errors from the same type tables as mxmoe_gg_plan_tiles; lab / persistent variants and bad joint
    lists are refused."""
    v = variant_index("v3_256x128_w4_dma_ring3_2wg")
    for bad in (prob("w4a16", 64), prob("w8a8", 64, k=K + 8), prob("fp16", 64, n=N + 4)):
        with pytest.raises(nat.GGError) as host:
            nat.plan_tiles([bad], v)
        with pytest.raises(nat.GGError) as dyn:
            nat.dynamic_tiles([bad], v, [0], 64, [(1, 0, 0, 0)])
        assert dyn.value.status == host.value.status and str(dyn.value) == str(host.value)
    for joint in ([0, 0], [2], [-1]):
        with pytest.raises(nat.GGError) as e:
            nat.dynamic_tiles([prob("w8a8", 64), prob("w8a8", 64)], v, joint, 64, [(1, 0, 0, 0)] * 2)
        assert e.value.status == nat.MXMOE_GG_ERR_INVALID
    with pytest.raises(nat.GGError) as e:
        nat.dynamic_tiles([prob("w8a8", 64)], nat.variant_count(), [0], 64, [(1, 0, 0, 0)])
    assert e.value.status == nat.MXMOE_GG_ERR_UNSUPPORTED


def test_auto_resolves_for_the_balanced_call():
    """AUTO at capacity = mxmoe_gg_resolve_variant of the call with rows_total spread evenly over the joint set."""
    for E, R, T, kinds in ((60, 512, 128, ["w8a8"]), (60, 32768, 8192, ["w8a8"]), (8, 4096, 64, ["w4a4"]),
                           (60, 512, 128, ["w4a16"])):
        ks = (kinds * E)[:E] + [kinds[0]]
        share = -(-R // E)
        bal = [prob(k, share, 1408, 2048) for k in ks[:E]] + [prob(ks[E], T, 1408, 2048)]
        want = nat.resolve_variant((nat.GGProblemC * len(bal))(*bal), len(bal))
        caps = [prob(k, R, 1408, 2048) for k in ks[:E]] + [prob(ks[E], T, 1408, 2048)]
        rows = [(share, 0, 0, 0)] * E + [(T, 0, 0, 0)]
        auto = nat.dynamic_tiles(caps, nat.VARIANT_AUTO, range(E), R, rows)[0]
        fixed = nat.dynamic_tiles(caps, want, range(E), R, rows)[0]
        assert (auto == fixed).all() and len(auto) > 0


MIXED_TAGS = [1, 2, 0, 3, 4, 6, 2, 1]  # int8, int4, fp16, g128, MXFP4, MXFP8, ...


@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("counts", [[5, 0, 17, 0, 3, 1, 0, 38], [0] * 7 + [64], [8] * 8, [1, 3, 5, 7, 9, 11, 13, 15]])
def test_segment_table_equals_make_segments(counts, shared):
    """mxmoe_moe_segments' function on the host == moe._make_segments field for field (mixed tags, empty experts,
    the odd scale offsets the MX tags must round up), and the GroupGEMM row table follows from it."""
    from mxmoe_amd import moe

    topk = 4
    T = sum(counts) // topk
    E = len(counts)
    tags = MIXED_TAGS[:E] + ([6] if shared else [])
    W, Ws, ldc = 256, 384, 520
    first = np.concatenate([[0], np.cumsum(counts)[:-1]]).tolist()
    rows = counts + ([T] if shared else [])
    want, _, out, scales = moe._make_segments(rows, first + ([T * topk] if shared else []),
                                              [W] * E + ([Ws] if shared else []), tags, "cpu")
    segs, dyn, status = nat.segments_host(counts, T, topk, tags, W, Ws if shared else 0, ldc)
    assert status == 0
    fields = [f for f, _ in nat.MoeSegC._fields_]
    assert [[getattr(s, f) for f in fields] for s in segs] == [[getattr(s, f) for f in fields] for s in want]
    ref_segs, ref_dyn = segments_ref(counts, T, topk, tags, W, Ws, ldc)
    assert [tuple(getattr(s, f) for f in fields) for s in segs] == ref_segs
    assert [(d.rows, d.a_off, d.sa_off, d.c_off) for d in dyn] == ref_dyn
    last = segs[-1]  # the table ends where _make_segments' store does
    end = last.out_off + -(-(last.rows * last.width * BITS[last.qtag] // 8) // 16) * 16
    assert max(end, 16) == out.numel() and scales.numel() >= 1


def test_segment_table_flags_counts_that_do_not_sum():
    tags = [1, 1, 1, 1]
    assert nat.segments_host([3, 3, 3, 3], 3, 4, tags, 128)[2] == 0
    segs, _, status = nat.segments_host([3, 3, 3, 2], 3, 4, tags, 128)  # an id outside [0, E) was dropped
    assert status == nat.SEG_COUNT_MISMATCH and [s.rows for s in segs] == [3, 3, 3, 2]
    segs, _, status = nat.segments_host([9, 9, -1, 9], 3, 4, tags, 128)  # not route's counts: clamped to T * topk rows
    assert status == nat.SEG_COUNT_MISMATCH and [s.rows for s in segs] == [9, 3, 0, 0]


def test_planner_functions_under_host_sanitizers(tmp_path):
    """tests/cpp/dyn_plan_check.cpp: the planner's functions and the capacity formula over adversarial row tables,
    built with the host compiler and -fsanitize=address,undefined, run as a program of its own."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    if subprocess.run([cxx, *flags, "-o", str(tmp_path / "probe"), str(probe)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("the host compiler has no address / undefined-behaviour sanitizer runtime")
    exe = tmp_path / "dyn_plan_check"
    r = subprocess.run([cxx, *flags, "-Wall", "-Wextra", "-Werror", "-o", str(exe),
                        str(ROOT / "tests" / "cpp" / "dyn_plan_check.cpp")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("dyn_plan_check ok")
