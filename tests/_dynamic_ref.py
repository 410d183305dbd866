"""Restatements for the device-planning tests, independent of the code under test: the segment table of
``mxmoe_amd.moe._make_segments`` in plain integers (no torch, no device), and the host planner's m-tile rule."""
from __future__ import annotations

BITS = {0: 16, 1: 8, 2: 4, 3: 4, 4: 4, 6: 8}  # MXMOE_ACT_* -> bits per element
MX_TAGS = (4, 6)


def mx_scale_row(width: int) -> int:
    """e8m0 bytes per row in the GroupGEMM's device layout: whole groups of 16 blocks of 32 elements."""
    return 16 * ((width // 32 + 15) // 16)


def segments_ref(counts, T: int, topk: int, qtags, width: int, width_shared: int = 0, ldc: int = 0):
    """[(qtag, first_slot, rows, width, out_off, scale_off)] and the GroupGEMM rows [(rows, a_off, sa_off, c_off)]
    for the routing counts; len(qtags) == len(counts) + 1 adds the shared segment (rows = T, slots from T * topk)."""
    E = len(counts)
    segs, dyn, off, soff, first = [], [], 0, 0, 0
    for e, tag in enumerate(qtags):
        shared = e == E
        r, f, w = (T, T * topk, width_shared) if shared else (int(counts[e]), first, width)
        if tag in MX_TAGS and soff % 2:
            soff += 1  # dword-read scale bytes: a 4-byte aligned block (2 fp16 elements)
        segs.append((tag, f, r, w, off, soff))
        dyn.append((r, off, 2 * soff, 0 if shared else 2 * f * ldc))
        off += -(-(r * w * BITS[tag] // 8) // 16) * 16
        if tag in MX_TAGS:
            soff += r * mx_scale_row(w) // 2
        elif tag == 3:
            soff += r * (w // 128)
        elif tag != 0:
            soff += r
        first += 0 if shared else r
    return segs, dyn


def m_tiles_ref(M: int, bm: int, tail_bm: int, tail2_bm: int):
    """[(m0, class)] by the host rule: main tiles while more than tail_bm rows remain, then one 64-row
    (tail2_bm, if the type takes it) or 128-row tile."""
    out, m0 = [], 0
    while m0 < M:
        rem = M - m0
        if tail2_bm and rem <= tail2_bm:
            out.append((m0, 2))
            m0 += tail2_bm
        elif tail_bm and rem <= tail_bm:
            out.append((m0, 1))
            m0 += tail_bm
        else:
            out.append((m0, 0))
            m0 += bm
    return out
