"""MoE-layer plumbing around the GroupGEMM, on the C-ABI of include/mxmoe_moe.h.

Reference interface mirrored (SeaCatComplexes/MxMoE, mxmoe/kernels/src/ref_bind.cu, pybind module
``mxmoe_ops``):
  * ``gg_permute_inp(hidden, topk_ids, E)`` ............................ ref_bind.cu:47-64
  * ``quant_inp_act(hidden, topk_ids, num_experts, N, num_shared_experts, qparams_per_exp)``
    -> (inp_list, inp_scale_list, out_list, inp_store, inp_scale_store, out_store,
        recv_tokens_per_exp, perm_indices, dst_exp_sorted) .................. :434-592
  * ``silu_mul_then_quant(inp, num_problems, num_experts, K, N, num_shared_experts, num_tokens, topk,
    values_sorted, recv_tokens_per_exp, qparams_per_exp)``
    -> (inp_list, inp_scale_list, out_list, inp_store, inp_scale_store, out_store) ... :595-757
  * the per-expert quant tag ``cvt_qparams_to_tag`` ...................... :467-479
  * ``gg_unpermute_out`` (an empty stub in the reference, :66) -> ``combine``
and ``MoEFFN``: route -> quant_inp_act -> fused gate_up GroupGEMM -> silu_mul_then_quant -> fused
down GroupGEMM -> combine, the layer the reference's ``gg_mxmoe_share_fused`` path builds toward.

Differences by design: the routing is a device counting sort (mxmoe_moe_route) instead of
torch::sort + bincount; the only host synchronisation is reading the per-expert token counts (the
reference also moves them to the host: ``.cpu()`` at :456), which the tile planner needs anyway.
The quantised activations are written in exactly the GroupGEMM operand layout: pack_wxax rows,
per-token scales [rows] or, for w4a4 g128, [K/128][rows] (permute_scale layout).
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import math
from typing import Optional, Sequence

import torch

from . import _native as nat
from .groupgemm import DynamicGroupGemm, GroupGemm, Problem, QParams

ACT_FP16, ACT_INT8, ACT_INT4, ACT_INT4_G128, ACT_MXFP4 = 0, 1, 2, 3, 4
ACT_MXFP8 = 6  # MXMOE_ACT_MXFP8 (w4a8_g32_sym_MXFP8); 5 is not assigned (include/mxmoe_moe.h)
ACT_E4M3 = 8   # MXMOE_ACT_E4M3 (w8a8_g-1_sym_E4M3: e4m3 codes, one fp16 scale per token); 7 is not assigned either
_BITS = {ACT_FP16: 16, ACT_INT8: 8, ACT_INT4: 4, ACT_INT4_G128: 4, ACT_MXFP4: 4, ACT_MXFP8: 8, ACT_E4M3: 8}
_MX_TAGS = (ACT_MXFP4, ACT_MXFP8)  # block-scaled tags: e8m0 scale rows, the MX builds of the activation kernel


def _mx_scale_row(width: int) -> int:
    """e8m0 scale bytes per row of an MXFP4 segment (the GroupGEMM's device layout, include/mxmoe_gg.h)."""
    return 16 * ((width // 32 + 15) // 16)


def _scale_elems(tag: int, width: int) -> int:
    """fp16 elements of scale store per row of a segment: the MX tags' e8m0 bytes two to an element, one scale per
    128-element group for g128, none for fp16, else (INT8, INT4, E4M3) one per row."""
    if tag in _MX_TAGS:
        return _mx_scale_row(width) // 2
    return width // 128 if tag == ACT_INT4_G128 else 0 if tag == ACT_FP16 else 1


def qtag_of(a_bits: int, gsize: int, fmt: str = "") -> int:
    """The reference's cvt_qparams_to_tag (ref_bind.cu:467-479); unsupported -> ValueError. ``fmt``: the QParams'
    operand format; it matters for (8, -1) alone, where "E4M3" (w8a8_g-1_sym_E4M3) is a tag of its own and anything
    else the integer one. A call without it behaves as before the E4M3 tag existed."""
    if a_bits >= 16:
        return ACT_FP16
    if a_bits == 8 and gsize == -1 and fmt == "E4M3":
        return ACT_E4M3
    if a_bits == 8 and gsize == -1:
        return ACT_INT8
    if a_bits == 4 and gsize == -1:
        return ACT_INT4
    if a_bits == 4 and gsize == 128:
        return ACT_INT4_G128
    if a_bits == 4 and gsize == 32:  # w4a4_g32_sym_MXFP4 (no integer g32 type exists)
        return ACT_MXFP4
    if a_bits == 8 and gsize == 32:  # w4a8_g32_sym_MXFP8 (likewise)
        return ACT_MXFP8
    raise ValueError(f"activation quantisation a{a_bits} g{gsize} not supported")


def _tag_mask(qtags: Sequence[int]) -> int:
    """mxmoe_moe_act_quant's tag_mask: bit t set when a segment carries tag t."""
    m = 0
    for t in qtags:
        m |= 1 << t
    return m


def _stream(stream: Optional[torch.cuda.Stream]) -> ctypes.c_void_p:
    s = stream if stream is not None else torch.cuda.current_stream()
    return ctypes.c_void_p(int(s.cuda_stream))


def _ptr(t: Optional[torch.Tensor]) -> Optional[ctypes.c_void_p]:
    return None if t is None else ctypes.c_void_p(t.data_ptr())


@dataclasses.dataclass
class Routing:
    """Result of mxmoe_moe_route: slots sorted by expert (stable in token-major order)."""

    sorted_expert: torch.Tensor  # int32 [T*topk] (the reference's values_sorted / dst_exp_sorted)
    perm_token: torch.Tensor     # int32 [T*topk] (perm_indices)
    inv_slot: torch.Tensor       # int32 [T*topk]: slot of (token t, choice k) at t*topk + k
    counts: list[int]            # host copy of recv_tokens_per_exp [E]
    T: int
    topk: int
    E: int

    @property
    def first_slot(self) -> list[int]:
        out, acc = [], 0
        for c in self.counts:
            out.append(acc)
            acc += c
        return out


# The element types of a layer's two ends (hidden, the router's weights, out): MXMOE_DT_* of include/mxmoe_moe.h.
# Everything between them (activation stores, h1, y, biases) is fp16 whatever the ends are.
_DT = {torch.float16: nat.DT_FP16, torch.bfloat16: nat.DT_BF16}


def _check_io_dtype(dtype, what: str) -> None:
    if dtype not in _DT:
        raise ValueError(f"{what} must be fp16 or bf16, got {dtype}")


GATE_SCORING = {"softmax": 0, "sigmoid": 1}  # MXMOE_GATE_SOFTMAX / MXMOE_GATE_SIGMOID (include/mxmoe_moe.h)
# beyond GATE_GROUPS_MAX_E experts the router is mxmoe_moe_gate_wide's kernel: up to GATE_MAX_E, one group
GATE_GROUPS_MAX_E, GATE_MAX_E = 256, 512


def gate_routing_args(E: int, topk: int, scoring: str = "softmax", e_bias: Optional[torch.Tensor] = None,
                      n_group: int = 1, topk_group: int = 1, group_top: Optional[int] = None,
                      routed_scaling_factor: float = 1.0, return_scores: bool = False):
    """Check the routing arguments ``gate`` and ``MoEBlock`` share as mxmoe_moe_gate_ex does (ValueError);
    returns (group_top resolved, whether the call is mxmoe_moe_gate's, i.e. everything at its default)."""
    if scoring not in GATE_SCORING:
        raise ValueError(f"scoring must be 'softmax' or 'sigmoid', got {scoring!r}")
    n_group, topk_group = int(n_group), int(topk_group)
    if E > GATE_MAX_E:
        raise ValueError(f"the router takes at most {GATE_MAX_E} experts, got E = {E}")
    if E > GATE_GROUPS_MAX_E and n_group > 1:
        raise ValueError(f"group-limited routing needs E <= {GATE_GROUPS_MAX_E} (mxmoe_moe_gate_wide routes without "
                         f"groups), got E = {E}, n_group = {n_group}")
    # (a multiple of 4 experts per group: the group stage's layout, which the kernel for E > 256 does not have)
    if not 1 <= n_group <= 8 or E % n_group or (E <= GATE_GROUPS_MAX_E and (E // n_group) % 4):
        raise ValueError(f"n_group must be in [1, 8] and split E = {E} into groups of a multiple of 4 experts, got {n_group}")
    gs = E // n_group
    if not 1 <= topk_group <= n_group:
        raise ValueError(f"topk_group must be in [1, n_group = {n_group}], got {topk_group}")
    if topk > topk_group * gs:
        raise ValueError(f"topk = {topk} exceeds the {topk_group * gs} experts of {topk_group} kept groups")
    if group_top is None:
        group_top = 2 if scoring == "sigmoid" and n_group > 1 else 1
    if group_top not in (1, 2) or group_top > gs or (E > GATE_GROUPS_MAX_E and group_top != 1):
        raise ValueError(f"group_top must be 1 or 2 and at most the group size {gs} (1 for E > {GATE_GROUPS_MAX_E}), "
                         f"got {group_top}")
    if scoring == "softmax" and (e_bias is not None or group_top != 1 or return_scores):
        raise ValueError("softmax scoring takes no e_bias, no return_scores and group_top = 1")
    if e_bias is not None and (e_bias.dtype != torch.float32 or not e_bias.is_contiguous() or tuple(e_bias.shape) != (E,)):
        raise ValueError(f"e_bias must be a contiguous f32 [{E}] tensor")
    if not math.isfinite(routed_scaling_factor):
        raise ValueError(f"routed_scaling_factor must be finite, got {routed_scaling_factor}")
    plain = (scoring == "softmax" and n_group == 1 and float(routed_scaling_factor) == 1.0)
    return group_top, plain


def _check_logit_bias(logit_bias: Optional[torch.Tensor], E: int, device=None) -> None:
    if logit_bias is None:
        return
    if logit_bias.dtype != torch.float32 or not logit_bias.is_contiguous() or tuple(logit_bias.shape) != (E,):
        raise ValueError(f"logit_bias must be a contiguous f32 [{E}] tensor")
    if device is not None and logit_bias.device != device:
        raise ValueError("logit_bias must be on hidden's device")


def gate(hidden: torch.Tensor, w_gate: torch.Tensor, topk: int, *, renormalize: bool = False,
         w_shared_gate: Optional[torch.Tensor] = None, return_logits: bool = False,
         stream: Optional[torch.cuda.Stream] = None, out=None, scoring: str = "softmax",
         e_bias: Optional[torch.Tensor] = None, n_group: int = 1, topk_group: int = 1,
         group_top: Optional[int] = None, routed_scaling_factor: float = 1.0, return_scores: bool = False,
         logit_bias: Optional[torch.Tensor] = None):
    """The router (mxmoe_moe_gate / mxmoe_moe_gate_ex, one launch): hidden fp16 [T, H], w_gate fp16 [E, H] ->
    (topk_ids int32 [T, topk], topk_weights f32 [T, topk], shared_w f32 [T] or None), and the f32
    [T, E] logits as a fourth item with ``return_logits``. Selection on the logits (ties: lower index),
    weights = softmax over all E experts, or over the chosen topk with ``renormalize``; with
    ``w_shared_gate`` (fp16 [H]) shared_w = sigmoid(hidden @ w_shared_gate). ``out``: the tuple a
    previous call with the same arguments returned, to relaunch on its buffers.

    The other models' rules (semantics: include/mxmoe_moe.h, mxmoe_moe_gate_ex): ``scoring="sigmoid"``
    selects on sigmoid(logit) + ``e_bias`` (f32 [E]) and weighs by the unbiased score (over the chosen
    scores' sum with ``renormalize``); ``n_group`` / ``topk_group`` keep the topk_group best of n_group
    contiguous expert groups, a group scored by its best selection value (``group_top=1``, the softmax
    default) or the sum of its two best (2, the default for sigmoid with groups);
    ``routed_scaling_factor`` multiplies the weights; ``return_scores`` appends the f32 [T, E] sigmoid
    scores after the logits, if any. DeepSeek-V3: scoring="sigmoid", e_bias, n_group=8, topk_group=4,
    renormalize=True, routed_scaling_factor=2.5. With all of these at their defaults the call is
    mxmoe_moe_gate's.

    ``logit_bias`` (f32 [E]; mxmoe_moe_gate_ex2): added to the logits before everything else — the returned
    logits, the selection and the weights all see the sum (the shared gate does not). gpt-oss:
    ``renormalize=True, logit_bias=router.bias`` (top-k on the biased logits, softmax over the chosen ones).

    More than 256 experts (up to 512; mxmoe_moe_gate_wide, still one launch): every rule above except the groups
    (``n_group`` must be 1). Kimi-K2: E 384, ``scoring="sigmoid", e_bias, renormalize=True,
    routed_scaling_factor=2.827``; Qwen3-Next: E 512, ``renormalize=True, w_shared_gate``.

    bf16: ``hidden``, ``w_gate`` and ``w_shared_gate`` may all be bf16 instead (one dtype per call; a mix raises).
    The logits are then bf16 x bf16 products — each exact in f32 — accumulated in f32 on the bf16 MFMA
    (mxmoe_moe_gate_dt, whatever E and the rules are): nothing is rounded to fp16 on the way, and everything after
    the logits is the same code."""
    if hidden.dim() != 2 or hidden.dtype not in _DT or not hidden.is_contiguous():
        raise ValueError("hidden must be a contiguous fp16 or bf16 [T, H] tensor")
    T, H = hidden.shape
    dt = hidden.dtype
    if w_gate.dim() != 2 or w_gate.dtype != dt or not w_gate.is_contiguous() or w_gate.shape[1] != H:
        raise ValueError(f"w_gate must be a contiguous [E, {H}] tensor of hidden's dtype ({dt}), got {w_gate.dtype} "
                         f"{list(w_gate.shape)}")
    E = w_gate.shape[0]
    sg = w_shared_gate
    if sg is not None and (sg.dtype != dt or not sg.is_contiguous() or sg.numel() != H):
        raise ValueError(f"w_shared_gate must be a contiguous tensor of {H} elements of hidden's dtype ({dt})")
    group_top, plain = gate_routing_args(E, topk, scoring, e_bias, n_group, topk_group, group_top,
                                         routed_scaling_factor, return_scores)
    dev = hidden.device
    if e_bias is not None and e_bias.device != dev:
        raise ValueError("e_bias must be on hidden's device")
    _check_logit_bias(logit_bias, E, dev)
    want = [((T, topk), torch.int32), ((T, topk), torch.float32), ((T,), torch.float32) if sg is not None else None]
    want += [((T, E), torch.float32)] * (int(bool(return_logits)) + int(bool(return_scores)))
    if out is None:
        out = tuple(None if w is None else torch.empty(*w[0], dtype=w[1], device=dev) for w in want)
    else:
        out = tuple(out)
        if len(out) != len(want):
            raise ValueError(f"out must hold {len(want)} items")
        for o, w in zip(out, want):
            if (o is None) != (w is None) or (o is not None and (
                    tuple(o.shape) != w[0] or o.dtype != w[1] or not o.is_contiguous() or o.device != dev)):
                raise ValueError("out does not match this call's outputs (shape, dtype, contiguity or device)")
    ids, wts, sw = out[:3]
    logits = out[3] if return_logits else None
    scores = out[-1] if return_scores else None
    if dt != torch.float16:  # one entry for every E and rule (the fp16 call keeps the entries and kernels it had)
        nat.check(nat.symbol("mxmoe_moe_gate_dt")(
            _DT[dt], _ptr(hidden), _ptr(w_gate), _ptr(sg), T, H, E, topk, int(bool(renormalize)), GATE_SCORING[scoring],
            _ptr(e_bias), int(n_group), int(topk_group), group_top, float(routed_scaling_factor), _ptr(logit_bias), _ptr(ids),
            _ptr(wts), _ptr(sw), _ptr(logits), _ptr(scores), _stream(stream)))
    elif E > GATE_GROUPS_MAX_E or logit_bias is not None:
        fn = "mxmoe_moe_gate_wide" if E > GATE_GROUPS_MAX_E else "mxmoe_moe_gate_ex2"
        nat.check(nat.symbol(fn)(
            _ptr(hidden), _ptr(w_gate), _ptr(sg), T, H, E, topk, int(bool(renormalize)), GATE_SCORING[scoring], _ptr(e_bias),
            int(n_group), int(topk_group), group_top, float(routed_scaling_factor), _ptr(logit_bias), _ptr(ids), _ptr(wts),
            _ptr(sw), _ptr(logits), _ptr(scores), _stream(stream)))
    elif plain:
        nat.check(nat.lib().mxmoe_moe_gate(_ptr(hidden), _ptr(w_gate), _ptr(sg), T, H, E, topk, int(bool(renormalize)),
                                           _ptr(ids), _ptr(wts), _ptr(sw), _ptr(logits), _stream(stream)))
    else:
        nat.check(nat.lib().mxmoe_moe_gate_ex(_ptr(hidden), _ptr(w_gate), _ptr(sg), T, H, E, topk, int(bool(renormalize)),
                                              GATE_SCORING[scoring], _ptr(e_bias), int(n_group), int(topk_group), group_top,
                                              float(routed_scaling_factor), _ptr(ids), _ptr(wts), _ptr(sw), _ptr(logits),
                                              _ptr(scores), _stream(stream)))
    return out


def route_device(topk_ids: torch.Tensor, E: int, stream: Optional[torch.cuda.Stream] = None, out=None):
    """The routing launch alone (no host synchronisation): (sorted_expert, perm_token, inv_slot, counts)
    device int32 tensors; `out` reuses a previous result's buffers."""
    if topk_ids.dim() != 2 or topk_ids.dtype != torch.int32 or not topk_ids.is_contiguous():
        raise ValueError("topk_ids must be a contiguous int32 [T, topk] tensor")
    T, topk = topk_ids.shape
    dev = topk_ids.device
    n = T * topk
    if out is None:
        out = tuple(torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3)) + (
            torch.empty(E, dtype=torch.int32, device=dev),)
    nat.check(nat.lib().mxmoe_moe_route(_ptr(topk_ids), T, topk, E, *(_ptr(t) for t in out), _stream(stream)))
    return out


def route(topk_ids: torch.Tensor, E: int, stream: Optional[torch.cuda.Stream] = None) -> Routing:
    """Stable counting sort of the routing choices by expert (one HIP launch + the counts to host)."""
    if topk_ids.dim() != 2:
        raise ValueError("topk_ids must be [T, topk]")
    T, topk = topk_ids.shape
    n = T * topk
    sorted_e, perm, inv, counts = route_device(topk_ids.to(torch.int32).contiguous(), E, stream)
    c = counts.cpu().tolist()
    if sum(c) != n:
        raise ValueError(f"topk_ids holds {n - sum(c)} ids outside [0, {E})")
    return Routing(sorted_e, perm, inv, c, T, topk, E)


@dataclasses.dataclass
class ActBatch:
    """Permuted (and quantised) activations: one segment per expert (+ the shared expert)."""

    out: torch.Tensor     # uint8 store of every segment's rows
    scales: torch.Tensor  # fp16 store of every segment's scales
    segs: list            # nat.MoeSegC per segment (host)
    qtags: list[int]

    def A(self, e: int) -> torch.Tensor:
        """Segment e as the GroupGEMM A operand: fp16 [rows, width] or packed uint8 [rows, width*bits/8]."""
        s = self.segs[e]
        bits = _BITS[self.qtags[e]]
        nbytes = s.rows * s.width * bits // 8
        v = self.out[s.out_off:s.out_off + nbytes]
        if bits == 16:
            return v.view(torch.float16).view(max(s.rows, 0), s.width)
        return v.view(s.rows, s.width * bits // 8)

    def scale(self, e: int) -> Optional[torch.Tensor]:
        s = self.segs[e]
        tag = self.qtags[e]
        if tag == ACT_FP16:
            return None
        v = self.scales[s.scale_off:s.scale_off + s.rows * _scale_elems(tag, s.width)]
        if tag in _MX_TAGS:  # e8m0 bytes [rows, 16 G] inside the fp16 store
            return v.view(torch.uint8).view(s.rows, _mx_scale_row(s.width))
        return v


def _make_segments(rows: Sequence[int], first: Sequence[int], widths: Sequence[int], qtags: Sequence[int],
                   device) -> tuple[list, torch.Tensor, torch.Tensor, torch.Tensor]:
    segs, off, soff = [], 0, 0
    for r, f, w, tag in zip(rows, first, widths, qtags):
        if w % 128:
            raise ValueError(f"segment width {w} must be a multiple of 128")
        if tag in _MX_TAGS:
            soff += soff % 2  # its scale bytes are read as dwords: a 4-byte aligned block
        segs.append(nat.MoeSegC(tag, f, r, w, off, soff))
        off += (r * w * _BITS[tag] // 8 + 15) // 16 * 16  # 16-B aligned A operands
        soff += r * _scale_elems(tag, w)
    arr = (nat.MoeSegC * len(segs))(*segs)
    dev_segs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)
    out = torch.empty(max(off, 16), dtype=torch.uint8, device=device)
    scales = torch.empty(max(soff, 1), dtype=torch.float16, device=device)
    return segs, dev_segs, out, scales


# The activation pass's input layouts (mxmoe_moe_act_quant's mode numbers, include/mxmoe_moe.h) and the entry point
# each had before the tagged one: "gather" reads hidden rows through perm_token, the others the gate_up output in
# slot order — "plain" [gate | up] columns, "fused" the activations themselves (the GroupGEMM's SiLU epilogue ran),
# "interleaved" gate / up alternating in 16-column blocks.
_ACT_MODES = {"gather": 0, "plain": 1, "fused": 2, "interleaved": 3}
_LEGACY_ENTRY = {"gather": "mxmoe_moe_quant_act", "plain": "mxmoe_moe_silu_mul_quant", "fused": "mxmoe_moe_quant_slots",
                 "interleaved": "mxmoe_moe_silu_mul_quant_il"}
_MX_MASK = _tag_mask(_MX_TAGS)
_TAGGED_MASK = _MX_MASK | _tag_mask([ACT_E4M3])  # tags only the entries with a tag_mask carry (builds of their own)


def _act_entry(mode: str, has_mx_tag: bool, glu: bool) -> str:
    """The C entry point of an activation pass: a gate_up bias or another activation (``glu``) needs
    mxmoe_moe_glu_quant, which reads the plain layout only; any MX tag or the E4M3 tag (``has_mx_tag``) needs the
    tagged entry (the builds of the kernel that carry those tags); everything else keeps the mode's own entry, which a library loaded through
    MXMOE_GG_LIB that predates the tagged one still has."""
    if mode not in _ACT_MODES:
        raise ValueError(f"activation-pass mode must be one of {list(_ACT_MODES)}, got {mode!r}")
    if glu:
        if mode != "plain":
            raise ValueError(f"a layer with a bias or another activation needs the plain gate_up layout, got {mode!r}")
        return "mxmoe_moe_glu_quant"
    return "mxmoe_moe_act_quant" if has_mx_tag else _LEGACY_ENTRY[mode]


def _launch_act(mode: str, glu: Optional["nat.MoeGluC"], src: torch.Tensor, src_shared: Optional[torch.Tensor], T: int,
                topk: int, width: int, width_shared: int, sorted_expert: torch.Tensor, perm: Optional[torch.Tensor],
                dsegs: torch.Tensor, nseg: int, mask: int, out: torch.Tensor, scales: torch.Tensor,
                stream: Optional[torch.cuda.Stream]) -> None:
    """One activation pass on preallocated buffers: exactly one native call, nothing allocated or converted.
    src / src_shared: hidden (and hidden again for a shared expert) with ``perm`` in "gather" mode, else the
    gate_up outputs; dsegs / nseg: the device segment table; mask: ``_tag_mask`` of the segments' tags."""
    entry = _act_entry(mode, bool(mask & _TAGGED_MASK), glu is not None)
    if src.dtype != torch.float16:  # only the gather reads another element type (bf16 rows: mxmoe_moe_gather_quant)
        if mode != "gather" or src.dtype not in _DT:
            raise ValueError(f"the activation pass reads fp16 (the gather: fp16 or bf16 hidden states), got {src.dtype} "
                             f"in mode {mode!r}")
        entry = "mxmoe_moe_gather_quant"
    fn = nat.symbol(entry)  # (a library from before the entry refuses here)
    slots = (_ptr(src), _ptr(src_shared), T, topk, width, width_shared, _ptr(sorted_expert))
    segs = (_ptr(dsegs), nseg)
    stores = (_ptr(out), _ptr(scales), _stream(stream))
    if entry == "mxmoe_moe_gather_quant":
        st = fn(_DT[src.dtype], _ptr(src), T, width, topk, int(src_shared is not None), _ptr(sorted_expert), _ptr(perm), *segs,
                mask, *stores)
    elif entry == "mxmoe_moe_quant_act":
        st = fn(_ptr(src), T, width, topk, int(src_shared is not None), _ptr(sorted_expert), _ptr(perm), *segs, *stores)
    elif entry == "mxmoe_moe_act_quant":
        st = fn(_ACT_MODES[mode], *slots, _ptr(perm), *segs, mask, *stores)
    elif entry == "mxmoe_moe_glu_quant":
        st = fn(ctypes.byref(glu), *slots, *segs, mask, *stores)
    else:
        st = fn(*slots, *segs, *stores)
    nat.check(st)


def _segments_of(r: Routing, qtags: Sequence[int], width: int, width_shared: int, has_shared: bool, device):
    """``_make_segments`` for a routing: one segment per expert in slot order (rows = its count) and, with
    ``has_shared``, the shared expert's T rows behind them (len(qtags) == E, or E + 1 with the shared expert last)."""
    nseg = r.E + (1 if has_shared else 0)
    if len(qtags) != nseg:
        raise ValueError(f"need {nseg} quant tags, got {len(qtags)}")
    rows = list(r.counts) + ([r.T] if has_shared else [])
    first = r.first_slot + ([r.T * r.topk] if has_shared else [])
    widths = [width] * r.E + ([width_shared] if has_shared else [])
    return _make_segments(rows, first, widths, qtags, device)


def _act_pass(mode: str, glu, src: torch.Tensor, src_shared: Optional[torch.Tensor], r: Routing, qtags: Sequence[int],
              width: int, width_shared: int, stream: Optional[torch.cuda.Stream]) -> ActBatch:
    """Segments and stores for this routing, the pass launched once, and the launch kept as ``relaunch``."""
    segs, dsegs, out, scales = _segments_of(r, qtags, width, width_shared, src_shared is not None, src.device)
    mask = _tag_mask(qtags)
    perm = r.perm_token if mode == "gather" else None

    def launch(st=stream):
        _launch_act(mode, glu, src, src_shared, r.T, r.topk, width, width_shared, r.sorted_expert, perm, dsegs, len(segs),
                    mask, out, scales, st)

    launch()
    b = ActBatch(out, scales, segs, list(qtags))
    b.relaunch = launch  # same buffers, kernel only (timing / graph capture); keeps the inputs and dsegs alive
    return b


def quant_act(hidden: torch.Tensor, r: Routing, qtags: Sequence[int], with_shared: bool,
              stream: Optional[torch.cuda.Stream] = None) -> ActBatch:
    """Gather hidden rows into expert order and quantise each expert's rows by its tag
    (len(qtags) == E, or E + 1 with the shared expert last). hidden: fp16, or bf16 (mxmoe_moe_gather_quant): each
    element is then rounded to fp16 as it is loaded (to nearest even, +-Inf beyond fp16's range, fp16 subnormals kept)
    and the stores are byte for byte those of ``quant_act(hidden.to(torch.float16), ...)`` — the experts compute on
    fp16 values either way. Any other dtype raises."""
    if hidden.dim() != 2:
        raise ValueError("hidden must be [T, K]")
    _check_io_dtype(hidden.dtype, "hidden")
    K = hidden.shape[1]
    h = hidden.contiguous()
    return _act_pass("gather", None, h, h if with_shared else None, r, qtags, K, K, stream)


def silu_mul_quant(routed: torch.Tensor, shared: Optional[torch.Tensor], r: Routing, qtags: Sequence[int],
                   stream: Optional[torch.cuda.Stream] = None, activated: bool = False,
                   interleaved: bool = False) -> ActBatch:
    """act = silu(gate) * up of the gate_up outputs (routed [T*topk, 2N] in slot order, shared
    [T, 2Ns]), quantised per expert for the down GroupGEMM. ``activated``: the inputs already are
    the activations (routed [T*topk, N], shared [T, Ns]: the gate_up GroupGEMM's fused SiLU
    epilogue) and only the quantisation runs (mxmoe_moe_quant_slots). ``interleaved``: the gate_up
    output's gate / up columns alternate in 16-column blocks (the fused layout's weights through the
    plain epilogue; mxmoe_moe_silu_mul_quant_il)."""
    div = 1 if activated else 2
    Ns = shared.shape[1] // div if shared is not None else 0
    mode = "fused" if activated else "interleaved" if interleaved else "plain"
    return _act_pass(mode, None, routed, shared, r, qtags, routed.shape[1] // div, Ns, stream)


def _f32(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.to(torch.float32).contiguous()


def _launch_combine(out: torch.Tensor, y: torch.Tensor, inv_slot: torch.Tensor, sorted_expert: Optional[torch.Tensor],
                    weights: torch.Tensor, shared: Optional[torch.Tensor], shared_w: Optional[torch.Tensor], topk: int,
                    stream: Optional[torch.cuda.Stream] = None, down_bias: Optional[tuple] = None) -> None:
    """The combine on preallocated device buffers (no allocation, one launch: graph-capturable): out [T, H] fp16
    (or bf16: mxmoe_moe_combine_dt rounds the same f32 accumulator to bf16; every input stays fp16),
    y [R, H] fp16 rows, inv_slot int32 [T*topk] rows of y, weights f32 [T, topk], shared fp16 [T, H] and shared_w
    f32 [T] or None. ``down_bias`` = (E, bias, shared_bias): mxmoe_moe_combine_bias, with the down projection's
    bias (fp16 [E, H], the expert of a slot from sorted_expert; the shared expert's fp16 [H]; either may be None)
    added to each down output before its weight (``MoEFFN.down_bias``: which layers run that kernel)."""
    T, H = out.shape
    _check_io_dtype(out.dtype, "out")
    if down_bias is not None:
        E, bias, shared_bias = down_bias
        _check_bias(bias, (E, H), "bias", out.device)
        _check_bias(shared_bias, (H,), "shared_bias", out.device)
    if out.dtype != torch.float16:  # (a layer without a down bias: no bias pointers, mxmoe_moe_combine's arithmetic)
        E, bias, shared_bias = down_bias if down_bias is not None else (1, None, None)
        st = nat.symbol("mxmoe_moe_combine_dt")(_DT[out.dtype], _ptr(y), _ptr(inv_slot), _ptr(sorted_expert), _ptr(weights),
                                                _ptr(bias), _ptr(shared), _ptr(shared_w), _ptr(shared_bias), T, topk, E, H,
                                                _ptr(out), _stream(stream))
    elif down_bias is not None:
        st = nat.symbol("mxmoe_moe_combine_bias")(_ptr(y), _ptr(inv_slot), _ptr(sorted_expert), _ptr(weights), _ptr(bias),
                                                  _ptr(shared), _ptr(shared_w), _ptr(shared_bias), T, topk, E, H, _ptr(out),
                                                  _stream(stream))
    else:
        st = nat.lib().mxmoe_moe_combine(_ptr(y), _ptr(inv_slot), _ptr(weights), _ptr(shared), _ptr(shared_w), T, topk, H,
                                         _ptr(out), _stream(stream))
    nat.check(st)


def combine(y: torch.Tensor, r: Routing, weights: torch.Tensor, shared: Optional[torch.Tensor] = None,
            shared_w: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
            out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """out[t] = sum_k weights[t,k] * y[slot(t,k)] (+ shared_w[t] * shared[t]), f32 fma chain, fp16 out
    (``out_dtype=torch.bfloat16``: the same chain rounded to bf16)."""
    _check_io_dtype(out_dtype, "out_dtype")
    out = torch.empty(r.T, y.shape[1], dtype=out_dtype, device=y.device)
    _launch_combine(out, y, r.inv_slot, None, _f32(weights), shared, _f32(shared_w), r.topk, stream)
    return out


def combine_into(out: torch.Tensor, y: torch.Tensor, inv_slot: torch.Tensor, weights: torch.Tensor,
                 shared: Optional[torch.Tensor], topk: int, stream: Optional[torch.cuda.Stream] = None) -> None:
    """combine() on preallocated device buffers (``_launch_combine`` without shared_w). dist.CombineExchange's
    token-owner combine."""
    if out.shape[0] == 0:
        return
    _launch_combine(out, y, inv_slot, None, weights, shared, None, topk, stream)


@dataclasses.dataclass(frozen=True)
class SwigluClamp:
    """gpt-oss's gated activation (GptOssExperts._apply_gate; MXMOE_GLU_SWIGLU_CLAMP of include/mxmoe_moe.h):
    act = (clamp(up, -limit, limit) + 1) * g * sigmoid(alpha * g), g = min(gate, limit)."""

    alpha: float = 1.702
    limit: float = 7.0

    def __post_init__(self):
        if not math.isfinite(self.alpha) or not math.isfinite(self.limit) or not self.limit > 0:
            raise ValueError(f"SwigluClamp needs a finite alpha and a finite limit > 0, got {self.alpha}, {self.limit}")


def _check_activation(activation) -> None:
    if activation != "silu" and not isinstance(activation, SwigluClamp):
        raise ValueError(f"activation must be 'silu' or a SwigluClamp, got {activation!r}")


def _glu_struct(activation, bias_routed: Optional[torch.Tensor], bias_shared: Optional[torch.Tensor]) -> "nat.MoeGluC":
    clamp = isinstance(activation, SwigluClamp)
    return nat.MoeGluC(nat.GLU_SWIGLU_CLAMP if clamp else nat.GLU_SILU, activation.alpha if clamp else 0.0,
                       activation.limit if clamp else 0.0, None if bias_routed is None else bias_routed.data_ptr(),
                       None if bias_shared is None else bias_shared.data_ptr())


def _check_bias(b: Optional[torch.Tensor], shape: tuple, what: str, device) -> None:
    if b is not None and (b.dtype != torch.float16 or not b.is_contiguous() or tuple(b.shape) != shape or b.device != device):
        raise ValueError(f"{what} must be a contiguous fp16 {list(shape)} tensor on the activations' device")


def glu_quant(routed: torch.Tensor, shared: Optional[torch.Tensor], r: Routing, qtags: Sequence[int],
              activation="silu", bias_routed: Optional[torch.Tensor] = None, bias_shared: Optional[torch.Tensor] = None,
              stream: Optional[torch.cuda.Stream] = None) -> ActBatch:
    """``silu_mul_quant`` (plain [gate | up] inputs) for a gate_up projection with a bias and / or another gated
    activation (mxmoe_moe_glu_quant): the expert's bias row (bias_routed fp16 [E, 2N], bias_shared fp16 [2Ns], each
    [gate | up]) is added to the gate_up output as it is read, then ``activation`` ("silu" or a ``SwigluClamp``)
    and the quantisation by tag. With "silu" and no bias: silu_mul_quant's output byte for byte."""
    _check_activation(activation)
    N = routed.shape[1] // 2
    Ns = shared.shape[1] // 2 if shared is not None else 0
    _check_bias(bias_routed, (r.E, 2 * N), "bias_routed", routed.device)
    _check_bias(bias_shared, (2 * Ns,), "bias_shared", routed.device)
    if bias_shared is not None and shared is None:
        raise ValueError("bias_shared given without a shared input")
    b = _act_pass("plain", _glu_struct(activation, bias_routed, bias_shared), routed, shared, r, qtags, N, Ns, stream)
    b.biases = (bias_routed, bias_shared)  # the struct holds their addresses only: alive as long as relaunch is
    return b


def combine_bias_into(out: torch.Tensor, y: torch.Tensor, inv_slot: torch.Tensor, sorted_expert: torch.Tensor,
                      weights: torch.Tensor, bias: Optional[torch.Tensor], shared: Optional[torch.Tensor],
                      shared_w: Optional[torch.Tensor], shared_bias: Optional[torch.Tensor], topk: int, E: int,
                      stream: Optional[torch.cuda.Stream] = None) -> None:
    """mxmoe_moe_combine_bias on preallocated device buffers (``_launch_combine`` with a down bias)."""
    _launch_combine(out, y, inv_slot, sorted_expert, weights, shared, shared_w, topk, stream, (E, bias, shared_bias))


def combine_bias(y: torch.Tensor, r: Routing, weights: torch.Tensor, bias: Optional[torch.Tensor],
                 shared: Optional[torch.Tensor] = None, shared_w: Optional[torch.Tensor] = None,
                 shared_bias: Optional[torch.Tensor] = None, stream: Optional[torch.cuda.Stream] = None,
                 out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    """``combine`` for a down projection with a bias per expert: out[t] = sum_k weights[t,k] * (y[slot(t,k)] +
    bias[expert(t,k)]) (+ shared_w[t] * (shared[t] + shared_bias)), f32 fma chain, fp16 out (or ``out_dtype`` bf16)."""
    _check_io_dtype(out_dtype, "out_dtype")
    out = torch.empty(r.T, y.shape[1], dtype=out_dtype, device=y.device)
    combine_bias_into(out, y, r.inv_slot, r.sorted_expert, _f32(weights), bias, shared, _f32(shared_w), shared_bias, r.topk,
                      r.E, stream)
    return out


# ------------------------------------------------------------------ reference-named entry points

def _qtags(qparams_per_exp, n: int) -> list[int]:
    return [qtag_of(int(q[0]), int(q[2])) for q in list(qparams_per_exp)[:n]]


def _problem_lists(b: ActBatch, out_store: torch.Tensor, ld_of):
    """The reference's per-PROBLEM lists (non-empty segments in order): (inp_list, inp_scale_list, out_list), a
    segment's output its rows x ld_of(e) slice of out_store, packed one behind the other; no scale: an empty tensor."""
    inp_list, scale_list, out_list = [], [], []
    off = 0
    for e, s in enumerate(b.segs):
        if s.rows == 0:
            continue
        ld = ld_of(e)
        inp_list.append(b.A(e))
        sc = b.scale(e)
        scale_list.append(sc if sc is not None else torch.empty(0, dtype=torch.float16, device=out_store.device))
        out_list.append(out_store[off:off + s.rows * ld].view(s.rows, ld))
        off += s.rows * ld
    return inp_list, scale_list, out_list


def gg_permute_inp(hidden: torch.Tensor, topk_ids: torch.Tensor, E: int):
    """(num_problems, inp_buffer [T*topk, K] fp16 in expert order, indices, recv_tokens_per_exp)."""
    r = route(topk_ids, E)
    b = quant_act(hidden, r, [ACT_FP16] * E, with_shared=False)
    T, K = hidden.shape
    inp = b.out[: T * r.topk * K * 2].view(torch.float16).view(T * r.topk, K)
    counts = torch.tensor(r.counts, dtype=torch.int64)
    return sum(1 for c in r.counts if c), inp, r.perm_token.to(torch.int64), counts


def quant_inp_act(hidden: torch.Tensor, topk_ids: torch.Tensor, num_experts: int, N: int, num_shared_experts: int,
                  qparams_per_exp, verbose: bool = False):
    """Mirror of ref_bind.cu:434-592. qparams_per_exp[e] = (a_bits, w_bits, gsize, sym), the shared
    expert last. out_store / out_list: the gate_up output buffers (routed [T*topk, 2N] then
    shared [T, 2N * num_shared_experts])."""
    T = hidden.shape[0]
    has_shared = num_shared_experts > 0
    r = route(topk_ids, num_experts)
    tags = _qtags(qparams_per_exp, num_experts + (1 if has_shared else 0))
    b = quant_act(hidden, r, tags, has_shared)
    out_store = torch.empty((num_shared_experts + r.topk) * T * N * 2, dtype=torch.float16, device=hidden.device)
    lists = _problem_lists(b, out_store, lambda e: 2 * N * (num_shared_experts if e == num_experts else 1))
    if verbose:
        print([(e, s.rows, s.qtag) for e, s in enumerate(b.segs)])
    counts = torch.tensor(r.counts, dtype=torch.int64)
    return (*lists, b.out, b.scales, out_store, counts, r.perm_token.to(torch.int64), r.sorted_expert)


def silu_mul_then_quant(inp: torch.Tensor, num_problems: int, num_experts: int, K: int, N: int,
                        num_shared_experts: int, num_tokens: int, topk: int, values_sorted: torch.Tensor,
                        recv_tokens_per_exp: torch.Tensor, qparams_per_exp):
    """Mirror of ref_bind.cu:595-757: inp = the gate_up out_store (routed [T*topk, 2N] then shared
    [T, 2N*S]); returns the quantised down-proj inputs and the down output store [(1+topk)*T*K]."""
    T = num_tokens
    S = num_shared_experts
    routed = inp[: T * topk * 2 * N].view(T * topk, 2 * N)
    shared = inp[T * topk * 2 * N: T * topk * 2 * N + T * 2 * N * S].view(T, 2 * N * S) if S > 0 else None
    counts = [int(c) for c in recv_tokens_per_exp.tolist()]
    r = Routing(values_sorted.to(torch.int32), torch.empty(0), torch.empty(0), counts, T, topk, num_experts)
    tags = _qtags(qparams_per_exp, num_experts + (1 if S > 0 else 0))
    b = silu_mul_quant(routed, shared, r, tags)
    out_store = torch.empty((1 + topk) * T * K, dtype=torch.float16, device=inp.device)
    return (*_problem_lists(b, out_store, lambda e: K), b.out, b.scales, out_store)


_SHARE_FUSED_PLANS: dict = {}


def gg_mxmoe_share_fused(inp: Sequence[torch.Tensor], experts: Sequence[torch.Tensor],
                         scale_zp_a: Sequence[torch.Tensor], scale_zp_b: Sequence[torch.Tensor],
                         output: Sequence[torch.Tensor], N: int, K: int, shared_N: int, shared_K: int,
                         qparams_per_exp, recv_tokens_per_exp: torch.Tensor, verbose: bool = False,
                         stream: Optional[torch.cuda.Stream] = None):
    """Mirror of the reference's fused GroupGEMM op (ref_bind.cu:312-431, pybind name
    ``gg_mxmoe_share_fused``), with its argument meaning:

    * ``recv_tokens_per_exp`` int64 [E] (host or device): routed rows per expert; experts with 0
      rows have no problem. ``experts`` has E entries, or E + 1 with the shared expert last, whose
      problem has ``inp[-1].size(0)`` rows and shape (shared_N, shared_K); routed ones (N, K).
    * ``inp`` / ``scale_zp_a`` / ``output`` are per PROBLEM (non-empty experts in expert order, then
      the shared one), ``experts`` / ``scale_zp_b`` / ``qparams_per_exp`` per EXPERT;
      qparams_per_exp[e] = (a_bits, w_bits, gsize, sym).
    * Operands are in the GroupGEMM layout (the outputs of ``quant_inp_act`` /
      ``silu_mul_then_quant`` and ``prepare_weight``); an empty scale tensor means "no scale" (fp16).

    The reference hard-codes one fused w4a16 + w8a8 kernel (``mxmoe_w4a16_w8a8_bs256``, :412); here
    any supported mix runs on the AUTO variant. The plan (tile table) is cached per shape / qparams
    signature, so repeated calls with the same routing only re-point the operands. Returns ``output``.
    """
    counts = [int(c) for c in recv_tokens_per_exp.tolist()]
    E = len(counts)
    has_shared = len(experts) > E
    num_tokens = int(inp[-1].shape[0]) if len(inp) else 0
    probs = []
    pi = 0
    for e in range(E + (1 if has_shared else 0)):
        rows = num_tokens if e == E else counts[e]
        if rows == 0:
            continue
        if pi >= len(inp):
            raise ValueError(f"gg_mxmoe_share_fused: {len(inp)} inputs for more non-empty experts")
        a_bits, w_bits, gsize, sym = (int(x) for x in qparams_per_exp[e])
        # (4, 4, 32, 1) is w4a4_g32_sym_MXFP4 and (16, 4, 32, 1) w4a16_g32_sym_MXFP4: the only g32 types, so
        # the tuple needs no format field ((8, 4, 32, 1) is w4a8_g32_sym_MXFP8)
        q = QParams(a_bits, w_bits, gsize, bool(sym), "MXFP4" if (w_bits, gsize) == (4, 32) and a_bits in (4, 16) else
                    "MXFP8" if (a_bits, w_bits, gsize) == (8, 4, 32) else "")
        n, k = (shared_N, shared_K) if e == E else (N, K)

        def opt(t):
            return None if t is None or t.numel() == 0 else t

        C = output[pi]
        probs.append(Problem(A=inp[pi], B=experts[e], C=C, M=rows, N=n, K=k, q=q, scale_a=opt(scale_zp_a[pi]),
                             scale_b=opt(scale_zp_b[e]), ldc=int(C.stride(0)) if C.dim() == 2 else 0))
        if verbose:
            print(f"problem {pi}: [{rows},{n},{k}] qparams: [{a_bits} {w_bits}] {gsize} {int(bool(sym))}")
        pi += 1
    if pi != len(inp):
        raise ValueError(f"gg_mxmoe_share_fused: {len(inp)} inputs for {pi} non-empty experts")
    if not probs:
        return output
    s = stream if stream is not None else torch.cuda.current_stream(probs[0].C.device)
    # one plan per (device, stream, shapes, qparams, strides): a plan's workspace is only ever rebound
    # and launched on its own stream, so a rebind (blocking on that stream) never re-points the
    # operands of a launch still running on another one
    key = (probs[0].C.device, int(s.cuda_stream), tuple((p.M, p.N, p.K, p.q, p.lda, p.ldb, p.ldc) for p in probs))
    gg = _SHARE_FUSED_PLANS.get(key)
    if gg is not None:
        try:
            gg.rebind(probs, stream=s)
        except nat.GGError:  # the library's plan signature disagrees (e.g. a stride the key missed): re-plan
            _evict_share_fused(key)
            gg = None
    if gg is None:
        if len(_SHARE_FUSED_PLANS) >= 64:
            for k in list(_SHARE_FUSED_PLANS):
                _evict_share_fused(k)
        gg = GroupGemm(probs, stream=s)
        gg.stream = s
        if s != torch.cuda.current_stream(gg.device):  # allocated on the current stream, used on s
            gg.workspace.record_stream(s)
        _SHARE_FUSED_PLANS[key] = gg
    gg.launch(s)
    return output


def _evict_share_fused(key) -> None:
    """Drop a cached plan whose launches may still be running on its stream: record the workspace on
    that stream first, so the caching allocator does not hand the memory out before they finish."""
    gg = _SHARE_FUSED_PLANS.pop(key)
    gg.workspace.record_stream(gg.stream)


# ------------------------------------------------------------------ the MoE FFN layer

@dataclasses.dataclass
class ExpertWeights:
    """One linear's GroupGEMM B operand: fp16 [N, K] or packed codes + scale_b, and its QParams."""

    B: torch.Tensor
    scale_b: Optional[torch.Tensor]
    q: QParams
    N: int
    K: int
    scale_out_of_range: int = 0  # prepare_weight_mx: scale bytes outside [104, 140] (include/mxmoe_gg.h);
    #                              prepare_weight_e4m3: f32 scales that fp16 changed or that left its normal range


def prepare_weight(w: torch.Tensor, q: QParams, interleave: bool = False) -> ExpertWeights:
    """fp16 [N, K] -> the GroupGEMM's B operand for qcfg q (setup, once per weight). interleave: a
    gate_up weight ([gate; up] rows) reordered for the fused SiLU epilogue (interleave_gate_up; the
    per-row scales follow their rows)."""
    from .groupgemm import interleave_gate_up
    from .quantize import (pack_e4m3, pack_mxfp4_scales, pack_weightonly_mi355x, pack_wxax, quant_e4m3, quant_mxfp4,
                           quant_rtn_sym, quant_weightonly)

    N, K = w.shape
    if interleave:
        w = interleave_gate_up(w)[0]  # (per-row quantisation commutes with the row order)
    if not q.is_quant:
        return ExpertWeights(w.contiguous(), None, q, N, K)
    if q.fmt in ("MXFP4", "MXFP8"):  # w4a4, w4a16 and w4a8 alike: canonical codes + device-layout scales, no repack
        codes, sc = quant_mxfp4(w)
        return ExpertWeights(codes, pack_mxfp4_scales(sc), q, N, K)
    if q.is_weight_only:
        codes, sz = quant_weightonly(w, q.w_bits, q.gsize, q.sym)
        return ExpertWeights(pack_weightonly_mi355x(codes, q.w_bits), sz, q, N, K)
    if q.is_fp8:  # w8a8_g-1_sym_E4M3: e4m3 codes in pack_wxax's 8-bit order, one fp16 scale per output row
        codes, sc = quant_e4m3(w)
        return ExpertWeights(pack_e4m3(codes), sc, q, N, K)
    qw, sw = quant_rtn_sym(w, q.w_bits, q.gsize)
    return ExpertWeights(pack_wxax(qw, q.w_bits), sw, q, N, K)


MX_QCFGS = ("w4a4_g32_sym_MXFP4", "w4a16_g32_sym_MXFP4", "w4a8_g32_sym_MXFP8")
MX_EXACT_SCALE_RANGE = (104, 140)  # scale bytes for which every dequantised weight is an exact fp16 (include/mxmoe_gg.h)


def prepare_weight_mx(codes: torch.Tensor, scales: torch.Tensor, q: QParams, warn: bool = True) -> ExpertWeights:
    """Weights that already are MXFP4 (a checkpoint's ``blocks`` / ``scales``) -> the GroupGEMM's B operand for any of
    the three MX qcfgs, with no requantisation: codes uint8 [N, K/2] (low nibble = element 2i, e2m1) are used as they
    are (no copy when contiguous: the three qcfgs' operands share the tensor), scales uint8 [N, K/32] (e8m0) are put
    into the device layout (``pack_mxfp4_scales``). ``scale_out_of_range`` of the result counts the scale bytes
    outside [104, 140], the range in which the weight-only type's fp16 dequantisation is exact (outside it the
    result is recorded, not specified: include/mxmoe_gg.h); a non-zero count warns unless ``warn`` is False."""
    from .quantize import MXFP4_BLOCK, pack_mxfp4_scales

    if q.qcfg not in MX_QCFGS:
        raise ValueError(f"prepare_weight_mx: qcfg must be one of {MX_QCFGS}, got {q.qcfg}")
    if codes.dtype != torch.uint8 or scales.dtype != torch.uint8 or codes.dim() != 2 or scales.dim() != 2:
        raise ValueError("prepare_weight_mx: codes uint8 [N, K/2] and scales uint8 [N, K/32]")
    N, K = codes.shape[0], 2 * codes.shape[1]
    if K % MXFP4_BLOCK or tuple(scales.shape) != (N, K // MXFP4_BLOCK):
        raise ValueError(f"prepare_weight_mx: K = {K} must be a multiple of 32 and scales [{N}, K/32], got "
                         f"{tuple(scales.shape)}")
    lo, hi = MX_EXACT_SCALE_RANGE
    bad = int(((scales < lo) | (scales > hi)).sum())
    if bad and warn:
        import warnings

        warnings.warn(f"prepare_weight_mx: {bad} of {scales.numel()} scale bytes lie outside [{lo}, {hi}]: with fp16 "
                      "activations their blocks' weights are not exact fp16 values (include/mxmoe_gg.h)", stacklevel=2)
    return ExpertWeights(codes.contiguous(), pack_mxfp4_scales(scales), q, N, K, bad)


def prepare_weight_e4m3(codes: torch.Tensor, scales: torch.Tensor, warn: bool = True) -> ExpertWeights:
    """Weights that already are per-channel FP8 (a checkpoint's ``weight`` / ``weight_scale``) -> the GroupGEMM's B
    operand for w8a8_g-1_sym_E4M3, with no requantisation: codes ``float8_e4m3fn`` or uint8 [N, K] (OCP e4m3 bit
    patterns, logical K order; K even) are put into pack_wxax's 8-bit byte order (``pack_e4m3``), scales [N] (or
    [N, 1]; fp16 or f32, one per output row) are kept as fp16. The kernel multiplies by fp16 scales: an f32 scale is
    rounded to nearest even, and ``scale_out_of_range`` of the result counts the scales whose value that changed or
    that are not normal fp16 numbers (zero, subnormal, beyond 65504 or not finite — a weight row scaled by one of
    those no longer is the checkpoint's); a non-zero count warns unless ``warn`` is False."""
    from .groupgemm import W8A8_E4M3
    from .quantize import pack_e4m3

    if codes.dtype == torch.float8_e4m3fn:
        codes = codes.view(torch.uint8)
    if codes.dtype != torch.uint8 or codes.dim() != 2 or codes.shape[1] % 2:
        raise ValueError("prepare_weight_e4m3: codes float8_e4m3fn or uint8 [N, K], K even")
    N, K = codes.shape
    if scales.dim() == 2 and scales.shape[1] == 1:
        scales = scales[:, 0]
    if scales.dtype not in (torch.float16, torch.float32) or tuple(scales.shape) != (N,):
        raise ValueError(f"prepare_weight_e4m3: scales fp16 or f32 [{N}] (one per output row), got {scales.dtype} "
                         f"{tuple(scales.shape)}")
    sc = scales.to(torch.float16)
    a = sc.float().abs()
    bad = int(((sc.float() != scales.float()) | ~torch.isfinite(sc) | (a < 2.0 ** -14)).sum())
    if bad and warn:
        import warnings

        warnings.warn(f"prepare_weight_e4m3: {bad} of {N} scales change value as fp16 or are no normal fp16 numbers: "
                      "their rows are not the checkpoint's weights (include/mxmoe_gg.h: fp16 scale_b)", stacklevel=2)
    return ExpertWeights(pack_e4m3(codes.contiguous()), sc.contiguous(), W8A8_E4M3, N, K, bad)


def pad_cols(t: torch.Tensor, width: int) -> torch.Tensor:
    """``t`` [..., C] zero-padded along its last dimension to ``width`` columns (hidden states and w_gate of a layer
    whose widths ``gptoss_layer`` padded; slice the layer's output back with ``out[:, :C]``)."""
    C = t.shape[-1]
    if C > width:
        raise ValueError(f"pad_cols: {C} columns do not fit {width}")
    if C == width:
        return t.contiguous()
    out = torch.zeros(*t.shape[:-1], width, dtype=t.dtype, device=t.device)
    out[..., :C] = t
    return out


def _stack_bias(bias, n: int, width: int, shared_width: int, what: str):
    """Per-expert bias rows (a sequence of n [width] tensors, the shared expert's [shared_width] last if the layer
    has one, or a stacked [n, width] tensor) -> (fp16 [E, width] of the routed experts, fp16 [shared_width] or None)."""
    if bias is None:
        return None, None
    rows = list(bias)
    if len(rows) != n:
        raise ValueError(f"{what}: need one row per expert ({n}), got {len(rows)}")
    E = n - (1 if shared_width else 0)
    for i, b in enumerate(rows):
        w = shared_width if i == E and shared_width else width
        if b.dim() != 1 or b.shape[0] != w:
            raise ValueError(f"{what}[{i}] must hold {w} elements, got {tuple(b.shape)}")
    routed = torch.stack([b.to(torch.float16) for b in rows[:E]]).contiguous()
    shared = rows[E].to(torch.float16).contiguous() if shared_width else None
    for t in (routed, shared):
        if t is not None and not torch.isfinite(t).all():
            raise ValueError(f"{what} must be finite as fp16")
    return routed, shared


def _problems(a: ActBatch, ws: Sequence[ExpertWeights], C_of, silu: bool = False) -> list[Problem]:
    """The GroupGEMM problems of an activation batch on the experts' weights ``ws``: one per non-empty segment, its
    output C_of(e, segment); silu: the SiLU epilogue (fused-layout gate_up weights)."""
    return [Problem(A=a.A(e), B=w.B, C=C_of(e, sg), M=sg.rows, N=w.N, K=w.K, q=w.q, scale_a=a.scale(e),
                    scale_b=w.scale_b, silu=silu) for e, (sg, w) in enumerate(zip(a.segs, ws)) if sg.rows]


class MoEFFN:
    """A quantised MoE FFN layer (routed experts + optional shared expert) on the fused GroupGEMM.

    gate_up[e]: fp16 [2N, H] (gate rows then up rows), down[e]: fp16 [H, N]; qcfg[e] = (QParams of
    gate_up, QParams of down) — the activation side (a_bits, gsize) of each QParams sets how the
    plumbing quantises that expert's input (qtag_of). Expert E (if given) is the shared expert.

    hidden may be fp16 or bf16, and ``out`` has its dtype. A bf16 layer has no cast pass: the gather rounds each
    hidden element to fp16 as it loads it (``quant_act``) and the combine rounds its f32 sums to bf16. The experts
    themselves compute on fp16 values (a hidden value beyond fp16's range is +-Inf to them), h1 / y / the biases
    stay fp16, and y is bit for bit the fp16 layer's on ``hidden.to(torch.float16)``."""

    # gate_up qcfgs with the SiLU epilogue: fp16 / w8a8 / w4a4 on every product kernel, weight-only
    # on the small-batch kernel (wo3; a large call of those falls back to the interleaved form).
    # w8a8_g-1_sym_E4M3 is not among them (its tile has no SiLU epilogue): a layer with an E4M3 gate_up is plain
    FUSE_QCFGS = ("fp16", "w8a8_g-1_sym", "w4a4_g-1_sym", "w4a8_g32_sym_MXFP8")
    FUSE_WEIGHT_ONLY = True

    def __init__(self, gate_up: Sequence[torch.Tensor], down: Sequence[torch.Tensor],
                 qcfg: Sequence[tuple[QParams, QParams]], num_routed: int, fuse_silu: Optional[bool] = None,
                 gate_up_bias=None, down_bias=None, activation="silu"):
        """gate_up / down may also be ``ExpertWeights`` (``prepare_weight_mx``: weights that already are MXFP4), used
        as they are (plain layout: no fuse_silu).

        gate_up_bias[e]: [2N] in [gate; up] order, down_bias[e]: [H] (one row per expert, the shared one last; kept as
        fp16, which must leave them finite); activation: "silu" or ``SwigluClamp`` (gpt-oss). The gate_up bias is added
        where the activation pass reads the gate_up output (mxmoe_moe_glu_quant), the down bias where the combine
        reads the down output (mxmoe_moe_combine_bias): no GroupGEMM kernel knows about either, so a layer with a
        bias or another activation runs the plain gate_up layout — fuse_silu defaults to False and True raises.

        fuse_silu: the gate_up GroupGEMM writes act = silu(gate) * up straight from its epilogue
        (MXMOE_GG_EPI_SILU_MUL; gate_up weights stored with gate / up rows interleaved in 16-row
        blocks) and only the quantisation runs after it — bit-identical outputs, half the gate_up C
        bytes and no separate SiLU pass (qwen2_moe layer step -6 %). Needs every gate_up qcfg in
        FUSE_QCFGS. None (default): fuse whenever the qcfgs allow. A call whose kernel has no SiLU
        epilogue (lab kernels; ``gate_up_mode = "interleaved"`` forces it) runs the plain epilogue on
        the interleaved weights and the interleaved-input SiLU pass instead — same outputs. (Before
        round 6 that was every small-batch call: the wo3 kernel's fp16 / w8a8 / w4a4 bodies now carry
        the epilogue too.)"""
        def dims(w):
            return (w.N, w.K) if isinstance(w, ExpertWeights) else tuple(w.shape)

        prepared = any(isinstance(w, ExpertWeights) for w in list(gate_up) + list(down))
        self.E = num_routed
        self.has_shared = len(gate_up) == num_routed + 1
        self.H = dims(gate_up[0])[1]
        self.N = dims(gate_up[0])[0] // 2
        self.Ns = dims(gate_up[-1])[0] // 2 if self.has_shared else 0
        self.qcfg = list(qcfg)
        _check_activation(activation)
        self.activation = activation
        self.b1, self.b1s = _stack_bias(gate_up_bias, len(gate_up), 2 * self.N, 2 * self.Ns, "gate_up_bias")
        self.b2, self.b2s = _stack_bias(down_bias, len(gate_up), self.H, self.H if self.has_shared else 0, "down_bias")
        eligible = all(q[0].qcfg in self.FUSE_QCFGS or (self.FUSE_WEIGHT_ONLY and q[0].is_weight_only) for q in qcfg)
        if fuse_silu and not eligible:
            raise ValueError(f"fuse_silu needs every gate_up qcfg in {self.FUSE_QCFGS} or weight-only")
        if fuse_silu and (self.biased_or_gated or prepared):
            raise ValueError("fuse_silu: a layer with a bias, an activation other than 'silu' or prepared weights runs "
                             "the plain gate_up layout (the SiLU epilogue knows neither)")
        self.fuse_silu = (eligible and not self.biased_or_gated and not prepared) if fuse_silu is None else fuse_silu

        def prep(w, q, interleave=False):
            if isinstance(w, ExpertWeights):
                if w.q != q:
                    raise ValueError(f"prepared weights carry qcfg {w.q.qcfg}, the layer's says {q.qcfg}")
                return w
            return prepare_weight(w, q, interleave=interleave)

        self.w1 = [prep(w, q[0], self.fuse_silu) for w, q in zip(gate_up, qcfg)]
        self.w2 = [prep(w, q[1]) for w, q in zip(down, qcfg)]
        self.tag1 = [qtag_of(q[0].a_bits, q[0].gsize, q[0].fmt) for q in qcfg]
        self.tag2 = [qtag_of(q[1].a_bits, q[1].gsize, q[1].fmt) for q in qcfg]
        self.gate_up_mode: Optional[str] = None  # None: the library decides; "interleaved": A/B override

    @property
    def biased_or_gated(self) -> bool:
        """The layer has a gate_up or down bias or an activation other than SiLU: its activation pass and combine
        are mxmoe_moe_glu_quant and mxmoe_moe_combine_bias (otherwise exactly the calls of a layer without)."""
        return (self.activation != "silu" or self.b1 is not None or self.b1s is not None or self.b2 is not None or
                self.b2s is not None)

    def act_quant(self, h1: torch.Tensor, h1s: Optional[torch.Tensor], r: Routing, mode: str) -> ActBatch:
        """The activation pass behind the gate_up GroupGEMM for its output layout ``mode`` (``gate_up_call``)."""
        if self.biased_or_gated:
            if mode != "plain":
                raise ValueError(f"a layer with a bias or another activation needs the plain gate_up layout, got {mode!r}")
            return glu_quant(h1, h1s, r, self.tag2, self.activation, self.b1, self.b1s)
        return silu_mul_quant(h1, h1s, r, self.tag2, activated=mode == "fused", interleaved=mode == "interleaved")

    @property
    def down_bias(self) -> Optional[tuple]:
        """``_launch_combine``'s down_bias of this layer: the bias kernel exactly when the layer is
        ``biased_or_gated`` (then also with no down bias at all), the plain combine (None) otherwise."""
        return (self.E, self.b2, self.b2s) if self.biased_or_gated else None

    def _view(self, q: QParams, tag: int, fuse_silu: bool) -> "MoEFFN":
        """This layer with every qcfg replaced by ``q`` (activation tag ``tag``) on the SAME weight tensors: the
        shapes, the biases and the activation carry over, the A/B override does not."""
        v = object.__new__(MoEFFN)
        for name in ("E", "has_shared", "H", "N", "Ns", "activation", "b1", "b1s", "b2", "b2s"):
            setattr(v, name, getattr(self, name))
        v.qcfg = [(q, q) for _ in self.qcfg]
        v.fuse_silu = fuse_silu
        v.w1 = [dataclasses.replace(w, q=q) for w in self.w1]
        v.w2 = [dataclasses.replace(w, q=q) for w in self.w2]
        v.tag1 = [tag] * len(self.qcfg)
        v.tag2 = [tag] * len(self.qcfg)
        v.gate_up_mode = None
        return v

    def a16_view(self) -> "MoEFFN":
        """This layer (every qcfg w4a4_g32_sym_MXFP4) with fp16 activations: a layer whose qcfgs are
        w4a16_g32_sym_MXFP4 on the SAME weight tensors — the two types share the B codes and scales
        byte for byte, so nothing is requantised or copied. Plain gate_up layout (no SiLU epilogue),
        as the w4a4 layer's. The form for decode-size batches (the small-batch kernel) and where
        4-bit activations cost accuracy."""
        from .groupgemm import W4A16_MXFP4

        if any(q.qcfg != "w4a4_g32_sym_MXFP4" for pair in self.qcfg for q in pair):
            raise ValueError("a16_view needs every qcfg of the layer to be w4a4_g32_sym_MXFP4")
        return self._view(W4A16_MXFP4, ACT_FP16, False)

    def a8_view(self) -> "MoEFFN":
        """This layer (every qcfg w4a4_g32_sym_MXFP4, or every one w4a16_g32_sym_MXFP4) with MXFP8
        activations: a layer whose qcfgs are w4a8_g32_sym_MXFP8 on the SAME weight tensors — the three MX
        types share the B codes and scales byte for byte. The gate_up layout (plain or interleaved for the
        SiLU epilogue) stays the source layer's, and with it whether the epilogue is fused."""
        from .groupgemm import W4A8_MXFP8

        names = {q.qcfg for pair in self.qcfg for q in pair}
        if names not in ({"w4a4_g32_sym_MXFP4"}, {"w4a16_g32_sym_MXFP4"}):
            raise ValueError("a8_view needs every qcfg of the layer to be w4a4_g32_sym_MXFP4, or every one "
                             "w4a16_g32_sym_MXFP4")
        return self._view(W4A8_MXFP8, ACT_MXFP8, self.fuse_silu)

    def gate_up_layout(self) -> str:
        """The gate_up output layout the layer asks for: "plain", or for fused-layout weights "fused" (where the
        call's kernel has the SiLU epilogue: ``gate_up_call``, ``GraphForward``) or, forced, "interleaved"."""
        if self.gate_up_mode not in (None, "interleaved"):
            raise ValueError(f"gate_up_mode must be None or 'interleaved', got {self.gate_up_mode!r}")
        return "plain" if not self.fuse_silu else "interleaved" if self.gate_up_mode == "interleaved" else "fused"

    def _planned(self, a: ActBatch, ws: Sequence[ExpertWeights], T: int, topk: int, width: int, width_shared: int,
                 silu: bool, dev):
        """A GroupGEMM over the non-empty segments of ``a`` and its fresh outputs: (GroupGemm, routed
        [T*topk, width] in slot order, shared [T, width_shared] or None)."""
        y = torch.empty(T * topk, width, dtype=torch.float16, device=dev)
        ys = torch.empty(T, width_shared, dtype=torch.float16, device=dev) if self.has_shared else None
        ps = _problems(a, ws, lambda e, sg: ys if e == self.E else y[sg.first_slot:sg.first_slot + sg.rows], silu)
        return GroupGemm(ps, device=dev), y, ys

    def gate_up_call(self, a1: ActBatch, T: int, topk: int, dev):
        """The planned gate_up GroupGEMM of one call and its output buffers: (GroupGemm, h1, h1s, mode),
        mode "plain" ([gate | up] columns), "fused" (the SiLU epilogue: N-wide activations) or
        "interleaved" (fused-layout weights through the plain epilogue and the interleaved-input SiLU
        pass, for calls whose kernel has no SiLU epilogue). The library decides: the variant AUTO
        resolves the call's shapes to is asked for MXMOE_GG_CAP_SILU_MUL (mxmoe_gg_variant_caps), and
        a fused plan the library still refuses (GGError UNSUPPORTED) falls back to "interleaved"."""
        mode = self.gate_up_layout()
        if mode == "fused":
            ph = torch.empty(0, dtype=torch.float16, device=dev)
            probe = _problems(a1, self.w1, lambda e, sg: ph)  # shapes only: AUTO's choice for the plain epilogue
            arr = (nat.GGProblemC * max(len(probe), 1))(*[p.to_c() for p in probe])
            v = nat.resolve_variant(arr, len(probe))
            mode = "fused" if nat.variant_caps(v) & nat.CAP_SILU_MUL else "interleaved"
        if mode == "fused":
            try:
                return *self._planned(a1, self.w1, T, topk, self.N, self.Ns, True, dev), mode
            except nat.GGError as e:
                if e.status != nat.MXMOE_GG_ERR_UNSUPPORTED:
                    raise
                mode = "interleaved"
        return *self._planned(a1, self.w1, T, topk, 2 * self.N, 2 * self.Ns, False, dev), mode

    def down_call(self, a2: ActBatch, T: int, topk: int, dev):
        """The planned down GroupGEMM of one call and its output buffers: (GroupGemm, y, ys)."""
        return self._planned(a2, self.w2, T, topk, self.H, self.H, False, dev)

    def forward(self, hidden: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor,
                shared_w: Optional[torch.Tensor] = None, return_intermediates: bool = False):
        T = hidden.shape[0]
        dev = hidden.device
        r = route(topk_ids, self.E)
        topk = r.topk
        a1 = quant_act(hidden, r, self.tag1, self.has_shared)
        g1, h1, h1s, mode = self.gate_up_call(a1, T, topk, dev)
        g1.launch()
        a2 = self.act_quant(h1, h1s, r, mode)
        g2, y, ys = self.down_call(a2, T, topk, dev)
        g2.launch()
        out = torch.empty(T, self.H, dtype=hidden.dtype, device=dev)
        _launch_combine(out, y, r.inv_slot, r.sorted_expert, _f32(topk_weights), ys, _f32(shared_w), topk, None,
                        self.down_bias)
        if return_intermediates:
            return out, dict(routing=r, a1=a1, h1=h1, h1s=h1s, a2=a2, y=y, ys=ys)
        return out


def gptoss_layer(blocks_gate_up: torch.Tensor, scales_gate_up: torch.Tensor, bias_gate_up: torch.Tensor,
                 blocks_down: torch.Tensor, scales_down: torch.Tensor, bias_down: torch.Tensor, *, act_bits: int = 16,
                 pad_to: int = 128, alpha: float = 1.702, limit: float = 7.0) -> MoEFFN:
    """A gpt-oss MoE layer's experts from the checkpoint's tensors, with no requantisation: ``*_blocks`` uint8
    [E, rows, K/32, 16] (16 bytes = 32 e2m1 codes, low nibble first: the canonical format of include/mxmoe_gg.h),
    ``*_scales`` uint8 [E, rows, K/32] (e8m0), biases [E, rows]; gate_up has rows = 2N with gate / up interleaved
    (rows 0::2 / 1::2) and K = H, down has rows = H and K = N.

    The rows are de-interleaved into [gate; up] (codes, scales and bias alike) and N and H are zero-padded up to
    multiples of ``pad_to`` (the plumbing needs widths that are multiples of 128: 2880 -> 2944): padded codes 0,
    padded scale bytes 127 (2^0), padded biases 0. The padding is neutral — a padded intermediate column has
    g = u = 0 and act = (0 + 1) * 0 * sigmoid(0) = 0, a padded output column is exactly 0 — so the caller feeds
    ``pad_cols(hidden, layer.H)`` (and ``pad_cols(w_gate, layer.H)`` to the router) and slices the output.
    act_bits: 16 (w4a16_g32_sym_MXFP4), 8 (w4a8_g32_sym_MXFP8) or 4 (w4a4_g32_sym_MXFP4); ``a16_view`` / ``a8_view``
    give the others on the same tensors. ``scale_out_of_range`` of the layer: the checkpoint's scale bytes outside
    [104, 140] (``prepare_weight_mx``; one warning for the layer).

    bf16 hidden states: the layer takes them as every ``MoEFFN`` does (bf16 in, bf16 out, a bf16 ``w_gate`` in its
    ``MoEBlock``); nothing here changes for them, and the biases stay fp16."""
    from .groupgemm import W4A4_MXFP4, W4A8_MXFP8, W4A16_MXFP4

    if act_bits not in (16, 8, 4):
        raise ValueError(f"act_bits must be 16, 8 or 4, got {act_bits}")
    q = {16: W4A16_MXFP4, 8: W4A8_MXFP8, 4: W4A4_MXFP4}[act_bits]
    if pad_to < 128 or pad_to % 128:
        raise ValueError(f"pad_to must be a positive multiple of 128, got {pad_to}")
    for name, blk, sc, bias in (("gate_up", blocks_gate_up, scales_gate_up, bias_gate_up),
                                ("down", blocks_down, scales_down, bias_down)):
        if blk.dtype != torch.uint8 or sc.dtype != torch.uint8 or blk.dim() != 4 or blk.shape[3] != 16 or \
                tuple(sc.shape) != tuple(blk.shape[:3]) or tuple(bias.shape) != tuple(blk.shape[:2]):
            raise ValueError(f"{name}: need blocks uint8 [E, rows, K/32, 16], scales uint8 [E, rows, K/32], bias [E, rows]")
    E, N2, H = blocks_gate_up.shape[0], blocks_gate_up.shape[1], 32 * blocks_gate_up.shape[2]
    N = N2 // 2
    if N2 % 2 or tuple(blocks_down.shape[:3]) != (E, H, N // 32) or N % 32:
        raise ValueError(f"down blocks must be [E = {E}, H = {H}, N / 32 = {N // 32}, 16] for gate_up's 2N = {N2} rows")
    up = lambda v: (v + pad_to - 1) // pad_to * pad_to
    Hp, Np = up(H), up(N)

    def padded(blk, sc, rows, rows_p, K, Kp):
        """one expert's [rows, K] weight -> canonical codes [rows_p, Kp / 2] and scales [rows_p, Kp / 32]"""
        codes = torch.zeros(rows_p, Kp // 2, dtype=torch.uint8, device=blk.device)
        scales = torch.full((rows_p, Kp // 32), 127, dtype=torch.uint8, device=blk.device)
        codes[:rows, :K // 2] = blk.reshape(rows, K // 2)
        scales[:rows, :K // 32] = sc
        return codes, scales

    w1, w2, b1, b2 = [], [], [], []
    for e in range(E):
        parts = [padded(blocks_gate_up[e, h::2], scales_gate_up[e, h::2], N, Np, H, Hp) for h in (0, 1)]  # gate, up
        w1.append(prepare_weight_mx(torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts]), q, warn=False))
        w2.append(prepare_weight_mx(*padded(blocks_down[e], scales_down[e], H, Hp, N, Np), q, warn=False))
        bgu = torch.zeros(2 * Np, dtype=torch.float16, device=bias_gate_up.device)
        bgu[:N] = bias_gate_up[e, 0::2].to(torch.float16)
        bgu[Np:Np + N] = bias_gate_up[e, 1::2].to(torch.float16)
        b1.append(bgu)
        b2.append(pad_cols(bias_down[e].to(torch.float16), Hp))
    layer = MoEFFN(w1, w2, [(q, q)] * E, num_routed=E, gate_up_bias=b1, down_bias=b2,
                   activation=SwigluClamp(alpha, limit))
    layer.scale_out_of_range = sum(w.scale_out_of_range for w in w1 + w2)
    if layer.scale_out_of_range:
        import warnings

        lo, hi = MX_EXACT_SCALE_RANGE
        warnings.warn(f"gptoss_layer: {layer.scale_out_of_range} scale bytes lie outside [{lo}, {hi}]: with fp16 activations "
                      "their blocks' weights are not exact fp16 values (include/mxmoe_gg.h)", stacklevel=2)
    return layer


class MoEBlock:
    """A MoE layer from hidden states: the router (``gate``) in front of a ``MoEFFN``.

    w_gate: fp16 or bf16 [E, H] (w_shared_gate of the same dtype; ``forward`` takes hidden of that dtype and
    returns it); topk / renormalize: the model's routing (qwen2_moe: 4, DeepSeek-V2-Lite: 6,
    both without renormalisation; Mixtral: 2 with); w_shared_gate: fp16 [H], qwen2_moe's
    shared_expert_gate (only for a layer with a shared expert); scoring, e_bias, n_group, topk_group,
    group_top, routed_scaling_factor: ``gate``'s (DeepSeek-V3 / V2, GLM-4.5); logit_bias: f32 [E], ``gate``'s
    (gpt-oss: with renormalize=True)."""

    def __init__(self, ffn: MoEFFN, w_gate: torch.Tensor, topk: int, renormalize: bool = False,
                 w_shared_gate: Optional[torch.Tensor] = None, scoring: str = "softmax",
                 e_bias: Optional[torch.Tensor] = None, n_group: int = 1, topk_group: int = 1,
                 group_top: Optional[int] = None, routed_scaling_factor: float = 1.0,
                 logit_bias: Optional[torch.Tensor] = None):
        if tuple(w_gate.shape) != (ffn.E, ffn.H):
            raise ValueError(f"w_gate must be [{ffn.E}, {ffn.H}], got {tuple(w_gate.shape)}")
        if w_shared_gate is not None and not ffn.has_shared:
            raise ValueError("w_shared_gate given for a layer without a shared expert")
        if w_shared_gate is not None and w_shared_gate.numel() != ffn.H:
            raise ValueError(f"w_shared_gate must hold {ffn.H} elements")
        _check_io_dtype(w_gate.dtype, "w_gate")
        if w_shared_gate is not None and w_shared_gate.dtype != w_gate.dtype:
            raise ValueError(f"w_shared_gate must have w_gate's dtype ({w_gate.dtype}), got {w_shared_gate.dtype}")
        gate_routing_args(ffn.E, topk, scoring, e_bias, n_group, topk_group, group_top, routed_scaling_factor)
        _check_logit_bias(logit_bias, ffn.E)
        self.ffn, self.topk, self.renormalize = ffn, topk, renormalize
        self.routing = dict(scoring=scoring, e_bias=None if e_bias is None else e_bias.contiguous(), n_group=n_group,
                            topk_group=topk_group, group_top=group_top, routed_scaling_factor=routed_scaling_factor)
        if logit_bias is not None:  # (a key of its own only when given: the routing of every other block is unchanged)
            self.routing["logit_bias"] = logit_bias
        self.w_gate = w_gate.contiguous()
        self.w_shared_gate = None if w_shared_gate is None else w_shared_gate.contiguous()

    def forward(self, hidden: torch.Tensor, return_intermediates: bool = False):
        if hidden.dtype != self.w_gate.dtype:
            raise ValueError(f"hidden must have the router's dtype ({self.w_gate.dtype}), got {hidden.dtype}")
        ids, wts, sw = gate(hidden, self.w_gate, self.topk, renormalize=self.renormalize,
                            w_shared_gate=self.w_shared_gate, **self.routing)
        res = self.ffn.forward(hidden, ids, wts, sw, return_intermediates=return_intermediates)
        if return_intermediates:
            out, mid = res
            mid.update(topk_ids=ids, topk_weights=wts, shared_w=sw)
            return out, mid
        return res


class PlannedForward:
    """MoEFFN.forward for a fixed routing with every launch planned once: the plumbing kernels
    relaunch on the same buffers and both GroupGEMMs keep their plans (the device work of a serving
    step whose routing shapes repeat; the host planning MoEFFN.forward redoes per call is left out).
    ``stages`` maps stage name -> launch; calling the object runs them in order into ``out``."""

    def __init__(self, layer: "MoEFFN", hidden: torch.Tensor, topk_ids: torch.Tensor, topk_weights: torch.Tensor):
        dev = hidden.device
        T = hidden.shape[0]
        self.r = r = route(topk_ids, layer.E)
        topk = r.topk
        self.a1 = quant_act(hidden, r, layer.tag1, layer.has_shared)
        self.g1, self.h1, self.h1s, self.mode = layer.gate_up_call(self.a1, T, topk, dev)
        self.a2 = layer.act_quant(self.h1, self.h1s, r, self.mode)
        self.g2, self.y, self.ys = layer.down_call(self.a2, T, topk, dev)
        self.out = torch.empty(T, layer.H, dtype=hidden.dtype, device=dev)
        self.w = _f32(topk_weights)
        comb = functools.partial(_launch_combine, self.out, self.y, r.inv_slot, r.sorted_expert, self.w, self.ys, None, topk,
                                 None, layer.down_bias)
        self.stages = {"quant_act": self.a1.relaunch, "gate_up": self.g1.launch, "act_quant": self.a2.relaunch,
                       "down": self.g2.launch, "combine": comb}

    def __call__(self) -> torch.Tensor:
        for fn in self.stages.values():
            fn()
        return self.out


class GraphForward:
    """A MoE layer (``MoEFFN``, or a ``MoEBlock`` with its router) planned once for ``T`` tokens whatever the
    routing: every buffer is allocated and both GroupGEMMs are planned here, at capacity (DynamicGroupGemm),
    and ``launch`` only issues kernel launches — gate (block only) -> route -> segments -> quant_act -> gate_up
    -> SiLU / quant -> down -> combine — with nothing copied to the host, so it can be captured with
    ``torch.cuda.graph`` and replayed while the routing changes (DESIGN.md §4 "Device planning / graph forward").

    The segment tables and the GroupGEMMs' row tables are written on the device from the routing counts
    (mxmoe_moe_segments), the tile tables by the device planner. Activation stores are sized for the worst case
    over the layer's tags; h1, y and out have their usual sizes. The gate_up mode ("fused" / "interleaved" /
    "plain") is fixed here from the chosen variant's capabilities, as ``MoEFFN.gate_up_call`` does per call.
    ``inv_slot`` starts zeroed: an id outside [0, E) spoils that token's value but every access stays inside the
    buffers; ``status()`` reports it (bit SEG_STATUS_SHIFT: the counts did not sum to T * topk; low bits: the
    MXMOE_GG_DYN_* bits of the two GroupGEMMs — all zero for a clean run)."""

    SEG_STATUS_SHIFT = 4

    def __init__(self, layer, T: int, topk: Optional[int] = None, device=None, dtype: Optional[torch.dtype] = None):
        """dtype: the element type of ``hidden`` and ``out`` (fp16 or bf16); default: the block's ``w_gate.dtype``
        (which it must equal), fp16 for a bare ``MoEFFN``. Every buffer between the two ends is fp16."""
        self.block = layer if isinstance(layer, MoEBlock) else None
        self.ffn = ffn = layer.ffn if self.block is not None else layer
        if dtype is None:
            dtype = self.block.w_gate.dtype if self.block is not None else torch.float16
        _check_io_dtype(dtype, "dtype")
        if self.block is not None and dtype != self.block.w_gate.dtype:
            raise ValueError(f"dtype = {dtype} differs from the block's router ({self.block.w_gate.dtype})")
        self.dtype = dtype
        if self.block is not None:
            if topk is not None and topk != self.block.topk:
                raise ValueError(f"topk = {topk} differs from the block's {self.block.topk}")
            topk = self.block.topk
        if topk is None or topk < 1 or T < 1:
            raise ValueError("GraphForward needs T >= 1 and, for a MoEFFN, topk >= 1")
        dev = torch.device(device) if device is not None else ffn.w1[0].B.device
        self.T, self.topk, self.device = T, topk, dev
        E, H, N, Ns, shared = ffn.E, ffn.H, ffn.N, ffn.Ns, ffn.has_shared
        n, nseg = T * topk, ffn.E + (1 if ffn.has_shared else 0)
        self.nseg = nseg
        i32 = dict(dtype=torch.int32, device=dev)
        # routing: zeroed once (slots an invalid id leaves unwritten then point at slot / expert 0)
        self.route_bufs = tuple(torch.zeros(n, **i32) for _ in range(3)) + (torch.zeros(E, **i32),)
        self.gate_out = None
        if self.block is not None:
            self.gate_out = (torch.zeros(T, topk, **i32), torch.zeros(T, topk, dtype=torch.float32, device=dev),
                             torch.zeros(T, dtype=torch.float32, device=dev) if self.block.w_shared_gate is not None else None)
        self.tags = [torch.tensor(t, **i32) for t in (ffn.tag1, ffn.tag2)]
        self.segs = [torch.zeros(nseg * ctypes.sizeof(nat.MoeSegC), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.dyn = [torch.zeros(nseg, ctypes.sizeof(nat.GGDynRowC), dtype=torch.uint8, device=dev) for _ in range(2)]
        self.seg_status = torch.zeros(1, **i32)

        def stores(tags, w, ws):
            """Worst-case activation and scale stores over the tags present (16-B / dword padding per segment)."""
            nbytes = n * w * max(_BITS[t] for t in tags[:E]) // 8 + 16 * E
            nscale = n * max(_scale_elems(t, w) for t in tags[:E]) + E
            if shared:
                nbytes += T * ws * _BITS[tags[E]] // 8 + 16
                nscale += T * _scale_elems(tags[E], ws) + 1
            return (torch.zeros(nbytes, dtype=torch.uint8, device=dev),
                    torch.zeros(max(nscale, 1), dtype=torch.float16, device=dev))

        self.a1, self.s1 = stores(ffn.tag1, H, H)
        self.a2, self.s2 = stores(ffn.tag2, N, Ns)
        self.mask1, self.mask2 = _tag_mask(ffn.tag1), _tag_mask(ffn.tag2)

        def plan(ws, store, scales, tags, C_routed, C_shared, silu):
            ps = []
            for e in range(nseg):
                w = ws[e]
                tag = tags[e]
                A = store.view(torch.float16) if tag == ACT_FP16 else store
                sa = None if tag == ACT_FP16 else scales.view(torch.uint8) if tag in _MX_TAGS else scales
                ps.append(Problem(A=A, B=w.B, C=C_shared if e == E else C_routed, M=T if e == E else n, N=w.N, K=w.K,
                                  q=w.q, scale_a=sa, scale_b=w.scale_b, silu=silu))
            return DynamicGroupGemm(ps, joint=range(E), rows_total=n, device=dev)

        self.mode = ffn.gate_up_layout()
        if ffn.biased_or_gated and self.mode != "plain":
            raise ValueError("a layer with a bias or another activation needs the plain gate_up layout")
        self._glu = _glu_struct(ffn.activation, ffn.b1, ffn.b1s) if ffn.biased_or_gated else None
        while True:
            f = 1 if self.mode == "fused" else 2
            self.h1 = torch.zeros(n, f * N, dtype=torch.float16, device=dev)
            self.h1s = torch.zeros(T, f * Ns, dtype=torch.float16, device=dev) if shared else None
            try:
                self.g1 = plan(ffn.w1, self.a1, self.s1, ffn.tag1, self.h1, self.h1s, self.mode == "fused")
                break
            except nat.GGError as err:  # the variant chosen at capacity has no SiLU epilogue for these types
                if self.mode != "fused" or err.status != nat.MXMOE_GG_ERR_UNSUPPORTED:
                    raise
                self.mode = "interleaved"
        self.y = torch.zeros(n, H, dtype=torch.float16, device=dev)
        self.ys = torch.zeros(T, H, dtype=torch.float16, device=dev) if shared else None
        self.g2 = plan(ffn.w2, self.a2, self.s2, ffn.tag2, self.y, self.ys, False)
        self.out = torch.zeros(T, H, dtype=dtype, device=dev)
        self._tables = (nat.MoeSegTableC * 2)(
            nat.MoeSegTableC(self.tags[0].data_ptr(), H, H if shared else 0, self.h1.shape[1], self.segs[0].data_ptr(),
                             self.dyn[0].data_ptr()),
            nat.MoeSegTableC(self.tags[1].data_ptr(), N, Ns, H, self.segs[1].data_ptr(), self.dyn[1].data_ptr()))

    def launch(self, hidden: torch.Tensor, topk_ids: Optional[torch.Tensor] = None,
               topk_weights: Optional[torch.Tensor] = None, shared_w: Optional[torch.Tensor] = None,
               stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """Launches only; returns ``self.out`` ([T, H] of ``self.dtype``, which hidden must have). A MoEFFN takes int32 ids and f32 weights [T, topk]
        (contiguous, as nothing may be converted here) and the optional f32 shared_w [T]; a MoEBlock routes itself."""
        ffn, T, topk = self.ffn, self.T, self.topk
        if tuple(hidden.shape) != (T, ffn.H) or hidden.dtype != self.dtype or not hidden.is_contiguous():
            raise ValueError(f"hidden must be a contiguous {self.dtype} [{T}, {ffn.H}] tensor, got {hidden.dtype} "
                             f"{list(hidden.shape)}")
        if self.block is not None:
            if topk_ids is not None or topk_weights is not None or shared_w is not None:
                raise ValueError("a MoEBlock routes itself: launch(hidden)")
            b = self.block
            topk_ids, topk_weights, shared_w = gate(hidden, b.w_gate, topk, renormalize=b.renormalize,
                                                    w_shared_gate=b.w_shared_gate, stream=stream, out=self.gate_out,
                                                    **b.routing)
        else:
            for t, dt, shape, what in ((topk_ids, torch.int32, (T, topk), "topk_ids"),
                                       (topk_weights, torch.float32, (T, topk), "topk_weights"),
                                       (shared_w, torch.float32, (T,), "shared_w")):
                if t is None and what == "shared_w":
                    continue
                if t is None or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"{what} must be a contiguous {dt} {list(shape)} tensor")
        sorted_e, perm, inv, counts = route_device(topk_ids, ffn.E, stream, out=self.route_bufs)
        shared = ffn.has_shared
        nat.check(nat.lib().mxmoe_moe_segments(_ptr(counts), ffn.E, T, topk, int(shared), self._tables, 2,
                                               _ptr(self.seg_status), _stream(stream)))
        _launch_act("gather", None, hidden, hidden if shared else None, T, topk, ffn.H, ffn.H, sorted_e, perm, self.segs[0],
                    self.nseg, self.mask1, self.a1, self.s1, stream)
        self.g1.launch(self.dyn[0], stream)
        _launch_act(self.mode, self._glu, self.h1, self.h1s, T, topk, ffn.N, ffn.Ns, sorted_e, None, self.segs[1],
                    self.nseg, self.mask2, self.a2, self.s2, stream)
        self.g2.launch(self.dyn[1], stream)
        _launch_combine(self.out, self.y, inv, sorted_e, topk_weights, self.ys, shared_w, topk, stream, ffn.down_bias)
        return self.out

    __call__ = launch

    def status(self, reset: bool = False) -> int:
        """0 for a clean history; synchronises (not for use under capture)."""
        seg = int(self.seg_status.item())
        if reset:
            self.seg_status.zero_()
        return self.g1.status(reset) | self.g2.status(reset) | (seg << self.SEG_STATUS_SHIFT)


class _DecodeBase:
    """What ``DecodeForward`` and ``DecodeForwardEx`` share: the constructor, ``launch`` and ``status``. A subclass names
    its kinds (``KINDS``: qcfg -> MXMOE_DECODE_*), its two entries (``ENTRIES``), whether the gate_up entry takes an
    mxmoe_moe_glu (``TAKES_GLU``) and what it refuses about a layer (``_check_layer``)."""

    MAX_T = nat.DECODE_MAX_T
    KINDS: dict = {}
    ENTRIES: tuple = ()
    TAKES_GLU = False
    TAKES_MX = False  # e8m0 scale rows are read by row and byte offset: they are checked like the weights

    def _check_layer(self, ffn: "MoEFFN") -> None:
        """What the class refuses about a layer beyond the experts' types."""

    def _check_scale(self, w: "ExpertWeights", dev) -> None:
        """What the class refuses about a weight's scale buffer (a kind whose kernel indexes it by more than the row)."""

    def __init__(self, layer, T: int, topk: Optional[int] = None, device=None, dtype: Optional[torch.dtype] = None):
        """T: the capacity in tokens (1..16; an uncaptured call may bring fewer rows). dtype: the element type of
        ``hidden`` and ``out`` (fp16 or bf16); default: the block's ``w_gate.dtype`` (which it must equal), fp16 for
        a bare ``MoEFFN``."""
        name = type(self).__name__
        self.block = layer if isinstance(layer, MoEBlock) else None
        self.ffn = ffn = layer.ffn if self.block is not None else layer
        if dtype is None:
            dtype = self.block.w_gate.dtype if self.block is not None else torch.float16
        _check_io_dtype(dtype, "dtype")
        if self.block is not None and dtype != self.block.w_gate.dtype:
            raise ValueError(f"dtype = {dtype} differs from the block's router ({self.block.w_gate.dtype})")
        self.dtype = dtype
        if self.block is not None:
            if topk is not None and topk != self.block.topk:
                raise ValueError(f"topk = {topk} differs from the block's {self.block.topk}")
            topk = self.block.topk
        if topk is None or topk < 1 or topk > min(ffn.E, 16):
            raise ValueError(f"{name} needs 1 <= topk <= min(E, 16), got {topk}")
        if T < 1 or T > self.MAX_T:
            raise ValueError(f"{name} takes 1 <= T <= {self.MAX_T} tokens, got T = {T}: larger batches are "
                             "GraphForward's")
        self._check_layer(ffn)
        for w in list(ffn.w1) + list(ffn.w2):
            if w.q.qcfg not in self.KINDS:
                raise ValueError(f"{name}: qcfg {w.q.qcfg} is not supported (experts must be one of "
                                 f"{tuple(self.KINDS)})")
        for what, v in (("H", ffn.H), ("N", ffn.N)) + ((("N_shared", ffn.Ns),) if ffn.has_shared else ()):
            if v <= 0 or v % 128 or v > 16384:
                raise ValueError(f"{name}: {what} = {v} must be a multiple of 128 and <= 16384")
        dev = torch.device(device) if device is not None else ffn.w1[0].B.device
        self.T, self.topk, self.device = T, topk, dev
        n, H = T * topk, ffn.H
        self.layout = nat.DECODE_GU_INTERLEAVED if ffn.fuse_silu else nat.DECODE_GU_PLAIN
        kinds1 = [self.KINDS[w.q.qcfg] for w in ffn.w1]
        kinds2 = [self.KINDS[w.q.qcfg] for w in ffn.w2]
        self.mask1, self.mask2 = _tag_mask(kinds1), _tag_mask(kinds2)
        table = (nat.MoeDecodeExpertC * len(ffn.w1))()
        for rec, w1, w2, k1, k2 in zip(table, ffn.w1, ffn.w2, kinds1, kinds2):
            for w in (w1, w2):
                if w.B.device != dev or not w.B.is_contiguous() or w.B.data_ptr() % 16:
                    raise ValueError(f"{name}: every weight must be a contiguous, 16-byte aligned tensor on the "
                                     "layer's device")
                if self.TAKES_MX and w.scale_b is not None and (w.scale_b.device != dev or not w.scale_b.is_contiguous()):
                    raise ValueError(f"{name}: every scale_b must be a contiguous tensor on the layer's device")
                self._check_scale(w, dev)
            rec.b1, rec.sb1 = w1.B.data_ptr(), 0 if w1.scale_b is None else w1.scale_b.data_ptr()
            rec.b2, rec.sb2 = w2.B.data_ptr(), 0 if w2.scale_b is None else w2.scale_b.data_ptr()
            rec.kind1, rec.kind2 = k1, k2
        self.experts = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).to(dev)
        # a layer with a bias or another activation (the _ex entries only): the gate_up entry's mxmoe_moe_glu, and the
        # combine with the down bias (``MoEFFN.down_bias``) — the eager layer's own choice of calls
        self._glu = None
        if self.TAKES_GLU and ffn.biased_or_gated:
            _check_bias(ffn.b1, (ffn.E, 2 * ffn.N), "gate_up_bias", dev)
            _check_bias(ffn.b1s, (2 * ffn.Ns,), "gate_up_bias (shared)", dev)
            self._glu = _glu_struct(ffn.activation, ffn.b1, ffn.b1s)
        f16 = dict(dtype=torch.float16, device=dev)
        self.act = torch.zeros(n, ffn.N, **f16)
        self.act_shared = torch.zeros(T, ffn.Ns, **f16) if ffn.has_shared else None
        self.y = torch.zeros(n, H, **f16)
        self.ys = torch.zeros(T, H, **f16) if ffn.has_shared else None
        self.out = torch.zeros(T, H, dtype=dtype, device=dev)
        self.inv_slot = torch.arange(n, dtype=torch.int32, device=dev)  # pair order: the combine's identity table
        self.dev_status = torch.zeros(1, dtype=torch.int32, device=dev)
        self.gate_out = None
        if self.block is not None:
            i32 = dict(dtype=torch.int32, device=dev)
            self.gate_out = (torch.zeros(T, topk, **i32), torch.zeros(T, topk, dtype=torch.float32, device=dev),
                             torch.zeros(T, dtype=torch.float32, device=dev) if self.block.w_shared_gate is not None else None)

    def launch(self, hidden: torch.Tensor, topk_ids: Optional[torch.Tensor] = None,
               topk_weights: Optional[torch.Tensor] = None, shared_w: Optional[torch.Tensor] = None,
               stream: Optional[torch.cuda.Stream] = None) -> torch.Tensor:
        """Launches only; returns ``self.out`` (its first rows for a call with fewer than ``T`` rows). A MoEFFN takes
        int32 ids and f32 weights [rows, topk] (contiguous, as nothing may be converted here) and the optional f32
        shared_w [rows]; a MoEBlock routes itself."""
        ffn, topk = self.ffn, self.topk
        T = hidden.shape[0] if hidden.dim() == 2 else -1
        if not 1 <= T <= self.T or hidden.shape[1] != ffn.H or hidden.dtype != self.dtype or not hidden.is_contiguous():
            raise ValueError(f"hidden must be a contiguous {self.dtype} [1..{self.T}, {ffn.H}] tensor, got {hidden.dtype} "
                             f"{list(hidden.shape)}")
        if self.block is not None:
            if topk_ids is not None or topk_weights is not None or shared_w is not None:
                raise ValueError("a MoEBlock routes itself: launch(hidden)")
            b = self.block
            out = tuple(None if t is None else t[:T] for t in self.gate_out)
            topk_ids, topk_weights, shared_w = gate(hidden, b.w_gate, topk, renormalize=b.renormalize,
                                                    w_shared_gate=b.w_shared_gate, stream=stream, out=out, **b.routing)
        else:
            for t, dt, shape, what in ((topk_ids, torch.int32, (T, topk), "topk_ids"),
                                       (topk_weights, torch.float32, (T, topk), "topk_weights"),
                                       (shared_w, torch.float32, (T,), "shared_w")):
                if t is None and what == "shared_w":
                    continue
                if t is None or t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
                    raise ValueError(f"{what} must be a contiguous {dt} {list(shape)} tensor")
        shared = int(ffn.has_shared)
        st = _stream(stream)
        gate_up, down = self.ENTRIES
        glu = (self._glu,) if self.TAKES_GLU else ()
        nat.check(nat.symbol(gate_up)(
            *glu, _DT[self.dtype], _ptr(hidden), T, topk, ffn.E, shared, _ptr(topk_ids), _ptr(self.experts), self.mask1, ffn.H,
            ffn.N, ffn.Ns, self.layout, _ptr(self.act), _ptr(self.act_shared), _ptr(self.dev_status), st))
        nat.check(nat.symbol(down)(
            T, topk, ffn.E, shared, _ptr(topk_ids), _ptr(self.experts), self.mask2, ffn.H, ffn.N, ffn.Ns, _ptr(self.act),
            _ptr(self.act_shared), _ptr(self.y), _ptr(self.ys), _ptr(self.dev_status), st))
        out = self.out[:T]
        if self._glu is not None:  # in pair order the expert of slot p is ids[p]; an id outside [0, E) adds no bias
            _launch_combine(out, self.y, self.inv_slot, topk_ids.view(-1), topk_weights, self.ys, shared_w, topk, stream,
                            ffn.down_bias)
        else:
            _launch_combine(out, self.y, self.inv_slot, None, topk_weights, self.ys, shared_w, topk, stream, None)
        return out

    __call__ = launch

    def status(self, reset: bool = False) -> int:
        """0 for a clean history (bits ``_native.DECODE_BAD_ID`` / ``DECODE_BAD_KIND``); synchronises (not for use
        under capture)."""
        st = int(self.dev_status.item())
        if reset:
            self.dev_status.zero_()
        return st


class DecodeForward(_DecodeBase):
    """A MoE layer (``MoEFFN``, or a ``MoEBlock`` with its router) for calls of 1 to ``DECODE_MAX_T`` (16) tokens, with
    no planner: gate (block only) -> decode_gate_up -> decode_down -> combine, three launches (four with the router),
    nothing copied to the host, so ``launch`` can be captured with ``torch.cuda.graph`` like ``GraphForward``'s
    (DESIGN.md §4 "Decode forward"). There is no sort, no segment table and no tile table: the two kernels
    (mxmoe_moe_decode_gate_up / mxmoe_moe_decode_down, include/mxmoe_moe.h) stream the weights of the experts the ids
    name and write ``act`` and ``y`` in pair order (row t * topk + k), which the existing combine reads through an
    identity slot table. The arithmetic is ``MoEFFN.forward``'s: for w8a8 / w4a4 experts ``out`` equals it bit for
    bit, for fp16 experts within the f32 summation order.

    Experts may be fp16, w8a8_g-1_sym or w4a4_g-1_sym, mixed freely per expert and per linear; the weights are the
    layer's own tensors (no copy). Anything else — the MX and weight-only types, g128, a layer with a bias or
    another activation — raises ValueError here (``DecodeForwardEx`` takes gpt-oss layers, ``DecodeForwardWo`` the
    integer weight-only types). An id outside [0, E)
    leaves its pair's rows as they were and sets ``DECODE_BAD_ID`` in ``status()``; every access stays inside the
    buffers."""

    KINDS = {"fp16": nat.DECODE_FP16, "w8a8_g-1_sym": nat.DECODE_W8A8, "w4a4_g-1_sym": nat.DECODE_W4A4}
    ENTRIES = ("mxmoe_moe_decode_gate_up", "mxmoe_moe_decode_down")

    def _check_layer(self, ffn: "MoEFFN") -> None:
        if ffn.biased_or_gated:
            raise ValueError("DecodeForward: a layer with a bias or an activation other than 'silu' (gpt-oss) is not "
                             "supported")


class DecodeForwardEx(_DecodeBase):
    """``DecodeForward`` for gpt-oss layers (DESIGN.md §4 "Decode forward: gpt-oss layers"): the same constructor,
    ``launch`` and ``status`` on the _ex entries (mxmoe_moe_decode_gate_up_ex / mxmoe_moe_decode_down_ex,
    include/mxmoe_moe.h), which also take

    - ``w4a16_g32_sym_MXFP4`` experts (``gptoss_layer``, ``prepare_weight_mx``: the checkpoint's codes and the e8m0
      scales in the GroupGEMM's device layout, read in place), mixed freely with fp16, w8a8_g-1_sym and w4a4_g-1_sym
      per expert and per linear;
    - a layer that is ``biased_or_gated``: any of the four biases, and "silu" or a ``SwigluClamp``. The gate_up
      biases and the activation are applied in decode_gate_up's epilogue with the activation pass's arithmetic
      (mxmoe_moe_glu_quant); the down biases stay in the combine, as in ``MoEFFN.forward``, which reads the expert of
      pair p from ``topk_ids`` (pair order) and adds no bias for an id outside [0, E).

    So a gpt-oss MoE block decodes as router -> decode_gate_up -> decode_down -> combine, launches only, with fp16 or
    bf16 ends. ``out`` equals ``MoEFFN.forward``'s bit for bit for w8a8 / w4a4 experts and within the f32 summation
    order for fp16 and MXFP4 experts. Still refused, naming the qcfg: w4a4_g32_sym_MXFP4, w4a8_g32_sym_MXFP8, g128
    and the integer weight-only types (``DecodeForwardWo`` takes those).

    On the gpt-oss layer shape (E = 32, topk = 4, H = N = 2944) this form takes 0.56x / 0.71x of ``GraphForward``'s
    device time at T = 1 / 4, 0.94x at T = 6 and 1.14x / 1.48x at T = 8 / 16: the crossover is between 6 and 8
    tokens, so take ``GraphForward`` from 8."""

    KINDS = dict(DecodeForward.KINDS, **{"w4a16_g32_sym_MXFP4": nat.DECODE_W4A16_MX})
    ENTRIES = nat.DECODE_EX_SYMBOLS
    TAKES_GLU = True
    TAKES_MX = True


class DecodeForwardWo(_DecodeBase):
    """``DecodeForwardEx`` for layers with integer weight-only experts (DESIGN.md §4 "Decode forward: weight-only
    experts"): the same constructor, ``launch`` and ``status`` on the _wo entries (mxmoe_moe_decode_gate_up_wo /
    mxmoe_moe_decode_down_wo, include/mxmoe_moe.h), which take everything the _ex entries take and also

    - ``w4a16`` and ``w8a16`` experts, per-channel (``g-1``) or ``g128``, ``sym`` or ``asym``: ``prepare_weight``'s
      repacked codes and its [G][rows] / [G][rows][2] fp16 scale buffer, read in place, mixed freely with the other
      kinds per expert and per linear. The A row stays fp16; a weight is fp16(fma(u - off, scale, zp)), the
      GroupGEMM's value, and a row's sum is accumulated in f32 in the kernel's order: ``out`` is within the f32
      summation order of ``MoEFFN.forward``'s.

    Which class takes which layer: ``DecodeForward`` fp16 / w8a8 / w4a4 experts with SiLU and no bias;
    ``DecodeForwardEx`` those plus w4a16_g32_sym_MXFP4, biases and ``SwigluClamp`` (gpt-oss); ``DecodeForwardWo``
    all of that plus the eight integer weight-only types — the reference's small-batch scheme w4a16 + w8a8
    (``workload.w4a16_w8a8_qconfig``) is a layer for this class. Still refused, naming the qcfg: w2a16, group sizes
    other than -1 and 128, w4a4_g32_sym_MXFP4, w4a8_g32_sym_MXFP8, w4a4_g128, E4M3 and bf16 experts.

    On qwen2_moe layer 11 with the w4a16 + w8a8 scheme (E = 60, topk = 4, the shared expert included) this form takes
    0.37x / 0.51x / 0.66x of ``GraphForward``'s device time at T = 1 / 4 / 6, 0.99x at T = 8 and 1.32x / 1.68x at
    T = 12 / 16: take ``GraphForward`` from T = 8."""

    KINDS = dict(DecodeForwardEx.KINDS, **{f"w{b}a16_g{g}_{'sym' if s else 'asym'}": nat.decode_wo_kind(b, g, s)
                                           for b in (4, 8) for g in (-1, 128) for s in (True, False)})
    ENTRIES = nat.DECODE_WO_SYMBOLS
    TAKES_GLU = True
    TAKES_MX = True

    def _check_scale(self, w: "ExpertWeights", dev) -> None:
        """The weight-only kernel reads scale_b by group and row: the buffer is checked like the weights."""
        q = w.q
        if not q.is_weight_only or q.fmt:  # (the MX kind's e8m0 rows: TAKES_MX's check)
            return
        want = (1 if q.gsize == -1 else w.K // q.gsize) * w.N * (1 if q.sym else 2)
        sb = w.scale_b
        if (sb is None or sb.device != dev or sb.dtype != torch.float16 or not sb.is_contiguous() or sb.data_ptr() % 2 or
                sb.numel() != want):
            raise ValueError(f"DecodeForwardWo: the scale buffer of a {q.qcfg} weight [{w.N}, {w.K}] must be a contiguous "
                             f"fp16 tensor of {want} elements on the layer's device")


def qwen2_layer_bench(*args, **kwargs) -> dict:
    """``moe_bench.qwen2_layer_bench`` under the name bench.py imports (the benchmarks live in mxmoe_amd/moe_bench.py)."""
    from .moe_bench import qwen2_layer_bench as bench
    return bench(*args, **kwargs)
