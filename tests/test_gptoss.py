"""gpt-oss MoE layers without a GPU: the numpy reference (tests/_gptoss_ref.py) pinned to the public model code, the
checkpoint loader, prepare_weight_mx, the three entry points' argument validation and MoEFFN's rules."""
from __future__ import annotations

import ctypes
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mxmoe_amd import _native as nat
from mxmoe_amd import moe
from mxmoe_amd.groupgemm import FP16, W4A4_MXFP4, W4A8_MXFP8, W4A16_MXFP4
from mxmoe_amd.quantize import dequant_mxfp4, quant_mxfp4, unpack_mxfp4_scales
from tests import _gptoss_ref as ref


# ------------------------------------------------------------------ the reference against the public model

def test_reference_activation_matches_transformers():
    m = pytest.importorskip("transformers.models.gpt_oss.modeling_gpt_oss")
    rng = np.random.default_rng(0)
    R, N = 64, 96
    g = rng.uniform(-12, 12, (R, N)).astype(np.float32)
    u = rng.uniform(-12, 12, (R, N)).astype(np.float32)
    g[0, :4], u[0, :4] = [7, -7, 7.5, 0], [7, -7, -7.5, 0]
    inter = np.empty((R, 2 * N), np.float32)  # the model's layout: gate / up alternate
    inter[:, 0::2], inter[:, 1::2] = g, u
    want = m.GptOssExperts._apply_gate(SimpleNamespace(alpha=ref.ALPHA, limit=ref.LIMIT), torch.from_numpy(inter)).numpy()
    got = ref.swiglu_clamp_f32(g, u)
    # f32 rounding: both are a handful of correctly rounded f32 operations on the same clamped inputs (libm exp vs
    # torch's sigmoid: a few ulps), so a few units in the last place of the result
    assert np.allclose(got, want, rtol=8 * 2.0 ** -24, atol=1e-30)
    assert (got[0, :4] == want[0, :4]).all() or np.allclose(got[0, :4], want[0, :4], rtol=8 * 2.0 ** -24)


def test_reference_router_matches_transformers():
    m = pytest.importorskip("transformers.models.gpt_oss.modeling_gpt_oss")
    rng = np.random.default_rng(1)
    T, H, E, topk = 50, 64, 32, 4
    hidden = rng.standard_normal((T, H)).astype(np.float32)
    w = (rng.standard_normal((E, H)) * H ** -0.5).astype(np.float32)
    b = rng.standard_normal(E).astype(np.float32)
    r = SimpleNamespace(top_k=topk, weight=torch.from_numpy(w), bias=torch.from_numpy(b))
    logits, scores, ids = m.GptOssTopKRouter.forward(r, torch.from_numpy(hidden))
    got_ids, got_w = ref.router(logits.numpy(), topk)  # (the same f32 logits: the selection then has no rounding in it)
    assert (got_ids == ids.numpy()).all()
    assert np.allclose(got_w, scores.numpy(), rtol=8 * 2.0 ** -24)
    assert np.allclose(got_w.sum(axis=1), 1, atol=1e-6)


def test_reference_layer_matches_transformers_experts():
    m = pytest.importorskip("transformers.models.gpt_oss.modeling_gpt_oss")
    rng = np.random.default_rng(2)
    T, H, N, E, topk = 12, 32, 48, 6, 3
    hidden = rng.standard_normal((T, H))
    w_gate, lb = rng.standard_normal((E, H)) * H ** -0.5, rng.standard_normal(E)
    gate_up, b1 = rng.standard_normal((E, 2 * N, H)) * 0.3, rng.standard_normal((E, 2 * N))  # [gate; up] rows
    down, b2 = rng.standard_normal((E, H, N)) * 0.3, rng.standard_normal((E, H))
    got = ref.layer(hidden, w_gate, lb, gate_up, b1, down, b2, topk)
    ex = SimpleNamespace(num_experts=E, alpha=ref.ALPHA, limit=ref.LIMIT)
    ex._apply_gate = lambda x: m.GptOssExperts._apply_gate(ex, x)
    inter = np.empty((E, 2 * N, H))
    inter[:, 0::2], inter[:, 1::2] = gate_up[:, :N], gate_up[:, N:]
    bi = np.empty((E, 2 * N))
    bi[:, 0::2], bi[:, 1::2] = b1[:, :N], b1[:, N:]
    ex.gate_up_proj, ex.gate_up_proj_bias = torch.from_numpy(inter).transpose(1, 2), torch.from_numpy(bi)
    ex.down_proj, ex.down_proj_bias = torch.from_numpy(down).transpose(1, 2), torch.from_numpy(b2)
    r = SimpleNamespace(top_k=topk, weight=torch.from_numpy(w_gate), bias=torch.from_numpy(lb))
    _, scores, ids = m.GptOssTopKRouter.forward(r, torch.from_numpy(hidden))
    forward = getattr(m.GptOssExperts.forward, "__wrapped__", m.GptOssExperts.forward)  # (the plain loop, undecorated)
    want = forward(ex, torch.from_numpy(hidden), ids, scores).numpy()
    assert np.allclose(got, want, rtol=1e-10, atol=1e-10)  # both float64


def test_reference_fma_agrees_with_the_oracle_where_that_applies():
    from oracle import moe_ref

    rng = np.random.default_rng(3)
    a = rng.uniform(0, 1, (64, 1)).astype(np.float32)
    b = rng.uniform(-1, 1, (64, 256)).astype(np.float16).astype(np.float32)
    c = rng.uniform(-1, 1, (64, 256)).astype(np.float32)
    assert (ref.fma_f32(a, b, c) == moe_ref.fma_f32(a, b, c)).all()
    # wide b (a 24-bit sum) against a large c: the oracle's exactness check refuses, the fallback must equal the
    # correctly rounded exact value (python fractions)
    from fractions import Fraction

    b2 = (rng.uniform(-1, 1, (8, 64)).astype(np.float32) * np.float32(2.0 ** -12)).astype(np.float32)
    c2 = rng.uniform(1, 2, (8, 64)).astype(np.float32)
    a2 = rng.uniform(0, 1, (8, 1)).astype(np.float32)
    got = ref.fma_f32(a2, b2, c2)
    for i in range(8):
        for j in range(64):
            exact = Fraction(float(a2[i, 0])) * Fraction(float(b2[i, j])) + Fraction(float(c2[i, j]))
            lo = np.float32(float(exact))  # float(Fraction) rounds correctly to f64; then check against neighbours
            cands = [lo, np.nextafter(lo, np.float32(np.inf)), np.nextafter(lo, np.float32(-np.inf))]
            best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
            assert got[i, j] == best


# ------------------------------------------------------------------ loader

def test_loader_on_a_synthetic_checkpoint():
    E, N, H = 4, 96, 160
    ck = ref.synthetic_checkpoint(E, N, H, seed=5)
    ck["gate_up_scales"][1, 3, 2] = 90   # planted: two bytes outside [104, 140]
    ck["down_scales"][2, 7, 1] = 150
    with pytest.warns(UserWarning, match="2 scale bytes"):
        layer = moe.gptoss_layer(ck["gate_up_blocks"], ck["gate_up_scales"], ck["gate_up_bias"], ck["down_blocks"],
                                 ck["down_scales"], ck["down_bias"], act_bits=16, pad_to=128)
    assert layer.scale_out_of_range == 2
    assert (layer.E, layer.N, layer.H, layer.has_shared) == (E, 128, 256, False)
    assert layer.activation == moe.SwigluClamp(1.702, 7.0) and not layer.fuse_silu and layer.biased_or_gated
    assert all(q.qcfg == "w4a16_g32_sym_MXFP4" for pair in layer.qcfg for q in pair)
    for e in range(E):
        w1, w2 = layer.w1[e], layer.w2[e]
        assert (w1.N, w1.K, w2.N, w2.K) == (256, 256, 256, 128)
        gu = dequant_mxfp4(ck["gate_up_blocks"][e].reshape(2 * N, H // 2), ck["gate_up_scales"][e])
        want = torch.zeros(256, 256, dtype=torch.float64)
        want[:N, :H], want[128:128 + N, :H] = gu[0::2], gu[1::2]
        got = dequant_mxfp4(w1.B, unpack_mxfp4_scales(w1.scale_b, w1.K))
        assert torch.equal(got, want)
        dn = dequant_mxfp4(ck["down_blocks"][e].reshape(H, N // 2), ck["down_scales"][e])
        want = torch.zeros(256, 128, dtype=torch.float64)
        want[:H, :N] = dn
        assert torch.equal(dequant_mxfp4(w2.B, unpack_mxfp4_scales(w2.scale_b, w2.K)), want)
        b = ck["gate_up_bias"][e].half()
        wb = torch.zeros(256, dtype=torch.float16)
        wb[:N], wb[128:128 + N] = b[0::2], b[1::2]
        assert torch.equal(layer.b1[e], wb)
        wd = torch.zeros(256, dtype=torch.float16)
        wd[:H] = ck["down_bias"][e].half()
        assert torch.equal(layer.b2[e], wd)
    assert layer.b1s is None and layer.b2s is None
    for bits, name in ((8, "w4a8_g32_sym_MXFP8"), (4, "w4a4_g32_sym_MXFP4")):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            other = moe.gptoss_layer(ck["gate_up_blocks"], ck["gate_up_scales"], ck["gate_up_bias"], ck["down_blocks"],
                                     ck["down_scales"], ck["down_bias"], act_bits=bits)
        assert other.qcfg[0][0].qcfg == name and torch.equal(other.w1[0].B, layer.w1[0].B)
    with pytest.raises(ValueError):
        moe.gptoss_layer(ck["gate_up_blocks"], ck["gate_up_scales"], ck["gate_up_bias"], ck["down_blocks"],
                         ck["down_scales"], ck["down_bias"], act_bits=2)
    with pytest.raises(ValueError):
        moe.gptoss_layer(ck["gate_up_blocks"], ck["gate_up_scales"][:, :, :2], ck["gate_up_bias"], ck["down_blocks"],
                         ck["down_scales"], ck["down_bias"])


def test_pad_cols():
    t = torch.arange(6, dtype=torch.float16).reshape(2, 3)
    p = moe.pad_cols(t, 8)
    assert p.shape == (2, 8) and torch.equal(p[:, :3], t) and (p[:, 3:] == 0).all() and p.is_contiguous()
    assert moe.pad_cols(t, 3).data_ptr() == t.data_ptr()
    with pytest.raises(ValueError):
        moe.pad_cols(t, 2)


def test_prepare_weight_mx_shares_tensors_and_counts_scales():
    g = torch.Generator().manual_seed(6)
    w = ((torch.rand(64, 128, generator=g) * 2 - 1) * 0.3).half()
    codes, scales = quant_mxfp4(w)
    ws = [moe.prepare_weight_mx(codes, scales, q) for q in (W4A4_MXFP4, W4A16_MXFP4, W4A8_MXFP8)]
    for x, q in zip(ws, (W4A4_MXFP4, W4A16_MXFP4, W4A8_MXFP8)):
        assert x.B.data_ptr() == codes.data_ptr() and x.q == q and (x.N, x.K) == (64, 128) and x.scale_out_of_range == 0
        assert torch.equal(x.scale_b, ws[0].scale_b)
    ref_w = moe.prepare_weight(w, W4A16_MXFP4)  # the quantising path arrives at the same operands
    assert torch.equal(ref_w.B, ws[1].B) and torch.equal(ref_w.scale_b, ws[1].scale_b)
    scales2 = scales.clone()
    scales2[0, 0], scales2[5, 3], scales2[6, 1] = 90, 150, 104
    with pytest.warns(UserWarning, match="2 of"):
        assert moe.prepare_weight_mx(codes, scales2, W4A16_MXFP4).scale_out_of_range == 2
    with pytest.raises(ValueError):
        moe.prepare_weight_mx(codes, scales, FP16)
    with pytest.raises(ValueError):
        moe.prepare_weight_mx(codes, scales[:, :3], W4A16_MXFP4)
    # a layer built from prepared weights keeps them and runs the plain layout
    layer = moe.MoEFFN([ws[1]] * 2, [moe.prepare_weight_mx(*quant_mxfp4(w[:, :64].t().contiguous().repeat(2, 1)[:128]), W4A16_MXFP4)] * 2,
                       [(W4A16_MXFP4, W4A16_MXFP4)] * 2, num_routed=2)
    assert layer.w1[0] is ws[1] and not layer.fuse_silu and (layer.N, layer.H) == (32, 128)
    with pytest.raises(ValueError):
        moe.MoEFFN([ws[0]] * 2, [ws[0]] * 2, [(W4A16_MXFP4, W4A16_MXFP4)] * 2, num_routed=2)  # qcfg mismatch


# ------------------------------------------------------------------ the C entry points' validation

A16 = 4096  # a fake, 16-byte aligned, never dereferenced address (T > 0 checks stop before any HIP call)


def test_abi_validation_without_gpu():
    lib = nat.lib()
    INV = nat.MXMOE_GG_ERR_INVALID
    glu = nat.MoeGluC(nat.GLU_SILU, 0.0, 0.0, None, None)
    call = lambda g, N=128, mask=1: lib.mxmoe_moe_glu_quant(ctypes.byref(g) if g is not None else None, None, None, 4, 2, N, 0,
                                                            None, None, 1, mask, None, None, None)
    assert call(None) == INV and b"glu->act" in lib.mxmoe_gg_last_error()
    assert call(nat.MoeGluC(2, 1.702, 7.0, None, None)) == INV and b"glu->act" in lib.mxmoe_gg_last_error()
    for limit in (0.0, -7.0, float("inf"), float("nan")):
        assert call(nat.MoeGluC(nat.GLU_SWIGLU_CLAMP, 1.702, limit, None, None)) == INV
        assert b"limit" in lib.mxmoe_gg_last_error()
    assert call(nat.MoeGluC(nat.GLU_SWIGLU_CLAMP, float("nan"), 7.0, None, None)) == INV
    assert call(nat.MoeGluC(nat.GLU_SILU, 0.0, 0.0, A16 + 8, None)) == INV and b"misaligned bias" in lib.mxmoe_gg_last_error()
    assert call(nat.MoeGluC(nat.GLU_SILU, 0.0, 0.0, None, A16 + 2)) == INV and b"misaligned bias" in lib.mxmoe_gg_last_error()
    assert call(glu, mask=1 << 5) == nat.MXMOE_GG_ERR_UNSUPPORTED
    assert call(glu, N=100) == INV and b"multiples of 128" in lib.mxmoe_gg_last_error()
    assert call(glu) == INV and b"NULL or misaligned" in lib.mxmoe_gg_last_error()
    assert lib.mxmoe_moe_glu_quant(ctypes.byref(glu), None, None, 0, 2, 128, 0, None, None, 1, 1, None, None, None) == 0  # T = 0
    assert ctypes.sizeof(nat.MoeGluC) == 32

    cb = lib.mxmoe_moe_combine_bias
    assert cb(None, None, None, None, None, None, None, None, 4, 2, 8, 12, None, None) == INV
    assert b"H % 8" in lib.mxmoe_gg_last_error()
    assert cb(None, None, None, None, None, None, None, None, 4, 2, 0, 16, None, None) == INV  # E < 1
    assert cb(None, None, None, None, A16 + 8, None, None, None, 4, 2, 8, 16, None, None) == INV
    assert b"misaligned bias" in lib.mxmoe_gg_last_error()
    assert cb(None, None, None, None, None, None, None, A16, 4, 2, 8, 16, None, None) == INV  # shared_bias without shared
    assert cb(A16, A16, None, A16, A16, None, None, None, 4, 2, 8, 16, A16, None) == INV  # a bias needs sorted_expert
    assert b"NULL or misaligned" in lib.mxmoe_gg_last_error()
    assert cb(None, None, None, None, None, None, None, None, 0, 2, 8, 16, None, None) == 0  # T = 0

    def gate2(logit_bias=None, scoring=0, T=0, E=32):
        return lib.mxmoe_moe_gate_ex2(None, None, None, T, 64, E, 4, 1, scoring, None, 1, 1, 1, 1.0, logit_bias, None, None,
                                      None, None, None, None)
    assert gate2() == 0 and gate2(A16) == 0  # T = 0: nothing to do
    assert gate2(A16 + 2) == INV and b"logit_bias" in lib.mxmoe_gg_last_error()
    assert gate2(A16, scoring=2) == INV
    assert gate2(A16, E=300) == INV and b"mxmoe_moe_gate_ex2" in lib.mxmoe_gg_last_error()
    assert gate2(A16, T=4) == INV and b"NULL pointer" in lib.mxmoe_gg_last_error()


def test_symbols_are_listed_and_a_library_without_them_is_refused(monkeypatch):
    for fn in ("mxmoe_moe_gate_ex2", "mxmoe_moe_glu_quant", "mxmoe_moe_combine_bias"):
        assert fn in nat.EXPORTED_SYMBOLS and hasattr(nat.lib(), fn)
    assert nat.ABI_VERSION == 7
    monkeypatch.delenv("MXMOE_GG_LIB", raising=False)
    with pytest.raises(nat.NativeLibraryError, match="stale build"):
        nat._check_symbols(SimpleNamespace(mxmoe_moe_gate_ex2=1), nat.LIB_PATH)
    nat._check_symbols(nat.lib(), nat.LIB_PATH)
    monkeypatch.setenv("MXMOE_GG_LIB", "/elsewhere/libmxmoe_gg_old.so")
    nat._check_symbols(SimpleNamespace(), nat.LIB_PATH)  # an A/B tool's older build may lack them ...
    monkeypatch.setattr(nat, "_lib", SimpleNamespace())
    with pytest.raises(nat.NativeLibraryError):  # ... and a call then says so
        nat.symbol("mxmoe_moe_glu_quant")


# ------------------------------------------------------------------ MoEFFN's rules

def _tiny_layer(**kw):
    g = torch.Generator().manual_seed(7)
    E, H, N = 4, 128, 128
    mk = lambda n, k: ((torch.rand(n, k, generator=g) * 2 - 1) * 0.2).half()
    q = kw.pop("q", W4A4_MXFP4)
    return moe.MoEFFN([mk(2 * N, H) for _ in range(E)], [mk(H, N) for _ in range(E)], [(q, q)] * E, num_routed=E, **kw), E, H, N


def test_moeffn_rules():
    E, H, N = 4, 128, 128
    b1 = [torch.full((2 * N,), 0.25) for _ in range(E)]
    b2 = [torch.full((H,), -0.5) for _ in range(E)]
    plain, *_ = _tiny_layer(q=W4A16_MXFP4)
    assert plain.fuse_silu and not plain.biased_or_gated and plain.activation == "silu"  # today's default: unchanged
    for kw in (dict(gate_up_bias=b1), dict(down_bias=b2), dict(activation=moe.SwigluClamp())):
        layer, *_ = _tiny_layer(q=W4A16_MXFP4, **kw)
        assert layer.biased_or_gated and not layer.fuse_silu
        with pytest.raises(ValueError, match="plain gate_up layout"):
            _tiny_layer(q=W4A16_MXFP4, fuse_silu=True, **kw)
    with pytest.raises(ValueError):
        _tiny_layer(activation="gelu")
    with pytest.raises(ValueError):
        moe.SwigluClamp(limit=0.0)
    with pytest.raises(ValueError):
        moe.SwigluClamp(alpha=float("inf"))
    with pytest.raises(ValueError, match="one row per expert"):
        _tiny_layer(gate_up_bias=b1[:3])
    with pytest.raises(ValueError):
        _tiny_layer(gate_up_bias=[torch.zeros(N)] * E)
    with pytest.raises(ValueError, match="finite"):
        _tiny_layer(down_bias=[torch.full((H,), 1e6)] * E)  # inf as fp16
    layer, *_ = _tiny_layer(gate_up_bias=b1, down_bias=b2, activation=moe.SwigluClamp(1.5, 6.0))
    assert layer.b1.dtype == torch.float16 and tuple(layer.b1.shape) == (E, 2 * N) and tuple(layer.b2.shape) == (E, H)
    for v, name in ((layer.a16_view(), "w4a16_g32_sym_MXFP4"), (layer.a8_view(), "w4a8_g32_sym_MXFP8"),
                    (layer.a16_view().a8_view(), "w4a8_g32_sym_MXFP8")):
        assert v.qcfg[0][0].qcfg == name and v.activation == moe.SwigluClamp(1.5, 6.0) and not v.fuse_silu
        assert v.b1 is layer.b1 and v.b2 is layer.b2 and v.biased_or_gated
        assert v.w1[0].B.data_ptr() == layer.w1[0].B.data_ptr()
    blk = moe.MoEBlock(layer, torch.zeros(E, H, dtype=torch.float16), 2, renormalize=True, logit_bias=torch.zeros(E))
    assert blk.routing["logit_bias"] is not None
    assert "logit_bias" not in moe.MoEBlock(layer, torch.zeros(E, H, dtype=torch.float16), 2).routing
    with pytest.raises(ValueError, match="logit_bias"):
        moe.MoEBlock(layer, torch.zeros(E, H, dtype=torch.float16), 2, logit_bias=torch.zeros(E + 1))
    with pytest.raises(ValueError, match="logit_bias"):
        moe.MoEBlock(layer, torch.zeros(E, H, dtype=torch.float16), 2, logit_bias=torch.zeros(E, dtype=torch.float16))
