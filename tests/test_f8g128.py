"""CPU tests of w8a8_g128_sym_E4M3 (block-scaled FP8): the quantisers against the independent restatement
(tests/_f8g128_ref.py), the contract's f32 fold against the f64 GEMM, and that the GPU test's exact family is exact."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from mxmoe_amd.groupgemm import SUPPORTED, W8A8_G128_E4M3, QParams
from mxmoe_amd.quantize import quant_e4m3_g128, quant_weight_e4m3_g128
from tests import _f8g128_ref as ref
from tests._util import assert_f16_close

SHAPES = [(17, 200, 384), (129, 384, 1152)]  # the GPU test's corner shapes


def _special_groups() -> np.ndarray:
    """[6, 256] fp16: each row one special group beside a random finite one."""
    rng = np.random.default_rng(3)
    x = rng.standard_normal((6, 256)).astype(np.float16)
    x[0, :128] = 0                                            # all zero (with a -0)
    x[0, 5] = -0.0
    x[1, :128] = 0
    x[1, 77] = 65504                                          # a single 65504
    x[2, :128] = np.tile(np.float16([448, 27, 29, 0.4375 + 2.0 ** -6, 1.0625, -1.1875, 2.0 ** -10, 3 * 2.0 ** -10]), 16)  # ties
    x[3, :128] = (rng.integers(-1023, 1024, 128) * 2.0 ** -24).astype(np.float16)  # fp16 subnormals
    x[4, 137] = np.inf                                        # an Inf group beside a finite one
    x[5, 130] = np.nan
    return x


@pytest.mark.parametrize("x", [np.random.default_rng(1).standard_normal((9, 384)).astype(np.float16) * 3, _special_groups()],
                         ids=["random", "special"])
def test_quant_e4m3_g128_matches_restatement(x):
    codes, sc = quant_e4m3_g128(torch.from_numpy(x))
    rcodes, rsc = ref.quant(x)
    assert (codes.numpy() == rcodes).all()
    assert np.array_equal(sc.numpy(), rsc, equal_nan=True)


def test_weight_quantiser_block_scales_partial_block():
    w = (np.random.default_rng(2).standard_normal((200, 256)) * 0.1).astype(np.float16)
    w[128:, 128:] = 0  # an all-zero (partial) block
    codes, sc = quant_weight_e4m3_g128(torch.from_numpy(w))
    assert codes.shape == (200, 256) and sc.shape == (2, 2) and sc.dtype == torch.float32
    assert (sc.numpy() == ref.weight_scales(w)).all() and sc[1, 1] == 1
    back = ref.e4m3(codes.numpy()) * np.repeat(np.repeat(sc.numpy().astype(np.float64), 128, 0)[:200], 128, 1)
    assert np.abs(back - w).max() <= np.abs(w).max() / 16  # 3 mantissa bits: half an ulp of the block's amax


@pytest.mark.parametrize("M,N,K", SHAPES)
def test_f32_fold_within_fp16_tolerance_and_exact_family_is_exact(M, N, K):
    ops = ref.operands(M, N, K, False, 5)
    assert_f16_close(ref.gemm_fold_f32(*ops), ref.gemm(*ops), K)
    ops = ref.operands(M, N, K, True, 6)
    c = ref.gemm(*ops)
    assert (c.astype(np.float32).astype(np.float64) == c).all() and np.abs(c).max() < 2.0 ** 15  # exact in f32, finite in fp16
    assert (ref.gemm_fold_f32(*ops).view(np.uint16) == c.astype(np.float16).view(np.uint16)).all()
    for g in range(1, K // 128):  # every partial fold too: 22 bits at the most
        part = ref.gemm(ops[0][:, :g * 128], ops[1][:, :g], ops[2][:, :g * 128], ops[3][:, :g])
        assert (part.astype(np.float32).astype(np.float64) == part).all()


def test_qparams_round_trip():
    assert W8A8_G128_E4M3.qcfg == "w8a8_g128_sym_E4M3" and SUPPORTED[W8A8_G128_E4M3.qcfg] is W8A8_G128_E4M3
    assert QParams.from_qcfg("w8a8_g128_sym_E4M3") == QParams(8, 8, 128, True, "E4M3")


def test_prepare_weight_e4m3_g128_gate_up_pairs():
    from mxmoe_amd import moe
    mk = lambda n: (torch.zeros(n, 256, dtype=torch.uint8), torch.ones((n + 127) // 128, 2))  # noqa: E731
    (g, sg), (u, su) = mk(128), mk(128)
    w = moe.prepare_weight_e4m3_g128((g, u), (sg, su))
    assert (w.N, w.K, w.q) == (256, 256, W8A8_G128_E4M3) and tuple(w.scale_b.shape) == (2, 2)
    (g, sg), (u, su) = mk(192), mk(192)
    with pytest.raises(ValueError, match="inter % 128"):
        moe.prepare_weight_e4m3_g128((g, u), (sg, su))
    assert moe.act_tag(W8A8_G128_E4M3) == moe.ACT_E4M3_G128 == 10


def test_new_unit_codegen():
    """gg_f8g128.hip's two kernels (outside tests/test_codegen.py's unit): no scratch, at most 256 VGPRs, no packed f32."""
    import re
    import subprocess
    import tempfile
    from mxmoe_amd import build as b
    src = next(s for s in b.SOURCES if s.name == "gg_f8g128.hip")
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([b.HIPCC, "-O3", "-std=c++17", f"--offload-arch={b.ARCH}", "--cuda-device-only", "-S", "-o", f"{d}/k.s",
                        "-I", str(b.ROOT / "include"), *b.SOURCE_FLAGS[src.name], str(src)], check=True, capture_output=True)
        asm = open(f"{d}/k.s").read()
    assert len(re.findall(r"\.amdhsa_kernel ", asm)) == 2 and not re.search(r"v_pk_(add|mul|fma)_f32", asm)
    assert set(re.findall(r"; ScratchSize: (\d+)", asm)) == {"0"}
    assert all(int(v) <= 256 for v in re.findall(r"; NumVgprs: (\d+)", asm))
