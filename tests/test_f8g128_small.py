"""w8a8_g128_sym_E4M3 on the small-batch kernel (wo3), host side: AUTO, a forced mixed call, the new unit's resources."""
from __future__ import annotations

import ctypes
import re
import subprocess

from mxmoe_amd import _native as nat
from mxmoe_amd import build as b
from mxmoe_amd.workload import load_workload, qwen2_layer11_workload

F8G = dict(a_bits=8, w_bits=8, gsize=128, sym=1, fmt=nat.FMT_E4M3)
F16 = dict(a_bits=16, w_bits=16, scale_a=0, scale_b=0)


def _prob(**kw):
    d = dict(A=16, B=16, scale_a=16, scale_b=16, C=16, M=64, N=128, K=256)
    d.update(kw)
    return nat.GGProblemC(**d)


def _wo3() -> int:
    return [ln.split()[1] for ln in nat.list_variants()].index("wo3_64x256_w8_3wg")


def _auto(ps) -> int:
    return nat.resolve_variant((nat.GGProblemC * len(ps))(*ps), len(ps))


def test_auto_takes_wo3_for_small_calls_of_the_type_alone():
    wo3, dflt = _wo3(), nat.default_variant()
    for gg in ("gate_up", "down"):
        small, big = ([_prob(M=s.M, N=s.N, K=s.K, **F8G) for s in load_workload(qwen2_layer11_workload(bs))["layer-11"][gg]]
                      for bs in (128, 8192))
        assert _auto(small) == wo3 and _auto(big) == dflt, gg
        assert _auto(small + [_prob(M=8, N=256, K=small[0].K, **F16)]) == dflt, gg  # no mixed wo3 build
        assert _auto(small + [_prob(M=0, **F16)]) == wo3, gg                        # an empty fp16 problem does not count
        # ... an empty w4a4 MXFP4 one does (auto_counts_empty: only v2x plans that type)
        assert _auto(small + [_prob(M=0, a_bits=4, w_bits=4, gsize=32, sym=1, fmt=nat.FMT_MXFP4)]) == dflt, gg


def test_forced_wo3_refuses_the_type_beside_another():
    ps = [_prob(**F8G), _prob(**F16)]
    arr, info = (nat.GGProblemC * 2)(*ps), nat.GGPlanInfo()
    st = nat.lib().mxmoe_gg_plan(arr, 2, _wo3(), None, 1 << 20, None, ctypes.byref(info))
    assert st == nat.MXMOE_GG_ERR_UNSUPPORTED
    assert "problem 0: variant wo3_64x256_w8_3wg does not implement" in nat.lib().mxmoe_gg_last_error().decode()


def test_small_unit_codegen(tmp_path):
    """gg_f8g128_small.hip: one kernel, no scratch, at most 80 VGPRs and the 52-KiB image (three workgroups per CU)."""
    src = next(s for s in b.SOURCES if s.name == "gg_f8g128_small.hip")
    subprocess.run([b.HIPCC, "-O3", "-std=c++17", f"--offload-arch={b.ARCH}", "--cuda-device-only", "-S", "-o", str(tmp_path / "k.s"),
                    "-I", str(b.ROOT / "include"), *b.SOURCE_FLAGS[src.name], str(src)], check=True, capture_output=True)
    asm = (tmp_path / "k.s").read_text()
    assert len(re.findall(r"\.amdhsa_kernel ", asm)) == 1
    assert re.findall(r"; ScratchSize: (\d+)", asm) == ["0"]
    assert int(re.search(r"; NumVgprs: (\d+)", asm).group(1)) <= 80
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", asm).group(1)) <= 53248
