"""Codegen guards (CPU, hipcc cross-compile): no kernel may use scratch (private segment), and the
VGPR count must leave the occupancy the variant was designed for (cdna_hip_programming.md rule 20)."""
from __future__ import annotations

import re
import subprocess
from pathlib import Path

import pytest

from mxmoe_amd import build as b


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = tmp_path_factory.mktemp("asm") / "gg.s"
    cmd = [b.HIPCC, "-O3", "-std=c++17", f"--offload-arch={b.ARCH}", "--cuda-device-only", "-S", "-o", str(out),
           "-I", str(b.ROOT / "include"), str(b.SOURCES[0])]
    subprocess.run(cmd, check=True, capture_output=True)
    return out.read_text()


def _kernels(asm):
    ks = {}
    for m in re.finditer(r"\.private_segment_fixed_size: (\d+)\n\s+\.sgpr_count:\s+\d+\n\s+\.sgpr_spill_count: (\d+)\n"
                         r"\s+\.symbol:\s+(\S+)\.kd\n(?:.*\n){0,12}?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count: (\d+)",
                         asm):
        ks[m.group(3)] = dict(private=int(m.group(1)), sgpr_spill=int(m.group(2)), vgpr=int(m.group(4)),
                              vgpr_spill=int(m.group(5)))
    return ks


def test_no_scratch_no_spills(asm):
    ks = _kernels(asm)
    assert len(ks) >= 4
    for name, k in ks.items():
        m = re.match(r"_ZN5mxmoe12gg_v2_kernelILi(\d+)E", name)
        if m and int(m.group(1)) & 64:
            continue  # abl_v2s_trace (V2_TRACE = 64): a diagnostics build, its timestamps may cost a spill
        if "gg_v2_kernelILi0ELi127E" in name:  # every tile body incl. 2-bit weight-only (mixed calls only)
            assert k["private"] <= 16, (name, k)  # a prologue / epilogue spill, none inside a K loop
            continue
        assert k["private"] == 0 and k["vgpr_spill"] == 0 and k["sgpr_spill"] == 0, (name, k)


def test_product_kernel_set(asm):
    """The kernels the product library instantiates are exactly the committed list: a build-table change
    that adds, drops or re-parametrises a kernel shows here, before it costs build time or library size."""
    want = (Path(__file__).parent / "golden" / "product_kernels.txt").read_text().split()
    assert sorted(set(re.findall(r"\.symbol:\s+(\S+)\.kd", asm))) == want


def test_v2_keeps_two_waves_per_simd(asm):
    ks = _kernels(asm)
    v2 = [k for n, k in ks.items() if "gg_v2_kernel" in n]
    assert v2 and v2[0]["vgpr"] <= 256  # 8-wave workgroup = 2 waves/SIMD needs <= 256 VGPRs
