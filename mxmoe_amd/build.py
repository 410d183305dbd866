"""Build libmxmoe_gg.so in-tree with hipcc for gfx950 (no JIT cache: the .so travels with the repo)."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

PKG = Path(__file__).resolve().parent
ROOT = PKG.parent
CSRC = PKG / "csrc"
LIB = PKG / "lib" / "libmxmoe_gg.so"
# tools-only lab library: the v2 family with the timing ablations and mainloop experiments
# (-DMXMOE_LAB; tools/kbench.py with MXMOE_GG_LIB=<this>). Never loaded by the product.
LAB_LIB = PKG / "lib" / "libmxmoe_gg_lab.so"
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("MXMOE_OFFLOAD_ARCH", "gfx950")

# gg_api.hip stays first (tests/test_codegen.py compiles SOURCES[0] for the device ISA); gg_plan.cpp is the
# host-only tile planner, compiled by the same hipcc and flags as the rest
SOURCES = [CSRC / "gg_api.hip", CSRC / "moe_ops.hip", CSRC / "gg_plan.cpp"]

FLAGS = ["-O3", "-std=c++17", "-fPIC", "-shared", f"--offload-arch={ARCH}", "-Wall", "-Wno-unused-function",
         "-I", str(ROOT / "include")]


def _deps() -> list[Path]:
    """What every object, and so every library, is built from: all of csrc/ and the public headers."""
    return sorted(p for p in CSRC.iterdir() if p.is_file()) + sorted((ROOT / "include").glob("*.h"))


def _newer(deps: list[Path], target: Path) -> bool:
    return not target.exists() or any(p.stat().st_mtime > target.stat().st_mtime for p in deps)


def needs_build(lib: Path = LIB) -> bool:
    """True when `lib` is missing or older than any source it is built from (the lab library's
    tests skip on a stale lab build: a binary HEAD does not produce must not pass for HEAD's)."""
    return _newer(_deps(), lib)


def build(force: bool = False, verbose: bool = False, extra: list[str] | None = None, lab: bool = False,
          lab_fast: bool = False) -> Path:
    """Compile each source to an object of its own (lib/obj/<product|lab|lab_fast>/, all at once, one hipcc
    per source; an object is kept while it is newer than its source and every header), then link.
    lab_fast: the lab library with only the experiments under test (-DMXMOE_LAB_FAST; gg_api.hip)."""
    lab = lab or lab_fast
    out = LAB_LIB if lab else LIB
    if not force and not needs_build(out):
        return out
    objdir = out.parent / "obj" / ("lab_fast" if lab_fast else "lab" if lab else "product")
    objdir.mkdir(parents=True, exist_ok=True)
    objs = [objdir / (src.stem + ".o") for src in SOURCES]
    defs = (["-DMXMOE_LAB"] if lab else []) + (["-DMXMOE_LAB_FAST"] if lab_fast else [])
    compile_flags = [f for f in FLAGS if f != "-shared"] + defs + list(extra or [])
    headers = [p for p in _deps() if p not in SOURCES]
    running = []
    for src, obj in zip(SOURCES, objs):
        if not force and not _newer([src, *headers], obj):
            continue
        cmd = [HIPCC, *compile_flags, "-c", "-o", str(obj), str(src)]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        running.append((cmd, subprocess.Popen(cmd)))
    failed = [cmd for cmd, proc in running if proc.wait() != 0]  # (every compile is waited for before any error)
    if failed:
        raise subprocess.CalledProcessError(1, failed[0])
    tmp = out.with_suffix(".so.tmp")
    cmd = [HIPCC, *FLAGS, *defs, *(extra or []), "-o", str(tmp), *map(str, objs)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    os.replace(tmp, out)
    return out


REF_HARNESS_SRC = [ROOT / "tests" / "cpp" / "ref_harness_call.cpp", ROOT / "tests" / "cpp" / "layout_check.cpp"]
# built beside the library it links, not under tests/: a build product in the test tree goes missing
# whenever that tree is replaced (another revision's tests run against this build)
REF_HARNESS = LIB.parent / "ref_harness_call"


def build_ref_harness(force: bool = False, verbose: bool = False) -> Path:
    """The reference-side C++ caller of groupgemm_mxmoe (tests/cpp): test
    infrastructure, linked against the product library (rpath to mxmoe_amd/lib)."""
    deps = REF_HARNESS_SRC + [ROOT / "include" / "mxmoe_gg.h", LIB]
    if not force and REF_HARNESS.exists() and all(p.stat().st_mtime <= REF_HARNESS.stat().st_mtime for p in deps):
        return REF_HARNESS
    REF_HARNESS.parent.mkdir(parents=True, exist_ok=True)
    cmd = [HIPCC, "-O2", "-std=c++17", f"--offload-arch={ARCH}", "-Wall", "-I", str(ROOT / "include"),
           "-o", str(REF_HARNESS), *map(str, REF_HARNESS_SRC), "-L", str(LIB.parent), "-lmxmoe_gg",
           "-Wl,-rpath,$ORIGIN"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True)
    return REF_HARNESS


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True, lab="--lab" in sys.argv, lab_fast="--lab-fast" in sys.argv))
