"""Compare two device-assembly files kernel by kernel: resources, mnemonic histogram, instruction text.

hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -I include --cuda-device-only -S mxmoe_amd/csrc/moe_ops.hip -o new.s
(the same at the other commit -> old.s), then: python tools/isa_compare.py old.s new.s > isa_compare.txt

A kernel is matched by its mangled name, a template's cut behind its template arguments. Per kernel: the .amdhsa_*
resource lines below, the histogram of all mnemonics, and the instruction text without comments, labels and directives
(the function number of a branch target and the file-wide counter of a long branch's .Lpost_getpc label removed). Exit status 1 when a kernel has no partner or differs in resources
or histogram.
"""
import collections
import re
import sys

RESOURCES = ("next_free_vgpr", "next_free_sgpr", "accum_offset", "group_segment_fixed_size", "private_segment_fixed_size")


def kernels(path):
    src = open(path).read()
    out = {}
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)\.end_amdhsa_kernel", src, flags=re.M | re.S):
        sym, desc = m.group(1), m.group(2)
        start = src.index(f"\n{sym}:") + len(sym) + 2
        lines = [re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", re.sub(r"\.LBB\d+_", ".LBB_", ln.split(";")[0].strip())) for ln in
                 src[start:src.index(".Lfunc_end", start)].split("\n")]
        lines = [ln for ln in lines if ln and not ln.startswith(".") and not ln.endswith(":")]
        res = tuple(re.search(rf"\.amdhsa_{r} (\S+)", desc).group(1) for r in RESOURCES)
        name = sym[:sym.index("EEv")] if "EEv" in sym else sym  # (a template's parameter list dropped)
        assert name not in out, name
        out[name] = (res, collections.Counter(ln.split()[0] for ln in lines), lines)
    return out


old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
print(f"kernels: {len(old)} old, {len(new)} new; resources compared: {', '.join(RESOURCES)}")
groups = collections.defaultdict(list)
for name in sorted(set(old) | set(new)):
    if name not in old or name not in new:
        groups["WITHOUT A PARTNER" + (" (old only)" if name in old else " (new only)")].append(name)
        continue
    (r0, h0, t0), (r1, h1, t1) = old[name], new[name]
    if r0 != r1:
        groups["RESOURCES DIFFER"].append(f"{name}: {r0} -> {r1}")
    elif h0 != h1:
        groups["HISTOGRAM DIFFERS"].append(f"{name}: { {k: (h0[k], h1[k]) for k in set(h0) | set(h1) if h0[k] != h1[k]} }")
    elif t0 != t1:
        groups["same resources and histogram, text differs"].append(
            f"{name}: {sum(a != b for a, b in zip(t0, t1))} of {len(t1)} lines")
    else:
        groups["identical text"].append(name)
for title, names in sorted(groups.items()):
    print(f"\n== {title}: {len(names)}\n  " + "\n  ".join(names))
sys.exit(1 if any(t[0].isupper() for t in groups) else 0)
