#!/usr/bin/env python3
"""Static resource table of every kernel in libqllm_mi355x (hipcc -S for gfx950, code-object metadata): VGPRs, spills, SGPRs,
static LDS, and the waves per SIMD the register allocation allows (512-entry file, granule 8: MI355X_MICROARCH.md).
Usage: python tools/kernel_resources.py > profiles/rNN_kernel_resources.md   (no GPU needed)"""
import os
import re
import subprocess

from kernel_asm import CSRC, asm_text, parse

FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "group_segment_fixed_size", "max_flat_workgroup_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return [o.replace("(anonymous namespace)::", "").replace("qllm::", "").split("(")[0].replace("void ", "") for o in out]


# every translation unit of the library (SRCS of the Makefile); those without a kernel add no row
srcs = re.search(r"^SRCS\s*:=\s*(.+)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
rows = []
for src in srcs:
    for name, r in parse(asm_text(src), FIELDS).items():
        vg = r["vgpr_count"]
        alloc = (vg + 7) // 8 * 8
        rows.append((src, name, vg, r["vgpr_spill_count"], r["sgpr_count"], r["group_segment_fixed_size"], r["max_flat_workgroup_size"],
                     min(8, 512 // max(alloc, 8))))
names = demangle([r[1] for r in rows])
print("# Static kernel resources (hipcc -O3 --offload-arch=gfx950, code-object metadata; `python tools/kernel_resources.py`)\n")
print("Dynamic LDS (strip: <= 156 KB, gemm2: 128 KB, gemm: 64-160 KB, skinny: per plan) is not in the static column.\n")
print("| file | kernel | VGPRs | spilled | SGPRs | static LDS B | max block | waves/SIMD by registers |")
print("|---|---|---|---|---|---|---|---|")
for (src, _, vg, sp, sg, lds, wg, occ), n in sorted(zip(rows, names), key=lambda t: (t[0][0], t[1])):
    print(f"| {src} | `{n}` | {vg} | {sp} | {sg} | {lds} | {wg} | {occ} |")
