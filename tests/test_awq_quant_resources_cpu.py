"""Build-time guard on csrc/awq_quant.hip (no GPU needed: hipcc cross-compiles gfx950 to assembly and the resource usage is read from
the code-object metadata only).  The design: 16 lanes own a row and hold g/16 columns of the current group; the clip search keeps the
candidates' quantization errors and their travelling copy in registers (nothing in private memory) and shares exactly one g x g fp32
Gram tile per block -- 64 KB at g = 128, two thread blocks per CU within the 160 KB of LDS and, at two waves per SIMD, 256 registers."""
import re

import pytest

from kernel_resources import resources


@pytest.fixture(scope="module")
def kernels():
    return resources("awq_quant.hip")


def _by_group(kernels, which):
    """{columns per lane: [resources of the fp16, bf16 and fp32 instantiation]} of one kernel template."""
    out = {}
    for n, r in kernels.items():
        m = re.search(which + r"I(.+)Li(\d)EEEv", n)
        if m:
            out.setdefault(int(m.group(2)), []).append((n, r))
    return out


@pytest.mark.parametrize("which", ["awq_clip_kernel", "awq_quant_kernel"])
def test_three_weight_dtypes_per_group_size_without_scratch(kernels, which):
    res = _by_group(kernels, which)
    assert sorted(res) == [2, 4, 8], sorted(kernels)                     # g = 32, 64, 128
    for cpl, insts in res.items():
        assert len(insts) == 3, insts                                     # fp16, bf16, fp32
        for n, r in insts:
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
            assert r["vgpr_count"] <= 256, (n, r)                          # two 256-thread blocks per CU: two waves per SIMD
            g = 16 * cpl
            want = g * g * 4 if which == "awq_clip_kernel" else g * 16 * 4  # the Gram tile / the codes on their way out
            assert r["group_segment_fixed_size"] == want, (n, r)
            assert r["group_segment_fixed_size"] * 2 <= 160 * 1024
