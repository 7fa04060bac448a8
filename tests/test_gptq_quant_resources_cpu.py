"""Build-time guard on csrc/gptq_quant.hip (no GPU needed: hipcc cross-compiles gfx950 to assembly and the resource usage is read from
the code-object metadata only).  The kernel's design: a row tile's 8 columns per lane, their codes, dequantized values and errors stay
in registers through the walk of a 128-column block (nothing in private memory), and the block shares exactly one 128 x 128 fp32 tile of
U (64 KB) plus one 16 x (128 + 4) fp32 tile (8.25 KB: the error history of an earlier block, rows padded against bank conflicts, then
the codes on their way out) -- two thread blocks per CU within the 160 KB of LDS."""
import pytest

from kernel_resources import resources


@pytest.fixture(scope="module")
def kernels():
    return resources("gptq_quant.hip")


def test_one_kernel_per_weight_dtype_without_scratch(kernels):
    res = {n: v for n, v in kernels.items() if "gptq_quant_kernel" in n}
    assert len(res) == 3, sorted(res)                       # fp16, bf16, fp32
    for n, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["group_segment_fixed_size"] == 128 * 128 * 4 + 16 * 132 * 4, (n, r)       # 73984 bytes <= 160 KB / 2
        assert r["group_segment_fixed_size"] * 2 <= 160 * 1024
        # 512 registers per SIMD lane: a 256-thread block is one wave per SIMD; two blocks per CU (the LDS limit) need <= 256
        assert r["vgpr_count"] <= 256, (n, r)
