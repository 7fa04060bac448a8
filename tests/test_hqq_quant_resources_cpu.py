"""Build-time guard on csrc/hqq_quant.hip (no GPU needed: hipcc cross-compiles gfx950 to assembly and the resource usage is read from
the code-object metadata).  A group lives in registers through every solver round: the per-lane element array must never end up in
private (scratch) memory -- a dynamically indexed register array, or a `break` inside an unrolled loop, would put it there -- and a
256-thread block must stay within the register file."""
import re

import pytest

from kernel_resources import asm_text, parse


@pytest.fixture(scope="module")
def asm():
    return asm_text("hqq_quant.hip")


def _kernels(text):
    return {n: (r["vgpr_count"], r["vgpr_spill_count"], r["private_segment_fixed_size"], r["group_segment_fixed_size"])
            for n, r in parse(text).items()}


def test_every_instantiation_is_built_and_uses_no_scratch(asm):
    res = {n: v for n, v in _kernels(asm).items() if "hqq_quant_kernel" in n}
    assert len(res) == 18   # {fp16, bf16, fp32} x {2, 4, 8, 16, 32, 64} elements per lane
    for e in (2, 4, 8, 16, 32, 64):
        assert sum(f"Li{e}EEEv" in n for n in res) == 3, e
    for n, (vgpr, spill, private, lds) in res.items():
        e = int(re.search(r"Li(\d+)EEEv", n).group(1))
        assert spill == 0 and private == 0, (n, vgpr, spill, private)
        assert vgpr <= 256, (n, vgpr)                     # 256-thread blocks: one wave per SIMD at the very least
        assert lds == 4 * 64 * 4 + e * 16 * 16, (n, lds)  # the error sums + the tile's codes, nothing else
    assert "scratch_load" not in asm and "scratch_store" not in asm
    assert all(int(v) == 0 for v in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", asm))


def test_the_common_group_sizes_keep_two_blocks_per_simd(asm):
    """g = 32, 64, 128 (2, 4, 8 elements per lane) are the sizes of every checkpoint the library serves: <= 64 registers."""
    for n, (vgpr, _, _, _) in _kernels(asm).items():
        m = re.search(r"hqq_quant_kernel.*Li(\d+)EEEv", n)
        if m and int(m.group(1)) <= 8:
            assert vgpr <= 64, (n, vgpr)
