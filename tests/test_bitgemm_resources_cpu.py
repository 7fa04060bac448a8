"""Build-time guard (no GPU) on the 2..8-bit prefill kernel (csrc/bitgemm.hip): each of its seven widths keeps its register arrays in
registers -- no spill, no scratch --, fits the register budget of its 768-thread block (twelve waves = three per SIMD: 512 / 3
registers per lane, allocated in steps of 8) and declares no static LDS (the opt-in to its 128 KB of dynamic LDS is refused next to
any: csrc/bitpanel.hip)."""
import re

import pytest

from kernel_resources import resources

LDS_PER_CU = 160 * 1024
DYNAMIC_LDS = (3 * 256 * 64 + 2 * 128 * 64) * 2   # A ring of three 256 x 64 tiles + two B stages of 128 x 64, fp16
VGPR_BUDGET = 512 // 3 // 8 * 8                   # 168


def _instantiations():
    res = {}
    for name, r in resources("bitgemm.hip").items():
        got = re.search(r"bitgemm_kernelILi(\d+)E", name)   # <BITS>
        if got:
            res[int(got.group(1))] = r
    return res


def test_every_width_is_built():
    assert sorted(_instantiations()) == list(range(2, 9))


@pytest.mark.parametrize("bits", range(2, 9))
def test_no_spill_no_scratch_no_static_lds_three_waves_per_simd(bits):
    r = _instantiations()[bits]
    assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (bits, r)
    assert r["group_segment_fixed_size"] == 0, (bits, r)
    assert r["vgpr_count"] <= VGPR_BUDGET, (bits, r)
    assert DYNAMIC_LDS == 128 * 1024 and DYNAMIC_LDS <= LDS_PER_CU
