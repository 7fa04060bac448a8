"""Build-time guard (no GPU) on the instantiations the Falcon-shaped routes reach: gemm3 with its half-wide last tile (the same k-loop for
every wave; the dead half leaves before the epilogue) and the batch-1 kernel's 64-wide-group forms at K % 128 == 64 (T = 142: 8 waves x 24; T = 34:
4 x 16, both non-EXACT) -- no spills, and the register counts that keep their occupancy."""
import re

import pytest

from kernel_resources import resources


def _resources(src):
    return {n: (r["vgpr_count"], r["vgpr_spill_count"]) for n, r in resources(src).items()}


def test_gemm3_with_the_tail_tile_keeps_three_waves_per_simd():
    res = {n: v for n, v in _resources("gemm3.hip").items() if "gemm3_kernel" in n}
    assert len(res) == 8
    for n, (vgpr, spill) in res.items():
        mw = int(re.search(r"gemm3_kernelILi\dELi(\d)E", n).group(1))
        # 8 matrix + 4 staging waves = 3 per SIMD: <= 168 registers; 4 + 4 = 2 per SIMD: <= 256
        assert spill == 0 and vgpr <= (168 if mw == 8 else 256), (n, vgpr, spill)


@pytest.mark.parametrize("nw,maxs", [(8, 24), (4, 16)])
def test_batch1_g64_forms_of_odd_k_do_not_spill(nw, maxs):
    res = _resources("strip1.hip")
    # strip1_kernel<NW, MAXS, EXACT = false, 2, 4, DBG = false, AR = false, G64 = true, MR = 1, B3 = false>
    name = f"_ZN4qllm13strip1_kernelILi{nw}ELi{maxs}ELb0ELi2ELi4ELb0ELb0ELb1ELi1ELb0EEEvNS_12Strip1ParamsE"
    assert name in res, sorted(n for n in res if "strip1_kernelILi%dELi%dE" % (nw, maxs) in n)
    vgpr, spill = res[name]
    assert spill == 0 and vgpr <= 128, (name, vgpr, spill)
