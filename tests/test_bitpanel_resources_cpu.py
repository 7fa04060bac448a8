"""Build-time guard (no GPU) on the mid-batch kernel (csrc/bitpanel.hip): every one of its 7 widths x 3 row-tile counts x 2 ingests keeps its
register arrays in registers -- no spill, no scratch (a `break` in an unrolled loop or stores under a per-kind branch
would move them to memory) -- and fits the 160 KiB of LDS of a CU with the dynamic part its geometry asks for."""
import ctypes as C
import re

import pytest

from kernel_resources import resources
from qllm_amd import _lib

LDS_PER_CU = 160 * 1024
ROWS_OF = {2: 17, 4: 64, 8: 128}   # a row count served by each row-tile count


def _instantiations():
    res = {}
    for name, r in resources("bitpanel.hip").items():
        got = re.search(r"bitpanel_kernelILi(\d+)ELi(\d+)ELb([01])E", name)   # <BITS, MT, LDSW>
        if got:
            res[(int(got.group(1)), int(got.group(2)), int(got.group(3)))] = r
    return res


def test_every_width_and_row_tile_count_is_built():
    assert sorted(_instantiations()) == [(b, mt, ldsw) for b in range(2, 9) for mt in (2, 4, 8) for ldsw in (0, 1)]


@pytest.mark.parametrize("bits", range(2, 9))
def test_no_spill_no_scratch_and_the_lds_fits(bits):
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    lib = _lib.load()
    for mt in (2, 4, 8):
        # the row tiles the geometry function gives
        w = _lib.QllmWeight(4096, 8192, None, None, None, 4096, 4096, 128, bits, _lib.LAYOUT_GPTQ, 0)
        buf = C.create_string_buffer(256)
        assert lib.qllm_bitpanel_describe(C.byref(w), ROWS_OF[mt], 1, buf, 256) == 0
        tiles = int(re.search(r"row_tiles=(\d+)", buf.value.decode()).group(1))
        assert tiles == mt, buf.value
        for ldsw in (0, 1):
            r = _instantiations()[(bits, mt, ldsw)]
            assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (bits, mt, ldsw, r)
            assert r["vgpr_count"] <= 512, (bits, mt, ldsw, r)   # 256 threads: one wave per SIMD may use the whole file
            # the dynamic part: two x tiles of 8 k-steps, [k-pair][row tile][16 rows][128 B]; the LDS ingest adds two tiles of word
            # rows, [8 bits rows][64 columns] dwords
            dynamic = 2 * 4 * tiles * 2048 + ldsw * 2 * 8 * bits * 256
            assert r["group_segment_fixed_size"] + dynamic <= LDS_PER_CU, (bits, mt, ldsw, r["group_segment_fixed_size"], dynamic)
