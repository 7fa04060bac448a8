"""Build-time guard on csrc/hqq_quant.hip (no GPU needed: hipcc cross-compiles gfx950 to assembly and the resource usage is read from
the code-object metadata).  A group lives in registers through every solver round: the per-lane element array must never end up in
private (scratch) memory -- a dynamically indexed register array, or a `break` inside an unrolled loop, would put it there -- and a
256-thread block must stay within the register file."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qllm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    out = str(tmp_path_factory.mktemp("hqq_res") / "hqq_quant.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                    os.path.join(CSRC, "hqq_quant.hip"), "-o", out], check=True, capture_output=True)
    return open(out).read()


def _kernels(text):
    res = {}
    for block in text.split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        vg = re.search(r"\.vgpr_count:\s+(\d+)", block)
        sp = re.search(r"\.vgpr_spill_count:\s+(\d+)", block)
        pr = re.search(r"\.private_segment_fixed_size:\s+(\d+)", block)
        lds = re.search(r"\.group_segment_fixed_size:\s+(\d+)", block)
        if name and vg and sp and pr and lds:
            res[name.group(1)] = tuple(int(m.group(1)) for m in (vg, sp, pr, lds))
    return res


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
