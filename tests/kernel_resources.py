"""What the *_resources_cpu tests read of a kernel source: its gfx950 assembly and the per-kernel resource usage, through the reader
tools/kernel_resources.py uses (tools/kernel_asm.py: one compile per source and session).  The tests skip where hipcc is absent."""
import functools
import os

import pytest

from tools import kernel_asm
from tools.kernel_asm import parse  # noqa: F401  (for the tests that parse the text themselves)


def asm_text(src):
    """The gfx950 assembly of csrc/<src>."""
    if not os.path.exists(kernel_asm.HIPCC):
        pytest.skip("hipcc not available")
    return kernel_asm.asm_text(src)


@functools.lru_cache(maxsize=None)
def resources(src):
    """{kernel name: {vgpr_count, vgpr_spill_count, sgpr_spill_count, private_segment_fixed_size, group_segment_fixed_size}} of
    csrc/<src>."""
    return parse(asm_text(src))
