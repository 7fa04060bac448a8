"""The gfx950 assembly of a kernel source and the per-kernel resource usage in its code-object metadata (hipcc -S, no GPU needed):
what tools/kernel_resources.py prints and the *_resources_cpu tests assert on.  Every source is compiled once per process, into a
private directory removed at exit."""
import atexit
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qllm_amd", "csrc")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only"]
FIELDS = ("vgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


@functools.lru_cache(maxsize=None)
def _tmpdir():
    d = tempfile.mkdtemp(prefix="qllm_res_")
    atexit.register(shutil.rmtree, d, True)
    return d


@functools.lru_cache(maxsize=None)
def asm_text(src):
    """The gfx950 assembly of csrc/<src>."""
    out = os.path.join(_tmpdir(), src + ".s")
    subprocess.run([HIPCC, *FLAGS, os.path.join(CSRC, src), "-o", out], check=True, capture_output=True)
    with open(out) as f:
        return f.read()


_SCALAR_KEPT = re.compile(r"s_(waitcnt|barrier|setprio|sleep|endpgm|branch|cbranch)")


def vector_lines(text):
    """The lines of an assembly text that a change of scalar bookkeeping cannot move: scalar-ALU / scalar-memory lines are dropped
    (waits, barriers, priority, sleep, end and branches stay), scalar register numbers are masked (s12 -> sR, s[4:5] -> s[R]) and so
    is the per-build __hip_cuid_ symbol; lines that are only an assembler comment go too (code sizes, register totals, and the
    `; sched_barrier` marks, which stand for no instruction).  Vector, LDS, MFMA, memory, wait, barrier, priority and branch lines
    stay as they are, vector register numbers included: two builds of a kernel whose lists are equal differ in the scalar unit's
    work only."""
    out = []
    for line in text.splitlines():
        op = line.split()[0] if line.strip() else ""
        if "__hip_cuid_" in line or op.startswith(";") or (op.startswith("s_") and not _SCALAR_KEPT.match(op)):
            continue
        out.append(re.sub(r"\bs\[\d+:\d+\]", "s[R]", re.sub(r"\bs\d+\b", "sR", line)))
    return out


def parse(text, fields=FIELDS):
    """{kernel name: {field: int}} from the amdhsa.kernels metadata of an assembly text."""
    res = {}
    for block in text.split("amdhsa.kernels:")[1].split("\n  - ")[1:]:
        name = re.search(r"\.name:\s+(\S+)", block)
        found = {k: re.search(r"\.%s:\s+(\d+)" % k, block) for k in fields}
        if name and all(found.values()):
            res[name.group(1)] = {k: int(m.group(1)) for k, m in found.items()}
    return res
