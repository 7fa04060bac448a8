"""The preloading twins of the batch-1 kernel (csrc/strip1_pre.hip) as the compiler built them, no GPU needed: the unit is compiled
device-only to assembly with the flags the Makefile gives this unit, and every twin must have its leading arguments in user SGPRs
(a non-zero .amdhsa_user_sgpr_kernarg_preload_length inside the 16 user SGPRs), no scratch, no spills, the registers of its plain
twin's launch bound, dynamic LDS only -- and the set of twins must be the table: every (waves, round) pair of strip1_forms.hpp in its
exact and its shifted-window form, plus the two diagnostics forms."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_asm  # noqa: E402

UNIT = "strip1_pre.hip"
NAME = re.compile(r"^_ZN4qllm17strip1_kernel_preILi(\d+)ELi(\d+)ELb([01])ELb([01])EEEvPKvijPKjS2_S2_S2_PvNS_12Strip1ParamsE$")


def unit_flags():
    """What the Makefile adds to CXXFLAGS for this unit, and for this unit only."""
    with open(os.path.join(kernel_asm.CSRC, "Makefile")) as f:
        mk = f.read()
    rules = re.findall(r"^(.*):\s*CXXFLAGS\s*\+=\s*(.+)$", mk, re.M)
    assert len(rules) == 1, rules
    targets, flags = rules[0]
    assert targets.split() == ["build/strip1_pre.o", "build_$(NAME)/strip1_pre.o"]
    assert "-amdgpu-kernarg-preload-count=8" in flags.split()
    assert "strip1_pre.hip" in re.search(r"^SRCS\s*:=\s*(.+)$", mk, re.M).group(1).split()
    return flags.split()


@pytest.fixture(scope="module")
def asm(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pre") / "strip1_pre.s")
    subprocess.run([kernel_asm.HIPCC, *kernel_asm.FLAGS, *unit_flags(), os.path.join(kernel_asm.CSRC, UNIT), "-o", out], check=True, capture_output=True)
    with open(out) as f:
        return f.read()


def descriptors(text):
    """{kernel: {directive: int}} from the .amdhsa_kernel blocks."""
    res = {}
    for name, body in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.M | re.S):
        res[name] = {k: int(v, 0) for k, v in re.findall(r"^\s*\.amdhsa_(\w+)\s+(\d+)\s*$", body, re.M)}
    return res


def pair_table():
    with open(os.path.join(kernel_asm.CSRC, "strip1_forms.hpp")) as f:
        return sorted((int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", f.read()))


def test_the_twins_are_the_table(asm):
    got = set()
    for n in descriptors(asm):
        m = NAME.match(n)
        assert m, n                                    # nothing else is built there, and the name is the one the benchmark's filter takes
        got.add(tuple(int(v) for v in m.groups()))
    pairs = pair_table()
    assert len(pairs) == 15 and {(8, 16), (4, 32), (15, 24)} <= set(pairs)
    want = {(nw, maxs, exact, 0) for nw, maxs in pairs for exact in (0, 1)} | {(8, 16, 1, 1), (15, 24, 0, 1)}
    assert got == want and len(got) == 32
    # the benchmark's counter pass selects dispatches by the demangled qllm::strip\d?_kernel: no _Float16 (DF16_) in the signature,
    # which profilers' demanglers leave mangled -- NAME above allows void, int, unsigned and Strip1Params only


def test_every_twin_is_preloaded_and_inside_its_budget(asm):
    desc, res = descriptors(asm), kernel_asm.parse(asm)
    assert sorted(desc) == sorted(res) and len(desc) == 32
    for n, d in sorted(desc.items()):
        nw, maxs, exact, dbg = (int(v) for v in NAME.match(n).groups())
        # eight leading arguments = 14 words, behind the 2 of the kernel-argument pointer
        assert d["user_sgpr_kernarg_preload_length"] == 14, (n, d["user_sgpr_kernarg_preload_length"])
        assert d["user_sgpr_kernarg_preload_length"] > 0 and d["user_sgpr_count"] <= 16, n
        r = res[n]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert d["private_segment_fixed_size"] == 0, n
        assert r["vgpr_count"] <= (64 if maxs <= 24 else 128), (n, r)    # the plain twin's launch bound (strip1_min_waves)
        assert r["group_segment_fixed_size"] == 0 and d["group_segment_fixed_size"] == 0, n   # dynamic LDS only


def test_problem_zero_blocks_load_nothing(asm):
    """Behind the compatibility prologue (the loads a driver without preload support runs, 256-byte aligned away from the entry the
    hardware uses) a non-diagnostics twin has exactly one batch of scalar loads, and it sits behind a scalar branch."""
    name = "_ZN4qllm17strip1_kernel_preILi8ELi16ELb1ELb0EEEvPKvijPKjS2_S2_S2_PvNS_12Strip1ParamsE"
    body = asm.split(name + ":")[1].split(".Lfunc_end")[0]
    entry = body.split(".p2align\t8")[1]
    lines = [l.split()[0] for l in entry.splitlines() if l.strip() and not l.lstrip().startswith((";", "."))]
    first_load = next(i for i, op in enumerate(lines) if op.startswith("s_load"))
    first_vmem = next(i for i, op in enumerate(lines) if op.startswith("global_load"))
    assert first_vmem < first_load                                          # the x chunk leaves before any scalar load
    assert any(op.startswith("s_cbranch") for op in lines[first_vmem:first_load])
    assert sum(op.startswith("s_load") for op in lines) == 2               # the 48-byte record: 8 + 4 words, one batch
