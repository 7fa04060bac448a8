"""The fused families of the batch-1 decode kernel (csrc/strip1_swiglu.hip, strip1_norm.hip, strip1_resid.hip, strip1_swiglu_resid.hip)
as the resource tests of test_swiglu_cpu.py, test_rmsnorm_cpu.py and test_residual_cpu.py see them: per family which forms of
csrc/strip1_forms.hpp's table are expected, the second launch bound, and the plain twin of strip1.hip -- read from the compiler's report
of every instantiation -- plus what the sources have to say once."""
import os
import re

from kernel_resources import resources

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "qllm_amd", "csrc")
SHARED = "strip1_forms.hpp"
PLAIN = "strip1.hip"
# source -> (kernel, whether its template list has MR (<NW, MAXS, EXACT, G64, [MR,] B3, WAVES>), four-row forms, instantiations, its LDS behind strip1_lds_bytes)
FAMILIES = {"strip1_swiglu.hip": ("strip1_swiglu_kernel", True, True, 122, "kLdsExtra = 0,"),
            "strip1_norm.hip": ("strip1_norm_kernel", True, False, 100, "kLdsExtra = kStrip1NormLdsBytes,"),
            "strip1_resid.hip": ("strip1_resid_kernel", False, False, 100, "kLdsExtra = 0,"),
            "strip1_swiglu_resid.hip": ("strip1_swiglu_resid_kernel", False, False, 100, "kLdsExtra = 0,")}


def _text(src):
    with open(os.path.join(CSRC, src)) as f:
        return f.read()


def pair_table():
    """The (NW, MAXS) pairs of the one table under csrc/."""
    holders = [f for f in sorted(os.listdir(CSRC)) if os.path.isfile(os.path.join(CSRC, f)) and re.search(r"X\(\d+, \d+\)", _text(f))]
    assert holders == [SHARED], holders
    pairs = [(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", _text(SHARED))]
    assert len(pairs) == len(set(pairs)) == 15, pairs
    return sorted(pairs)


def expected_forms(rows4):
    """(nw, maxs, exact, g64, mr, b3) of every form a family builds: plain up to rounds of 64 k-steps, 64-wide groups up to 48, 3 bits
    and (where built) four rows up to 32."""
    want = set()
    for nw, maxs in pair_table():
        for exact in (0, 1):
            want.add((nw, maxs, exact, 0, 1, 0))
            if maxs <= 48:
                want.add((nw, maxs, exact, 1, 1, 0))
            if maxs <= 32:
                want.update({(nw, maxs, exact, 0, 1, 1), (nw, maxs, exact, 1, 1, 1)})
                if rows4:
                    want.add((nw, maxs, exact, 0, 4, 0))
    return want


def check_family(src):
    """Every instantiation of the family in `src` is free of scratch and spills inside its twin's launch bound, and the set is the table's."""
    kernel, has_mr, rows4, count, lds_extra = FAMILIES[src]
    res = resources(src)
    assert all(kernel in n for n in res), sorted(res)[:3]             # nothing else is built there
    twins = resources(PLAIN)
    fields = r"_ZN4qllm%d%sILi(\d+)ELi(\d+)ELb([01])ELb([01])E%sLb([01])ELi(\d)EEEvNS_12Strip1ParamsE$" % (len(kernel), kernel, r"Li(\d)E" if has_mr else "()")
    want = expected_forms(rows4)
    got = {}
    for n, r in res.items():
        m = re.search(fields, n)
        assert m, n
        nw, maxs, exact, g64, mr, b3, waves = (int(v or 1) for v in m.groups())
        assert rows4 or mr == 1, n                                                # one row only
        got[(nw, maxs, exact, g64, mr, b3)] = (waves, r)
    assert len(res) == len(got) == len(want) == count and set(got) == want
    for key, (waves, r) in sorted(got.items()):
        nw, maxs, exact, g64, mr, b3 = key
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (key, r)
        assert waves == (8 if maxs <= 24 and not g64 and mr == 1 and not b3 else 4), key   # the twin's launch bound
        # the registers its launch bound allows (512 per SIMD lane over `waves` waves; a 16-wave block needs 4 per SIMD)
        assert r["vgpr_count"] <= 512 // waves, (key, waves, r)
        assert waves * 4 >= nw, (key, waves)
        twin = f"_ZN4qllm13strip1_kernelILi{nw}ELi{maxs}ELb{exact}ELi2ELi4ELb0ELb0ELb{g64}ELi{mr}ELb{b3}EEEvNS_12Strip1ParamsE"
        assert twin in twins, twin
        # LDS: all of it is dynamic -- strip1_lds_bytes<NW, MAXS, MR>() + the family's own at the launch -- and none static
        assert r["group_segment_fixed_size"] == twins[twin]["group_segment_fixed_size"] == 0, key
        assert twins[twin]["vgpr_spill_count"] == 0
    # the sources: one LDS expression and one launch for all families, each unit's own share of the LDS stated once, the shared header included once
    shared = _text(SHARED)
    assert shared.count("strip1_lds_bytes<NW, MAXS, MR>() + F::kLdsExtra") == 1 and "lds_bytes, stream, p)" in shared
    units = [PLAIN, *sorted(FAMILIES)]
    assert sum(_text(f).count("hipLaunchKernelGGL") for f in [SHARED, *units]) == shared.count("hipLaunchKernelGGL") == 1
    assert _text(src).count(lds_extra) == 1 and _text(src).count("kLdsExtra =") == 1
    for f in units:
        assert _text(f).count('#include "%s"' % SHARED) == 1, f
