"""-m gpu: the batch-1 kernel (csrc/strip1_kernel.hpp) computes, bit for bit, what it computed before its instruction-budget rework
(profiles/strip1_valu_budget.md).  tests/golden/strip1_parent/<case>.npz hold the outputs of the commit before that rework, written on
an MI355X by tools/make_strip1_fixtures.py; the inputs are regenerated here from the same seeds.  Every 4-bit g128 form of the shape
table at its smallest shape (shifted and exact windows, one and two 16-byte chunks of x per lane, more strips than CUs, the odd wave
count), packed / fp16 / symmetric zero points, fp16 and bf16 activations, with and without bias, the AutoGPTQ offset on the packed
cases; a grouped launch of unequal widths; 64-wide groups; the four-row form at M = 3; 3 bits with 128- and 64-wide groups.  Each
case asserts its plan line first, so a planner change cannot turn it into a test of another kernel.  Tolerance: zero."""
import importlib.util
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("make_strip1_fixtures", os.path.join(ROOT, "tools", "make_strip1_fixtures.py"))
fx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(fx)

CASES = fx.cases()


def test_every_case_has_its_fixture():
    have = sorted(f[:-4] for f in os.listdir(fx.OUT_DIR) if f.endswith(".npz"))
    assert have == sorted(n for n, _ in CASES)


@pytest.mark.parametrize("name,spec", CASES, ids=[n for n, _ in CASES])
def test_outputs_equal_the_parents(name, spec):
    want = dict(np.load(os.path.join(fx.OUT_DIR, name + ".npz"), allow_pickle=False))
    got = fx.run_case(name, spec)   # (asserts the plan line before it runs the kernel)
    assert sorted(got) == sorted(want)
    assert len(got) == 2 * 2 * len(spec["compats"])   # activations x bias x add_zero_bias
    for key in sorted(want):
        assert got[key].shape == want[key].shape == (spec["M"], sum(spec["widths"])), key
        assert torch.equal(torch.from_numpy(got[key].astype(np.int32)), torch.from_numpy(want[key].astype(np.int32))), (name, key)
