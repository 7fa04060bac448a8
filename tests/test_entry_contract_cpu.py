"""The host side of every entry with a check of its own, replayed against tests/golden/entry_contract.json (written by
tools/record_entry_contract.py on the commit whose behaviour it pins): the exact status and qllm_last_error() text of every refusal --
and with the calls that trip two checks at once, which check fires first --, every describe line and every workspace size.  Fake,
aligned, never-dereferenced pointers (tests/capi_fakes.py); geometry for 256 compute units, so a child process with QLLM_NUM_CU set does
the calls (the variable is read once per process)."""
import json
import os
import subprocess
import sys

import pytest

from qllm_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "entry_contract.json")

_CHILD = r"""
import json, sys
import capi_fakes
from qllm_amd import _lib
lib = _lib.load()
forward = sys.argv[2] == "forward"
bad = []
n = 0
for rec in json.load(open(sys.argv[1])):
    if (rec["entry"] in capi_fakes.FORWARD_ENTRIES) != forward:
        continue
    n += 1
    got = capi_fakes.call_with_knobs(lib, rec["entry"], rec["args"], rec.get("knobs"))
    if got != rec["got"]:
        bad.append({"case": {k: rec[k] for k in rec if k != "got"}, "want": rec["got"], "got": got})
print(json.dumps({"n": n, "bad": bad}))
"""


def replay(which):
    env = dict(os.environ, QLLM_NUM_CU="256", PYTHONPATH=os.pathsep.join([HERE, os.path.dirname(HERE)] + sys.path))
    got = subprocess.run([sys.executable, "-c", _CHILD, GOLDEN, which], env=env, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr
    out = json.loads(got.stdout.strip().splitlines()[-1])
    assert out["n"] > 0
    assert not out["bad"], f"{len(out['bad'])} of {out['n']} records differ, the first: {json.dumps(out['bad'][0], indent=1)}"
    return out["n"]


@pytest.fixture(scope="module")
def built():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")


def test_the_file_covers_every_entry():
    entries = {rec["entry"] for rec in json.load(open(GOLDEN))}
    for name in ("bitpanel", "bitgemm", "bitgroup"):
        assert {f"qllm_linear_forward_{name}", f"qllm_{name}_workspace_bytes", f"qllm_{name}_describe"} <= entries, name
    assert {"qllm_linear_forward_grouped", "qllm_linear_forward_rmsnorm", "qllm_linear_forward_permuted", "qllm_plan_describe",
            "qllm_rmsnorm_describe", "qllm_swiglu_describe", "qllm_gather_columns", "qllm_gather_describe"} <= entries
    for rec in json.load(open(GOLDEN)):   # a forward entry is in the file with refused arguments only
        if rec["entry"] in ("qllm_linear_forward_grouped", "qllm_linear_forward_rmsnorm", "qllm_linear_forward_permuted", "qllm_gather_columns") or rec["entry"].startswith("qllm_linear_forward_bit"):
            assert rec["got"]["rc"] in (_lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_WORKSPACE), rec


def test_describe_and_size_entries_answer_as_recorded(built):
    assert replay("host") >= 200


def test_forward_entries_refuse_as_recorded(built):
    """Only where no HIP device is visible: a slip that turned one of these refusals into a launch would run a kernel on fake pointers."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: the forward entries are not called with fake pointers")
    assert replay("forward") >= 100
