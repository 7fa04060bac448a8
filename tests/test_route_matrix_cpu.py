"""The route matrix (tests/route_matrix.py), checked without a GPU: every row plans exactly the way it says (qllm_plan_describe with a
workspace, placeholder descriptors that are never launched), and the rows together cover every kernel family and every form-token the
planner prints -- so a planner change that moves a row elsewhere fails here, not as silently thinner coverage on the GPU."""
import ctypes as C
import re

import pytest

import route_matrix as RM
from qllm_amd import _lib

COUNTERS = 16384


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def _plan(lib, r):
    ws = RM.placeholder_weights(r)
    arr = (_lib.QllmWeight * len(ws))(*ws)
    buf = C.create_string_buffer(256)
    try:
        for k, v in r.knobs.items():
            _lib.check(lib.qllm_set_knob(k.encode(), v))
        rc = lib.qllm_plan_describe(arr, len(ws), r.M, 1, buf, 256)
    finally:
        lib.qllm_reset_knobs()
    assert rc == 0, (r.id, _lib.last_error())
    return buf.value.decode()


def test_row_ids_are_unique():
    ids = [r.id for r in RM.ROWS]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("r", RM.ROWS, ids=[r.id for r in RM.ROWS])
def test_row_plans_as_stated(lib, r):
    assert _plan(lib, r) == r.plan
    # the workspace every row's GPU run gets (workspace B): the size function's answer, or the grouped rule -- never below the counters
    for w in RM.placeholder_weights(r):
        assert lib.qllm_workspace_bytes_act(C.byref(w), r.M, RM.act_dtype(r)) >= COUNTERS


def test_every_family_and_form_is_covered(lib):
    missing = [what for what, rx, which in RM.REQUIRED
               if not any(re.search(rx, r.plan) and RM.selects(r, which) for r in RM.ROWS)]
    assert not missing, missing
    families = {r.plan.split()[0] for r in RM.ROWS}
    assert families == {"strip1", "strip", "panel", "skinny", "bitgemv", "gemm", "gemm2", "gemm3"}
    kinds = {r.kind for r in RM.ROWS}
    assert kinds == set(RM.KIND_LAYOUT)


def test_the_staged_bf16_row_needs_the_fp16_copy(lib):
    """The bf16 row-stream gemm3 row takes the fp16 staging copy of x: the dtype-aware size charges exactly M x K x 2 bytes for it."""
    r = next(r for r in RM.ROWS if r.id == "bf16-gemm3-staged")
    (w,) = RM.placeholder_weights(r)
    f16 = lib.qllm_workspace_bytes_act(C.byref(w), r.M, _lib.DT_F16)
    bf16 = lib.qllm_workspace_bytes_act(C.byref(w), r.M, _lib.DT_BF16)
    assert bf16 - f16 == r.M * r.K * 2


def test_prefill_groups_need_more_than_their_layers(lib):
    """A prefill group's tail split counts the tiles of all its layers: for the grouped gemm3 rows the layers' own sizes add up to less
    than the split the group takes -- the grouped rule (include/qllm_mi355x.h, ops.grouped_workspace_bytes) adds 128 KB per CU."""
    r = next(r for r in RM.ROWS if r.id == "gemm3-group-tail")
    total = sum(lib.qllm_workspace_bytes_act(C.byref(w), r.M, RM.act_dtype(r)) for w in RM.placeholder_weights(r))
    tiles = sum((r.M + 255) // 256 * (n // 128) for n in RM.widths(r))      # 2 x 86 x 2 = 344 = one round of 256 CUs + 88
    need = COUNTERS + (tiles - 256) * 2 * 256 * 128 * 4                      # tail_split=2
    assert total < need <= COUNTERS + 256 * 256 * 128 * 4
