"""The 2..8-bit prefill entry (qllm_linear_forward_bitgemm, csrc/bitgemm.hip) without a GPU: the symbols and the header's default,
the knob ranges, every refusal before any device work (fake, aligned, never-dereferenced pointers, as tests/test_capi_symbols.py), the
launch geometry through qllm_bitgemm_describe (pure host code; QLLM_NUM_CU=256, read once per process: a child process pins it) with
its workspace size, and the planner's unchanged answer."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

import capi_fakes
from capi_fakes import W
from qllm_amd import _lib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = os.path.join(ROOT, "include", "qllm_mi355x.h")


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def call(lib, w, x=20480, y=24576, m=300, dt=_lib.DT_F16):
    return lib.qllm_linear_forward_bitgemm(C.byref(w), x, y, m, dt, None, 0, None)


def describe(lib, w, m, have_ws=1):
    return capi_fakes.describe(lib, "bitgemm", w, m, have_ws)


def test_symbols_are_exported_and_declared(lib):
    """The entry is additive: three new symbols within ABI 7, and one constant that the header and the loader agree on."""
    text = open(HEADER).read()
    for name in ("qllm_linear_forward_bitgemm", "qllm_bitgemm_workspace_bytes", "qllm_bitgemm_describe"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in text, name
    assert lib.qllm_abi_version() == _lib.ABI_VERSION
    assert f"#define QLLM_BITGEMM_MIN_M_DEFAULT {_lib.BITGEMM_MIN_M_DEFAULT}\n" in text
    # 0: the modules do not route to the entry; else above every row count the mid-batch cutoff's default leaves alone
    assert _lib.BITGEMM_MIN_M_DEFAULT == 0 or 257 <= _lib.BITGEMM_MIN_M_DEFAULT <= 65536


def test_knob_ranges(lib):
    try:
        assert lib.qllm_set_knob(b"QLLM_BITGEMM_MIN_M", 128) == _lib.QLLM_ERR_INVALID
        assert lib.qllm_set_knob(b"QLLM_BITGEMM_MIN_M", 65537) == _lib.QLLM_ERR_INVALID
        assert lib.qllm_set_knob(b"QLLM_BITGEMM_MIN_M", 129) == 0 and lib.qllm_set_knob(b"QLLM_BITGEMM_MIN_M", 65536) == 0
        assert lib.qllm_set_knob(b"QLLM_BITGEMM", 2) == _lib.QLLM_ERR_INVALID
        # the callers' line does not move the entry: it always takes 129 rows and up
        assert describe(lib, W(), 129).startswith("bitgemm bits=8 ")
    finally:
        lib.qllm_reset_knobs()
    v, is_set = C.c_int32(0), C.c_int32(0)
    assert lib.qllm_get_knob(b"QLLM_BITGEMM_MIN_M", C.byref(v), C.byref(is_set)) == 0 and is_set.value == 0


def test_ops_min_m_follows_the_knobs(lib):
    from qllm_amd import ops
    try:
        assert ops.bitgemm_min_m() == _lib.BITGEMM_MIN_M_DEFAULT
        assert lib.qllm_set_knob(b"QLLM_BITGEMM_MIN_M", 300) == 0 and ops.bitgemm_min_m() == 300
        assert lib.qllm_set_knob(b"QLLM_BITGEMM", 0) == 0 and ops.bitgemm_min_m() == 0
    finally:
        lib.qllm_reset_knobs()


def test_refusals_come_before_any_device_work(lib):
    err = _lib.last_error
    # rows: the alternatives are the mid-batch entry and the planner's
    for m in (1, 17, 128):
        assert call(lib, W(), m=m) == _lib.QLLM_ERR_UNSUPPORTED, m
        assert "qllm_linear_forward_bitpanel" in err() and "qllm_linear_forward" in err() and "129" in err()
        assert describe(lib, W(), m).startswith("unsupported (")
    # bf16 activations as they are
    assert call(lib, W(), dt=_lib.DT_BF16) == _lib.QLLM_ERR_UNSUPPORTED
    assert "convert x to fp16, pass QLLM_F16_IN_BF16_OUT" in err()
    # other layouts, shapes, alignments: dequant + GEMM
    for w in (W(bits=4, layout=_lib.LAYOUT_AWQ_GEMM), W(bits=4, layout=_lib.LAYOUT_NATIVE), W(K=4128), W(g=48), W(N=4100), W(qweight=4098),
              W(layout=_lib.LAYOUT_HQQ, qzeros=12290), W(K=1 << 20, N=4096)):
        assert call(lib, w) == _lib.QLLM_ERR_UNSUPPORTED, (w.K, w.N, w.group_size, w.layout)
        assert "qllm_dequant" in err(), err()
    assert call(lib, W(), x=20488) == _lib.QLLM_ERR_UNSUPPORTED and "16-byte" in err() and "qllm_dequant" in err()
    assert call(lib, W(), y=24584) == _lib.QLLM_ERR_UNSUPPORTED and "16-byte" in err()
    assert call(lib, W(K=65536, N=64), m=16385) == _lib.QLLM_ERR_UNSUPPORTED and "2 GiB" in err()   # M K 2 = 2 GiB
    # arguments no call takes
    assert call(lib, W(), x=None) == _lib.QLLM_ERR_INVALID
    assert call(lib, W(), y=None) == _lib.QLLM_ERR_INVALID
    assert call(lib, W(g_idx=28672)) == _lib.QLLM_ERR_INVALID and "g_idx" in err() and "qllm_gather_columns" in err()
    for bits in (1, 9):
        assert call(lib, W(bits=bits)) == _lib.QLLM_ERR_INVALID and "bits" in err()
    assert call(lib, W(), dt=_lib.DT_F32) == _lib.QLLM_ERR_INVALID
    # served shapes pass every host check of describe: all widths, the three zero-point kinds, ragged widths
    for bits in range(2, 9):
        assert describe(lib, W(bits=bits), 129).startswith(f"bitgemm bits={bits} tile=256x128 ")
    assert describe(lib, W(N=1000, qzeros=None), 300).startswith("bitgemm ")
    assert describe(lib, W(N=1000, layout=_lib.LAYOUT_HQQ), 300).startswith("bitgemm ")
    assert describe(lib, W(K=576, N=256, g=576), 300).startswith("bitgemm ")


def test_entry_follows_its_knob(lib):
    try:
        assert lib.qllm_set_knob(b"QLLM_BITGEMM", 0) == 0
        assert call(lib, W()) == _lib.QLLM_ERR_UNSUPPORTED
        assert "QLLM_BITGEMM" in _lib.last_error() and "qllm_dequant" in _lib.last_error()
        assert describe(lib, W(), 300).startswith("unsupported (QLLM_BITGEMM is off")
        assert lib.qllm_bitgemm_workspace_bytes(C.byref(W(N=128)), 300) == 16384
    finally:
        lib.qllm_reset_knobs()
    assert describe(lib, W(), 300).startswith("bitgemm bits=8 ")


# (K, N, M, tiles, S with a workspace): the largest power of two S <= 8 with tiles x S <= 256 CUs and K / 64 / S >= 8
SPLIT_TABLE = [
    (4096, 256, 129, 2, 8),      # 2 tiles x 64 k-tiles
    (4096, 128, 513, 3, 8),
    (1216, 128, 300, 2, 2),      # 19 k-tiles: 9 + 10
    (1152, 128, 1152, 5, 2),     # 18 k-tiles
    (512, 992, 300, 16, 1),      # 8 k-tiles
    (64, 128, 129, 1, 1),
    (4096, 4096, 300, 64, 4),    # 64 tiles: 4 x 64 = 256 CUs
    (4096, 4096, 257, 64, 4),
    (4096, 4096, 513, 96, 2),
    (4096, 4096, 2048, 256, 1),
    (4096, 11008, 300, 172, 1),
    (11008, 4096, 300, 64, 4),   # 172 k-tiles
    (4096, 1000, 300, 16, 8),    # a ragged last column tile counts as one
    (1024, 1000, 129, 8, 2),
]

_CHILD = r"""
import ctypes as C, json, sys
from qllm_amd import _lib
lib = _lib.load()
out = []
for K, N, M in json.loads(sys.argv[1]):
    w = _lib.QllmWeight(4096, 8192, 12288 if N % 32 == 0 else None, None, None, K, N, 128 if K % 128 == 0 else 32, 8, _lib.LAYOUT_GPTQ, 0)
    row = []
    for have in (1, 0):
        buf = C.create_string_buffer(512)
        assert lib.qllm_bitgemm_describe(C.byref(w), M, have, buf, 512) == 0, _lib.last_error()
        row.append(buf.value.decode())
    row.append(lib.qllm_bitgemm_workspace_bytes(C.byref(w), M))
    out.append(row)
print(json.dumps(out))
"""


def test_describe_and_workspace_follow_the_split_rule(lib):
    """Under QLLM_NUM_CU=256 (the variable is read once per process, so a child process asks)."""
    env = dict(os.environ, QLLM_NUM_CU="256", PYTHONPATH=os.pathsep.join([os.path.abspath(ROOT)] + sys.path))
    got = subprocess.run([sys.executable, "-c", _CHILD, json.dumps([row[:3] for row in SPLIT_TABLE])], env=env, capture_output=True, text=True)
    assert got.returncode == 0, got.stderr
    rows = json.loads(got.stdout.strip().splitlines()[-1])
    for (K, N, M, tiles, S), (with_ws, without_ws, nbytes) in zip(SPLIT_TABLE, rows):
        assert with_ws == f"bitgemm bits=8 tile=256x128 tiles={tiles} split_k={S}", (K, N, M, with_ws)
        assert without_ws == f"bitgemm bits=8 tile=256x128 tiles={tiles} split_k=1", (K, N, M, without_ws)   # have_workspace = 0 -> S = 1
        assert nbytes == 16384 + (tiles * S * 256 * 128 * 4 if S > 1 else 0), (K, N, M, nbytes)
        assert nbytes <= 64 << 20, (K, N, M, nbytes)   # inside the modules' persistent workspace
        assert re.fullmatch(r"bitgemm bits=\d tile=256x128 tiles=\d+ split_k=[1248]", with_ws)


def test_the_planner_does_not_know_the_entry(lib):
    """qllm_linear_forward / qllm_plan_describe answer these calls exactly as before: the kernel is reached through its own entry."""
    w = W(bits=5)
    buf = C.create_string_buffer(256)
    assert lib.qllm_plan_describe(C.byref(w), 1, 300, 1, buf, 256) == 0
    assert buf.value.decode() == "unsupported (no fused kernel for bits=5 K=4096 N=4096 g=128 layout=0 act_order=0; use qllm_dequant + GEMM)"
    assert lib.qllm_linear_forward(C.byref(w), 20480, 24576, 300, _lib.DT_F16, None, 0, None) == _lib.QLLM_ERR_UNSUPPORTED
