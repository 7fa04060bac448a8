"""The mid-batch entry (qllm_linear_forward_bitpanel, csrc/bitpanel.hip) without a GPU: the symbols, every refusal before any device work
(fake, aligned, never-dereferenced pointers, as tests/test_bitgemv_actorder_cpu.py), the launch geometry through
qllm_bitpanel_describe (pure host code; 256 CUs without a device), its workspace size, and the planner's unchanged answer."""
import ctypes as C
import os
import re

import pytest

import capi_fakes
from capi_fakes import W
from qllm_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qllm_mi355x.h")


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def call(lib, w, x=20480, y=24576, m=64):
    return lib.qllm_linear_forward_bitpanel(C.byref(w), x, y, m, _lib.DT_F16, None, 0, None)


def describe(lib, w, m, have_ws=1):
    return capi_fakes.describe(lib, "bitpanel", w, m, have_ws)


def geometry(lib, w, m, have_ws=1):
    text = describe(lib, w, m, have_ws)
    got = re.fullmatch(r"bitpanel bits=(\d+) cols=64 row_tiles=(\d+) row_blocks=(\d+) split_k=(\d+)", text)
    assert got, text
    return tuple(int(v) for v in got.groups())


def test_symbols_are_exported_and_declared(lib):
    """The entry is additive: three new symbols, everything else as it was.  (The ABI number stays where the four quantizer test files
    pin it -- an additive symbol has never moved it.)"""
    text = open(HEADER).read()
    for name in ("qllm_linear_forward_bitpanel", "qllm_bitpanel_workspace_bytes", "qllm_bitpanel_describe"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in text, name
    assert lib.qllm_abi_version() == _lib.ABI_VERSION
    assert f"#define QLLM_BITPANEL_MAX_M_DEFAULT {_lib.BITPANEL_MAX_M_DEFAULT}\n" in text
    assert _lib.BITPANEL_MAX_M_DEFAULT == 0 or 17 <= _lib.BITPANEL_MAX_M_DEFAULT <= 512   # 0: the modules do not route to the entry


def test_refusals_come_before_any_device_work(lib):
    for m in (16, 513):
        assert call(lib, W(), m=m) == _lib.QLLM_ERR_UNSUPPORTED, m
        assert "17..512" in _lib.last_error() and "qllm_dequant" in _lib.last_error()
    assert call(lib, W(g_idx=28672)) == _lib.QLLM_ERR_INVALID and "g_idx" in _lib.last_error()
    assert call(lib, W(), x=None) == _lib.QLLM_ERR_INVALID
    assert call(lib, W(), y=None) == _lib.QLLM_ERR_INVALID
    assert call(lib, W(bits=4, layout=_lib.LAYOUT_AWQ_GEMM)) == _lib.QLLM_ERR_UNSUPPORTED
    assert "qllm_dequant" in _lib.last_error()
    assert call(lib, W(K=1040)) == _lib.QLLM_ERR_UNSUPPORTED      # K % 32 != 0
    assert call(lib, W(g=48)) == _lib.QLLM_ERR_UNSUPPORTED        # group_size % 32 != 0
    assert call(lib, W(layout=_lib.LAYOUT_HQQ, N=1001)) == _lib.QLLM_ERR_UNSUPPORTED   # fp16 zero points are fetched as dwords
    assert call(lib, W(layout=_lib.LAYOUT_HQQ, qzeros=12290)) == _lib.QLLM_ERR_UNSUPPORTED
    for m in (16, 513):
        assert describe(lib, W(), m).startswith("unsupported (")


def test_entry_follows_its_knob(lib):
    try:
        assert lib.qllm_set_knob(b"QLLM_BITPANEL", 0) == 0
        assert call(lib, W()) == _lib.QLLM_ERR_UNSUPPORTED
        assert "QLLM_BITPANEL" in _lib.last_error() and "qllm_dequant" in _lib.last_error()
        assert describe(lib, W(), 64).startswith("unsupported (QLLM_BITPANEL is off")
    finally:
        lib.qllm_reset_knobs()
    assert describe(lib, W(), 64).startswith("bitpanel bits=8 ")   # served again
    v, is_set = C.c_int32(0), C.c_int32(0)
    assert lib.qllm_get_knob(b"QLLM_BITPANEL", C.byref(v), C.byref(is_set)) == 0 and is_set.value == 0
    # the module's cutoff is a knob too, inside the rows the entry serves
    assert lib.qllm_set_knob(b"QLLM_BITPANEL_MAX_M", 16) == _lib.QLLM_ERR_INVALID
    assert lib.qllm_set_knob(b"QLLM_BITPANEL_MAX_M", 513) == _lib.QLLM_ERR_INVALID
    # the ingest of the packed words is a knob of the kernel, not of the geometry that describe prints
    try:
        before = describe(lib, W(), 64)
        assert lib.qllm_set_knob(b"QLLM_BITPANEL_LDS", 1) == 0 and describe(lib, W(), 64) == before
        assert lib.qllm_set_knob(b"QLLM_BITPANEL_LDS", 2) == _lib.QLLM_ERR_INVALID
    finally:
        lib.qllm_reset_knobs()
    try:
        assert lib.qllm_set_knob(b"QLLM_BITPANEL_MAX_M", 64) == 0
        assert describe(lib, W(), 512).startswith("bitpanel ")     # the entry itself always takes up to 512 rows
    finally:
        lib.qllm_reset_knobs()


def test_describe_pins_the_geometry(lib):
    """4096 x 4096 is 64 panels: 4 splits cover 256 CUs up to 128 rows, two row blocks leave room for 2, four for none."""
    w = W()
    assert describe(lib, w, 64) == "bitpanel bits=8 cols=64 row_tiles=4 row_blocks=1 split_k=4"
    want = {17: (8, 2, 1, 4), 32: (8, 2, 1, 4), 33: (8, 4, 1, 4), 64: (8, 4, 1, 4), 65: (8, 8, 1, 4), 128: (8, 8, 1, 4), 129: (8, 8, 2, 2),
            256: (8, 8, 2, 2), 257: (8, 8, 3, 1), 512: (8, 8, 4, 1)}
    for m, geo in want.items():
        assert geometry(lib, w, m) == geo, m
        assert geometry(lib, w, m, have_ws=0) == geo[:3] + (1,), m
    assert geometry(lib, W(bits=5), 64) == (5, 4, 1, 4)
    # two panels: split until every split still has two K-tiles of 8 units (K / 32 / 16 = 8)
    narrow = W(N=128)
    assert geometry(lib, narrow, 64) == (8, 4, 1, 8) and geometry(lib, narrow, 64, have_ws=0) == (8, 4, 1, 1)
    # a split is a whole number of groups: one group over all of K leaves nothing to split
    assert geometry(lib, W(N=128, g=4096), 64)[3] == 1
    # ragged widths are served: 1000 = 15 panels and 40 columns
    assert geometry(lib, W(N=1000, qzeros=None), 64)[:3] == (8, 4, 1)
    assert geometry(lib, W(N=1000, layout=_lib.LAYOUT_HQQ), 200)[:3] == (8, 8, 2)
    assert geometry(lib, W(bits=3, N=1000, qzeros=None), 17)[:3] == (3, 2, 1)


def test_workspace_is_the_counter_page_plus_the_slabs(lib):
    size = lambda w, m: lib.qllm_bitpanel_workspace_bytes(C.byref(w), m)  # noqa: E731
    w = W()
    for m in (17, 64, 128, 129, 512):
        _bits, mt, rb, split = geometry(lib, w, m)
        slabs = 64 * rb * split * mt * 16 * 64 * 4 if split > 1 else 0   # [panel x row block][split][mt x 16 rows x 64 columns] fp32
        assert size(w, m) == 16384 + slabs, m
    assert size(w, 512) == 16384 and size(w, 64) > size(w, 17) > 16384
    narrow = W(N=128)
    assert size(narrow, 64) == 16384 + 2 * 8 * 64 * 64 * 4
    assert size(W(N=128, g=4096), 64) == 16384   # no split, no slabs
    assert size(w, 16) == 16384 and size(W(K=1040), 64) == 16384   # unserved calls: the counter page alone
    assert size(w, 512) <= 64 << 20 and size(W(N=65536, K=1024), 128) <= 64 << 20   # inside the modules' persistent workspace


def test_the_planner_does_not_know_the_entry(lib):
    """qllm_linear_forward / qllm_plan_describe answer these calls exactly as before: the kernel is reached through its own entry."""
    w = W(bits=5)
    buf = C.create_string_buffer(256)
    assert lib.qllm_plan_describe(C.byref(w), 1, 64, 1, buf, 256) == 0
    assert buf.value.decode() == "unsupported (no fused kernel for bits=5 K=4096 N=4096 g=128 layout=0 act_order=0; use qllm_dequant + GEMM)"
    assert lib.qllm_linear_forward(C.byref(w), 20480, 24576, 64, _lib.DT_F16, None, 0, None) == _lib.QLLM_ERR_UNSUPPORTED
