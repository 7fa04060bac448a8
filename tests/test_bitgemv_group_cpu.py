"""The grouped bit-stream entry (qllm_linear_forward_bitgroup, csrc/bitgemv_group.hip) without a GPU: the symbols, every refusal before
any device work (fake, aligned, never-dereferenced pointers, as tests/test_bitpanel_cpu.py), the launch geometry through
qllm_bitgroup_describe (pure host code; 256 CUs without a device) -- every member keeps the split of its own single launch --, the
workspace size, the planner's unchanged answers, and the resources of the 35 instantiations."""
import ctypes as C
import os
import re

import pytest

import capi_fakes
from capi_fakes import W, arr
from kernel_resources import resources
from qllm_amd import _lib

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qllm_mi355x.h")
X, Y0 = capi_fakes.X, capi_fakes.Y   # fake device addresses (16-byte aligned)

# Llama-2-7B q/k/v, gate/up and a GQA triple
SHAPE_SETS = {"qkv": (4096, (4096, 4096, 4096)), "gate_up": (4096, (11008, 11008)), "gqa": (4096, (4096, 1024, 1024))}


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def call(lib, ws, x=X, ys=None, m=1, n=None):
    n = len(ws) if n is None else n
    ys = [Y0 + 4096 * i for i in range(len(ws))] if ys is None else ys
    return lib.qllm_linear_forward_bitgroup(arr(ws), (C.c_void_p * len(ys))(*ys), n, x, m, _lib.DT_F16, None, 0, None)


def describe(lib, ws, m, have_ws=1):
    return capi_fakes.describe(lib, "bitgroup", ws, m, have_ws)


def geometry(lib, ws, m, have_ws=1):
    """(bits, layers, blocks, [split_k per member])"""
    text = describe(lib, ws, m, have_ws)
    got = re.fullmatch(r"bitgroup bits=(\d+) cols=32 layers=(\d+) blocks=(\d+) split_k=([\d,]+)", text)
    assert got, text
    return int(got.group(1)), int(got.group(2)), int(got.group(3)), [int(v) for v in got.group(4).split(",")]


def single_split(lib, w, m, have_ws=1):
    buf = C.create_string_buffer(256)
    assert lib.qllm_plan_describe(C.byref(w), 1, m, have_ws, buf, 256) == 0
    got = re.fullmatch(r"bitgemv bits=\d+ cols=32 waves=8 split_k=(\d+)", buf.value.decode())
    assert got, buf.value
    return int(got.group(1))


def test_symbols_are_exported_and_declared(lib):
    text = open(HEADER).read()
    for name in ("qllm_linear_forward_bitgroup", "qllm_bitgroup_workspace_bytes", "qllm_bitgroup_describe"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and name + "(" in text, name
    assert lib.qllm_abi_version() == _lib.ABI_VERSION == 7
    assert f"#define QLLM_BITGROUP_MAX_M_DEFAULT {_lib.BITGROUP_MAX_M_DEFAULT}\n" in text
    assert 0 <= _lib.BITGROUP_MAX_M_DEFAULT <= 16   # 0: the sibling groups do not route to the entry


def test_refusals_come_before_any_device_work(lib):
    pair = [W(), W(N=1024)]
    # invalid arguments
    assert call(lib, pair, x=None) == _lib.QLLM_ERR_INVALID
    assert call(lib, pair, ys=[Y0, None]) == _lib.QLLM_ERR_INVALID
    assert call(lib, pair, n=0) == _lib.QLLM_ERR_INVALID and "1..4" in _lib.last_error()
    assert call(lib, [W()] * 5) == _lib.QLLM_ERR_INVALID and "1..4" in _lib.last_error()
    for other in (W(K=2048), W(bits=5), W(g=64), W(azb=1)):
        assert call(lib, [W(), other]) == _lib.QLLM_ERR_INVALID, other
        assert "agree" in _lib.last_error()
    assert call(lib, [W(), W(bits=4, layout=_lib.LAYOUT_AWQ_GEMM)]) == _lib.QLLM_ERR_INVALID   # bits, and the layout family
    assert call(lib, [W(), W(g_idx=28672)]) == _lib.QLLM_ERR_INVALID and "g_idx" in _lib.last_error()
    # unsupported: the message names the alternative
    for m in (17, 64):
        assert call(lib, pair, m=m) == _lib.QLLM_ERR_UNSUPPORTED, m
        assert "1..16" in _lib.last_error() and "layer by layer" in _lib.last_error()
        assert describe(lib, pair, m).startswith("unsupported (")
    assert call(lib, [W(bits=4, layout=_lib.LAYOUT_AWQ_GEMM)] * 2) == _lib.QLLM_ERR_UNSUPPORTED and "layer by layer" in _lib.last_error()
    assert call(lib, [W(bits=4, N=64, layout=_lib.LAYOUT_NATIVE)] * 2) == _lib.QLLM_ERR_UNSUPPORTED and "layer by layer" in _lib.last_error()
    assert call(lib, [W(K=1040, g=1040)] * 2) == _lib.QLLM_ERR_UNSUPPORTED          # K % 32 != 0
    assert call(lib, [W(layout=_lib.LAYOUT_HQQ, N=1001)] * 2) == _lib.QLLM_ERR_UNSUPPORTED   # fp16 zero points are fetched as dwords
    # HQQ and GPTQ members are one layout family
    assert describe(lib, [W(), W(layout=_lib.LAYOUT_HQQ)], 1).startswith("bitgroup ")


def test_entry_follows_its_knobs(lib):
    pair = [W(), W(N=1024)]
    try:
        assert lib.qllm_set_knob(b"QLLM_BITGROUP", 0) == 0
        assert call(lib, pair) == _lib.QLLM_ERR_UNSUPPORTED
        assert "QLLM_BITGROUP is off" in _lib.last_error() and "layer by layer" in _lib.last_error()
        assert describe(lib, pair, 1).startswith("unsupported (QLLM_BITGROUP is off")
    finally:
        lib.qllm_reset_knobs()
    assert describe(lib, pair, 1).startswith("bitgroup bits=8 ")
    assert lib.qllm_set_knob(b"QLLM_BITGROUP", 2) == _lib.QLLM_ERR_INVALID
    assert lib.qllm_set_knob(b"QLLM_BITGROUP_MAX_M", 17) == _lib.QLLM_ERR_INVALID
    assert lib.qllm_set_knob(b"QLLM_BITGROUP_MAX_M", -1) == _lib.QLLM_ERR_INVALID
    try:
        assert lib.qllm_set_knob(b"QLLM_BITGROUP_MAX_M", 0) == 0
        assert describe(lib, pair, 16).startswith("bitgroup ")   # the callers' cutoff: the entry itself always takes up to 16 rows
    finally:
        lib.qllm_reset_knobs()
    v, is_set = C.c_int32(0), C.c_int32(0)
    assert lib.qllm_get_knob(b"QLLM_BITGROUP_MAX_M", C.byref(v), C.byref(is_set)) == 0 and is_set.value == 0


@pytest.mark.parametrize("shapes", sorted(SHAPE_SETS))
@pytest.mark.parametrize("bits", (2, 5, 8))
@pytest.mark.parametrize("m", (1, 16))
def test_every_member_keeps_the_split_of_its_own_launch(lib, shapes, bits, m):
    K, ns = SHAPE_SETS[shapes]
    ws = [W(bits=bits, K=K, N=n) for n in ns]
    got_bits, layers, blocks, splits = geometry(lib, ws, m)
    assert (got_bits, layers) == (bits, len(ns))
    assert splits == [single_split(lib, w, m) for w in ws]
    assert blocks == sum(s * ((n + 31) // 32) for s, n in zip(splits, ns))
    assert geometry(lib, ws, m, have_ws=0)[3] == [1] * len(ns)
    assert geometry(lib, ws, m, have_ws=0)[3] == [single_split(lib, w, m, have_ws=0) for w in ws]
    assert lib.qllm_bitgroup_workspace_bytes(arr(ws), len(ws), m) == 16384 + sum(s * m * n * 4 for s, n in zip(splits, ns))


def test_splits_are_listed_in_the_callers_order(lib):
    """The launch lays the members out widest first; the text (and the outputs) keep the caller's order."""
    narrow_first = [W(N=1024), W(N=4096), W(N=1024)]
    splits = geometry(lib, narrow_first, 1)[3]
    assert splits == [single_split(lib, w, 1) for w in narrow_first] and splits[0] > splits[1]
    assert geometry(lib, [W()], 1)[3] == [single_split(lib, W(), 1)]     # a group of one


def test_unserved_calls_need_the_counter_page_alone(lib):
    assert lib.qllm_bitgroup_workspace_bytes(arr([W(), W()]), 2, 17) == 16384
    assert lib.qllm_bitgroup_workspace_bytes(arr([W(), W(bits=5)]), 2, 1) == 16384
    # inside the modules' persistent workspace
    wide = [W(N=11008)] * 4
    assert lib.qllm_bitgroup_workspace_bytes(arr(wide), 4, 16) <= 64 << 20


def test_the_planner_does_not_know_the_entry(lib):
    """qllm_plan_describe / qllm_linear_forward_grouped answer an 8-bit pair exactly as before."""
    pair = [W(), W(N=1024)]
    buf = C.create_string_buffer(256)
    assert lib.qllm_plan_describe(arr(pair), 2, 1, 1, buf, 256) == 0
    refusal = "grouped forward needs the decode kernel (4-bit, M<=64, K%32==0, no act-order)"
    assert buf.value.decode() == f"unsupported ({refusal})"
    ys = (C.c_void_p * 2)(Y0, Y0 + 4096)
    assert lib.qllm_linear_forward_grouped(arr(pair), ys, 2, X, 1, _lib.DT_F16, None, 0, None) == _lib.QLLM_ERR_UNSUPPORTED
    assert _lib.last_error() == refusal
    assert lib.qllm_plan_describe(C.byref(pair[0]), 1, 1, 1, buf, 256) == 0 and buf.value.decode().startswith("bitgemv bits=8 ")


# ---- resources (hipcc -S; no GPU) ------------------------------------------------------------------------------------------------------
def _instantiations(src, kernel):
    res = {}
    for name, r in resources(src).items():
        got = re.search(kernel + r"ILi(\d+)ELi(\d+)E", name)   # <BITS, MT>
        if got:
            res[(int(got.group(1)), int(got.group(2)))] = r
    return res


def _waves_per_simd(vgprs):
    """gfx950: 512 registers per SIMD lane, allocated in blocks of 8; at most 8 waves"""
    return min(8, 512 // (-(-vgprs // 8) * 8))


def test_all_35_instantiations_are_built_without_spill_or_scratch():
    group = _instantiations("bitgemv_group.hip", "bitgemv_group_kernel")
    assert sorted(group) == [(b, mt) for b in range(2, 9) for mt in (1, 2, 4, 8, 16)]
    for key, r in group.items():
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0, (key, r)


def test_register_use_allows_the_occupancy_of_the_single_layer_kernel():
    group = _instantiations("bitgemv_group.hip", "bitgemv_group_kernel")
    twin = _instantiations("bitgemv.hip", "bitgemv_kernel")
    assert sorted(twin) == sorted(group)
    for key in group:
        assert _waves_per_simd(group[key]["vgpr_count"]) >= _waves_per_simd(twin[key]["vgpr_count"]), (key, group[key], twin[key])
