"""Falcon-shaped native layers (N or K an odd multiple of 64), checked without a GPU through qllm_plan_describe: prefill sizes on
gemm3's half-wide last column tile (` n_tail=64`), batch 1 on the 64-wide-group forms of the batch-1 kernel at K % 128 == 64, the
workspace that covers their splits -- and every neighbouring route left as it was."""
import ctypes as C

import pytest

from qllm_amd import _lib

GPTQ, NATIVE, NATIVE_F16Z = _lib.LAYOUT_GPTQ, _lib.LAYOUT_NATIVE, _lib.LAYOUT_NATIVE_F16Z
G3 = "gemm3 tile=256x128 matrix-waves=8 staging-waves=4"
SM = " layout=strip-major"
COUNTERS = 16384                 # the workspace's arrival counters (planner.hpp, kCounterBytes)
TILE_SLAB = 256 * 128 * 4        # one fp32 partial 256x128 tile


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("libqllm_mi355x.so not built")
    return _lib.load()


def W(K, N, g=64, bits=4, layout=NATIVE, zeros=16):
    return _lib.QllmWeight(16, 16, zeros, None, None, K, N, g, bits, layout, 0)


def describe(lib, ws, m, have_ws=1):
    arr = (_lib.QllmWeight * len(ws))(*ws)
    buf = C.create_string_buffer(256)
    rc = lib.qllm_plan_describe(arr, len(ws), m, have_ws, buf, 256)
    return rc, buf.value.decode()


def plan(lib, ws, m, have_ws=1):
    rc, s = describe(lib, ws, m, have_ws)
    assert rc == 0, _lib.last_error()
    return s


@pytest.mark.parametrize("layout", [NATIVE, NATIVE_F16Z])
def test_falcon_prefill_layers_fuse_on_the_half_wide_tail(lib, layout):
    o, down, qkv = W(4544, 4544, layout=layout), W(18176, 4544, layout=layout), W(4544, 4672, layout=layout)
    # K = 4544 is 71 k-tiles: the split blocks own 35 / 36 of them (k-tile counts may differ by one on these layers)
    assert plan(lib, [o], 300) == G3 + " split_k=2 n_tail=64" + SM        # 2 x 36 tiles
    assert plan(lib, [o], 777) == G3 + " n_tail=64" + SM                   # 4 x 36 = 144 tiles: no split fits
    assert plan(lib, [o], 2048) == G3 + " tail_split=4 n_tail=64" + SM     # 288 tiles: the 32 of the ragged round split four ways
    assert plan(lib, [qkv], 2048) == G3 + " tail_split=4 n_tail=64" + SM   # 8 x 37 tiles
    assert plan(lib, [down], 100) == G3 + " split_k=4 n_tail=64" + SM      # (2^26 weights: past the panel kernel's 2^25)
    assert plan(lib, [down], 300) == G3 + " split_k=2 n_tail=64" + SM
    assert plan(lib, [down], 2048) == G3 + " tail_split=8 n_tail=64" + SM
    assert plan(lib, [W(1088, 320, layout=layout)], 300) == G3 + " split_k=2 n_tail=64" + SM
    assert plan(lib, [o], 300, have_ws=0) == G3 + " n_tail=64" + SM        # no workspace: no split, still fused


def test_falcon_batch1_layers_take_the_batch1_kernel(lib):
    assert plan(lib, [W(4544, 4544)], 1) == "strip1 nw=8 round=24 g64 grid=strips x 1" + SM   # T = 142: six live waves of 24
    assert plan(lib, [W(4544, 18176)], 1) == "strip1 nw=8 round=24 g64 grid=strips x 1" + SM
    assert plan(lib, [W(4544, 4672)], 1) == "strip1 nw=8 round=24 g64 grid=strips x 1" + SM
    assert plan(lib, [W(4544, 4544), W(4544, 64), W(4544, 64)], 1) == "strip1 nw=8 round=24 g64 grid=strips x 3" + SM  # multi-query q/k/v
    assert plan(lib, [W(1088, 320)], 1) == "strip1 nw=4 round=16 g64 grid=strips x 1" + SM
    assert plan(lib, [W(18176, 4544)], 1) == "strip1 nw=16 round=40 g64 grid=strips x 1" + SM  # (K % 128 == 0: as before)


def test_neighbouring_routes_are_unchanged(lib):
    o = W(4544, 4544)
    assert plan(lib, [o], 100) == "panel cols=64 row_tiles=8 k_halves=1 split_k=3" + SM
    assert plan(lib, [W(1088, 320)], 100) == "panel cols=64 row_tiles=8 k_halves=1 split_k=2" + SM
    for m in (2, 3, 4):   # batches 2..4: the four-row forms stay 128-wide-group only
        assert plan(lib, [o], m) == "strip nw=8 cpl=2 spw=18 form=dma-A row_tiles=1" + SM
    # 3 bits: the B3 batch-1 forms and the 3-bit prefill kernel keep K % 128 == 0 / N % 128 == 0
    assert plan(lib, [W(4544, 4544, bits=3)], 1) == "strip nw=16 cpl=1 spw=10 form=register-A row_tiles=1" + SM
    assert plan(lib, [W(4544, 4544, bits=3)], 300).startswith("unsupported (native-layout layer:")
    # grouped prefill grids keep whole 128-column tiles: a group with an odd-64 member is refused (its layers then run one by one)
    assert plan(lib, [o, W(4544, 64), W(4544, 64)], 2048).startswith("unsupported (grouped forward:")
    assert plan(lib, [W(4544, 18176), W(4544, 18176)], 2048) == G3 + " layers=2" + SM
    # widths that are not a multiple of 64
    for n in (4000, 1040):
        assert plan(lib, [W(4096, n)], 2048).startswith("unsupported (native-layout layer:")
        assert plan(lib, [W(4096, n)], 300).startswith("unsupported (native-layout layer:")
    # the reference layouts in place: the 128x128 kernel, as before
    assert plan(lib, [W(4544, 4544, layout=GPTQ)], 2048) == "gemm tile=128x128"
    assert plan(lib, [W(4544, 4544, layout=GPTQ)], 300) == "gemm tile=128x128"
    # 128-wide groups cannot tile K = 4544
    rc, _ = describe(lib, [W(4544, 4544, g=128)], 1)
    assert rc != 0 and "whole groups" in _lib.last_error()


@pytest.mark.parametrize("K,N,M,slabs", [
    (4544, 4544, 300, 2 * 36 * 2),      # split_k = 2 over 2 x 36 tiles
    (4544, 4544, 2048, 32 * 4),         # tail split: 32 tiles x 4
    (4544, 4672, 2048, 40 * 4),         # 8 x 37 = 296 tiles: 40 in the ragged round
    (18176, 4544, 100, 36 * 4),         # split_k = 4
    (18176, 4544, 2048, 32 * 8),
    (1088, 320, 300, 2 * 3 * 2),
])
def test_workspace_covers_the_new_splits(lib, K, N, M, slabs):
    w = W(K, N)
    need = COUNTERS + slabs * TILE_SLAB
    assert lib.qllm_workspace_bytes_act(C.byref(w), M, _lib.DT_F16) >= need
    # bf16 activations are served natively on these layers (no fp16 copy needed), and the bf16 size covers at least as much
    assert lib.qllm_workspace_bytes(C.byref(w), M) >= need


def test_fused_allreduce_refuses_64_wide_groups_at_k_4544(lib):
    """qllm_linear_forward_allreduce is built for 128-wide groups only; the batch-1 kernel now plans K = 4544 g64 layers, and the
    fused form must keep refusing them (UNSUPPORTED -> RowParallelQuantLinear runs the layer and the collective as two steps).  Refused
    before anything touches a device: fake, aligned pointers suffice."""
    for w in (W(4544, 4544), W(4544, 4544, layout=NATIVE_F16Z), W(18176, 4544)):
        rc = lib.qllm_linear_forward_allreduce(C.byref(w), 4096, 8192, 1, _lib.DT_F16, 12288, 0, 1, 1 << 20, None, None)
        assert rc == _lib.QLLM_ERR_UNSUPPORTED, (w.K, rc, _lib.last_error())
        assert "128-wide groups" in _lib.last_error()


@pytest.mark.parametrize("layout", [NATIVE, NATIVE_F16Z])
@pytest.mark.parametrize("K", [4096, 3584, 16384])
def test_fused_allreduce_refuses_3bit_layers(lib, layout, K):
    """The batch-1 kernel plans 3-bit native layers with 128-wide groups too, but its all-reduce instantiations are 4-bit only: the fused
    form refuses them (UNSUPPORTED, as parallel.py expects) before anything touches a device -- fake, aligned pointers suffice."""
    w = W(K, 4096, g=128, bits=3, layout=layout)
    assert plan(lib, [w], 1).startswith("strip1 ")   # (the plan the refusal must not follow)
    rc = lib.qllm_linear_forward_allreduce(C.byref(w), 4096, 8192, 1, _lib.DT_F16, 12288, 0, 1, 1 << 20, None, None)
    assert rc == _lib.QLLM_ERR_UNSUPPORTED, (K, rc, _lib.last_error())
    assert "4-bit" in _lib.last_error()
