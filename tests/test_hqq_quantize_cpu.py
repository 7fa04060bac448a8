"""The HQQ quantizer's entry points (ABI 7: qllm_hqq_quantize, qllm_hqq_quantize_workspace_bytes) on a GPU-less host: symbols,
argument validation (it runs before any device work), the workspace rule, and the planner left exactly as it was."""
import ctypes
import os

import pytest

from qllm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = 0, 1, 3


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    lib = _lib.load()
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    return lib


def _call(lib, w=16, dtype=F16, N=64, K=256, bits=4, g=64, iters=20, p=0.7, beta=10.0, kappa=1.01, qw=16, s=16, z=16, rounds=None, ws=16,
          ws_bytes=None):
    """Fake 16-byte-aligned pointers: every call below is refused before anything is dereferenced or launched."""
    if ws_bytes is None:
        ws_bytes = lib.qllm_hqq_quantize_workspace_bytes(N, K, g, iters)
    return lib.qllm_hqq_quantize(w, dtype, N, K, bits, g, iters, p, beta, kappa, qw, s, z, rounds, ws, ws_bytes, None)


def test_symbols_and_abi_version(lib):
    text = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    assert "#define QLLM_ABI_VERSION 7" in text and "QLLM_F32 = 3" in text
    for name in ("qllm_hqq_quantize", "qllm_hqq_quantize_workspace_bytes"):
        assert name in _lib.EXPORTS and name in text
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value
    assert _lib.DT_F32 == F32


def test_validation_runs_before_any_device_work(lib):
    for null in ("w", "qw", "s", "z"):
        assert _call(lib, **{null: None}) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error(), null
    assert _call(lib, bits=0) == _lib.QLLM_ERR_INVALID and "bits" in _lib.last_error()
    assert _call(lib, bits=9) == _lib.QLLM_ERR_INVALID and "bits" in _lib.last_error()
    assert _call(lib, dtype=2) == _lib.QLLM_ERR_INVALID and "w_dtype" in _lib.last_error()
    assert _call(lib, iters=0, ws_bytes=1 << 20) == _lib.QLLM_ERR_INVALID
    assert _call(lib, iters=65, ws_bytes=1 << 20) == _lib.QLLM_ERR_INVALID
    assert _call(lib, w=24) == _lib.QLLM_ERR_INVALID and "aligned" in _lib.last_error()
    # valid requests the kernel does not serve
    for kw in (dict(bits=5), dict(bits=6), dict(bits=7), dict(K=224), dict(g=48, K=240), dict(g=16), dict(g=2048, K=4096), dict(N=72),
               dict(p=1.0)):
        assert _call(lib, ws_bytes=1 << 20, **kw) == _lib.QLLM_ERR_UNSUPPORTED, kw
        assert _lib.last_error()
    # the workspace: NULL, or one byte short
    need = lib.qllm_hqq_quantize_workspace_bytes(64, 256, 64, 20)
    assert _call(lib, ws=None) == _lib.QLLM_ERR_WORKSPACE
    assert _call(lib, ws_bytes=need - 1) == _lib.QLLM_ERR_WORKSPACE and str(need) in _lib.last_error()
    with pytest.raises(_lib.QllmUnsupported):
        _lib.check(_call(lib, bits=5))


def test_workspace_bytes_is_a_pure_function_of_the_shape(lib):
    f = lib.qllm_hqq_quantize_workspace_bytes
    # header (1 KB) + one fp32 error sum per block and round; a block per 16-row x one-group tile, at most 2048 blocks
    assert f(64, 256, 64, 20) == 1024 + (64 // 16) * (256 // 64) * 20 * 4
    assert f(48, 384, 128, 20) == 1024 + 3 * 3 * 20 * 4
    assert f(64, 256, 64, 5) == 1024 + 16 * 5 * 4
    assert f(4096, 4096, 64, 20) == f(4096, 11008, 64, 20) == 1024 + 2048 * 20 * 4
    assert [f(4096, 4096, 128, 20) for _ in range(3)] == [1024 + 2048 * 80] * 3
    assert f(64, 250, 64, 20) == 0 and f(60, 256, 64, 20) == 0 and f(64, 256, 64, 0) == 0 and f(64, 256, 64, 65) == 0


PLANS = [   # (K, N, group_size, bits, layout, M) -> qllm_plan_describe before this entry point existed
    ((4096, 4096, 128, 4, 0, 1), "strip nw=16 cpl=1 spw=8 form=lds-slab row_tiles=1"),
    ((4096, 4096, 64, 3, 2, 1), "strip nw=16 cpl=1 spw=8 form=lds-slab row_tiles=1"),
    ((4096, 11008, 64, 4, 4, 16), "strip nw=8 cpl=3 spw=16 form=dma-A row_tiles=1 layout=strip-major"),
    ((4096, 4096, 128, 4, 3, 512), "gemm2 tile=256x128 split_k=4 layout=strip-major"),
    ((256, 128, 64, 2, 2, 1), "bitgemv bits=2 cols=32 waves=8 split_k=1"),
    ((256, 128, 64, 8, 2, 1), "bitgemv bits=8 cols=32 waves=8 split_k=1"),
    ((256, 128, 64, 3, 4, 1), "strip1 nw=4 round=8 g64 bits=3 grid=strips x 1 layout=strip-major"),
    ((256, 128, 64, 4, 4, 33), "panel cols=64 row_tiles=4 k_halves=2 split_k=1 layout=strip-major"),
    ((4096, 4096, 128, 5, 0, 64), "unsupported (no fused kernel for bits=5 K=4096 N=4096 g=128 layout=0 act_order=0; use qllm_dequant + GEMM)"),
    ((4096, 4096, 128, 4, 1, 2048), "gemm3 tile=256x128 matrix-waves=8 staging-waves=4"),
]


@pytest.mark.parametrize("desc,plan", PLANS)
def test_existing_plans_are_unchanged(lib, desc, plan):
    K, N, g, bits, layout, M = desc
    w = _lib.QllmWeight(16, 16, 16, None, None, K, N, g, bits, layout, 0)
    buf = ctypes.create_string_buffer(256)
    assert lib.qllm_plan_describe(ctypes.byref(w), 1, M, 1, buf, 256) == 0
    assert buf.value.decode() == plan


def test_python_entry_points_refuse_cpu_tensors(lib):
    import torch
    from qllm_amd.quantization import hqq_quantize_weight
    with pytest.raises(RuntimeError, match="no CPU quantizer"):
        hqq_quantize_weight(torch.zeros(64, 256, dtype=torch.float16), 4, 64)
    with pytest.raises(TypeError):
        hqq_quantize_weight(torch.zeros(64, 256, dtype=torch.float16), 4, 64, rounds=3)
