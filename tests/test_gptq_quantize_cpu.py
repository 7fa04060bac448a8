"""The GPTQ quantizer's entry points (qllm_gptq_quantize, qllm_gptq_quantize_workspace_bytes) on a GPU-less host: symbols, argument
validation (it runs before any device work), the workspace rule, and the torch plumbing that needs no device."""
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
    return _lib.load()


def _call(lib, w=16, dtype=F16, u=16, N=64, K=256, bits=4, g=128, sym=0, codes=16, s=16, z=16, wq=16, loss=16, ws=16, ws_bytes=None):
    """Fake aligned pointers: every call below is refused before anything is dereferenced or launched."""
    if ws_bytes is None:
        ws_bytes = lib.qllm_gptq_quantize_workspace_bytes(N, K)
    return lib.qllm_gptq_quantize(w, dtype, u, N, K, bits, g, sym, codes, s, z, wq, loss, ws, ws_bytes, None)


def test_symbols_exist_and_the_abi_version_is_unchanged(lib):
    text = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    assert "#define QLLM_ABI_VERSION 7" in text and lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("qllm_gptq_quantize", "qllm_gptq_quantize_workspace_bytes"):
        assert name in _lib.EXPORTS and name in text
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value


def test_workspace_bytes_is_pure_and_monotone(lib):
    f = lib.qllm_gptq_quantize_workspace_bytes
    assert f(64, 256) == 64 * 256 * 4                       # the fp32 error history of every row, rounded up to 256 bytes
    assert f(48, 320) == 48 * 320 * 4 and f(1, 1) == 256
    assert [f(4096, 11008) for _ in range(3)] == [4096 * 11008 * 4] * 3
    assert f(0, 256) == 0 and f(64, 0) == 0 and f(-1, 256) == 0
    sizes = [f(n, k) for n in (1, 16, 17, 64, 4096) for k in (32, 128, 320, 4096)]
    assert all(f(n + 1, k) >= f(n, k) and f(n, k + 32) >= f(n, k) for n in (1, 16, 17, 64, 4096) for k in (32, 128, 320, 4096))
    assert all(s > 0 and s % 256 == 0 for s in sizes)


def test_validation_runs_before_any_device_work(lib):
    for null in ("w", "codes", "s", "z"):
        assert _call(lib, **{null: None}) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error(), null
    assert _call(lib, dtype=2) == _lib.QLLM_ERR_INVALID and "w_dtype" in _lib.last_error()
    assert _call(lib, N=0) == _lib.QLLM_ERR_INVALID and _call(lib, K=-4, ws_bytes=1 << 20) == _lib.QLLM_ERR_INVALID
    assert _call(lib, sym=2) == _lib.QLLM_ERR_INVALID and "sym" in _lib.last_error()
    # widths other than 2..8, groups other than 32 / 64 / 128 / K
    for kw in (dict(bits=1), dict(bits=9), dict(bits=0), dict(g=48, K=240), dict(g=16), dict(g=256, K=512), dict(g=96, K=384)):
        assert _call(lib, ws_bytes=1 << 22, **kw) == _lib.QLLM_ERR_UNSUPPORTED, kw
        assert "bits 2..8" in _lib.last_error() and "32 / 64 / 128 / K" in _lib.last_error()
    with pytest.raises(_lib.QllmUnsupported):
        _lib.check(_call(lib, bits=9))
    # an allowed group that does not divide K
    assert _call(lib, K=224, g=64) == _lib.QLLM_ERR_INVALID and "multiple of group_size" in _lib.last_error()
    assert _call(lib, K=320, g=128) == _lib.QLLM_ERR_INVALID
    # optional pointers may be NULL, group_size == K is served: these reach the workspace check, the last one before a launch
    for kw in (dict(u=None), dict(wq=None), dict(loss=None), dict(g=256), dict(K=320, g=64), dict(dtype=F32), dict(dtype=BF16)):
        assert _call(lib, ws=None, **kw) == _lib.QLLM_ERR_WORKSPACE, kw
    assert _call(lib, w=18, dtype=F32) == _lib.QLLM_ERR_INVALID and "aligned" in _lib.last_error()
    assert _call(lib, u=18) == _lib.QLLM_ERR_INVALID and _call(lib, codes=18) == _lib.QLLM_ERR_INVALID
    # U's tiles are read four floats at a time: a 16-byte aligned u_kk, and (reachable with group_size == K only) K % 4 == 0
    assert _call(lib, u=24) == _lib.QLLM_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert _call(lib, K=250, g=250) == _lib.QLLM_ERR_INVALID and "multiple of 4" in _lib.last_error()
    # the workspace: NULL, misaligned, one byte short
    need = lib.qllm_gptq_quantize_workspace_bytes(64, 256)
    assert _call(lib, ws=None) == _lib.QLLM_ERR_WORKSPACE
    assert _call(lib, ws=24) == _lib.QLLM_ERR_WORKSPACE and "16-byte aligned" in _lib.last_error()
    assert _call(lib, ws_bytes=need - 1) == _lib.QLLM_ERR_WORKSPACE and str(need) in _lib.last_error()


def test_python_entry_points_refuse_cpu_tensors(lib):
    import torch
    from qllm_amd.quantization import gptq_quantize_weight
    from qllm_amd.quantization.gptq import quantize_linear
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X: qllm_amd ships no CPU quantizer"):
        gptq_quantize_weight(torch.zeros(64, 256, dtype=torch.float16), None, 4, 128)
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X"):
        gptq_quantize_weight(torch.zeros(64, 256, dtype=torch.float16), torch.eye(256), 4, 128, act_order=True)
    assert callable(quantize_linear)


def test_accumulate_hessian_is_the_running_mean_of_2_xtx():
    import torch
    from qllm_amd.quantization import accumulate_hessian
    gen = torch.Generator().manual_seed(0)
    x = torch.randn((5, 7, 24), generator=gen, dtype=torch.float64)
    H, n = torch.zeros((24, 24), dtype=torch.float64), 0
    for b in range(5):
        H, n = accumulate_hessian(H, n, x[b])                 # one batch of 7 tokens at a time
    X = x.reshape(-1, 24)
    assert n == 5 and torch.allclose(H, 2.0 / 5 * X.T @ X, rtol=1e-13, atol=1e-13)
    H3, n3 = accumulate_hessian(None, 0, x[:2].float())       # a [batch, tokens, K] tensor counts its batches; fp32 by default
    H3, n3 = accumulate_hessian(H3, n3, x[2:].float())
    assert n3 == 5 and H3.dtype == torch.float32 and torch.allclose(H3.double(), H, rtol=1e-5, atol=1e-5)


def test_quant_config_round_trips_desc_act_and_sym(tmp_path):
    import json
    from qllm_amd.modeling import base
    cfg = base.QuantConfig(bits=4, group_size=128, version="GPTQ", quant_method="gptq", desc_act=True, sym=True)
    json.dump(cfg.to_dict(), open(tmp_path / "quantize_config.json", "w"))
    back = base.QuantConfig.from_dir(str(tmp_path))
    assert back.desc_act and back.sym and back.version == "GPTQ" and not back.compatible_with_autogptq
    assert "desc_act" not in base.QuantConfig().to_dict() and "sym" not in base.QuantConfig().to_dict()
