"""The static-groups GPTQ entry point (qllm_gptq_quantize_static, csrc/gptq_static.hip) on a GPU-less host: the symbol, argument
validation (it runs before any device work), the kernel's resources read from the gfx950 code object, and the Python plumbing that
needs no device."""
import ctypes
import os

import pytest

from kernel_resources import resources
from qllm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = 0, 1, 3


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _call(lib, w=16, dtype=F16, u=16, perm=16, N=64, K=256, bits=4, g=128, sym=0, codes=16, s=16, z=16, wq=16, loss=16, ws=16, ws_bytes=None):
    """Fake aligned pointers: every call below is refused before anything is dereferenced or launched."""
    if ws_bytes is None:
        ws_bytes = lib.qllm_gptq_quantize_workspace_bytes(N, K)
    return lib.qllm_gptq_quantize_static(w, dtype, u, perm, N, K, bits, g, sym, codes, s, z, wq, loss, ws, ws_bytes, None)


def test_symbol_is_exported_and_declared_and_the_abi_version_is_unchanged(lib):
    text = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    assert "#define QLLM_ABI_VERSION 7" in text and lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert "qllm_gptq_quantize_static" in _lib.EXPORTS and "int qllm_gptq_quantize_static(" in text
    assert ctypes.cast(lib.qllm_gptq_quantize_static, ctypes.c_void_p).value
    assert len(lib.qllm_gptq_quantize_static.argtypes) == len(lib.qllm_gptq_quantize.argtypes) + 1      # perm_k


def test_validation_runs_before_any_device_work(lib):
    for null in ("w", "codes", "s", "z"):
        assert _call(lib, **{null: None}) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error(), null
    assert _call(lib, dtype=2) == _lib.QLLM_ERR_INVALID and "w_dtype" in _lib.last_error()
    assert _call(lib, N=0) == _lib.QLLM_ERR_INVALID and _call(lib, K=-4, ws_bytes=1 << 20) == _lib.QLLM_ERR_INVALID
    assert _call(lib, sym=2) == _lib.QLLM_ERR_INVALID and "sym" in _lib.last_error()
    # widths other than 2..8, groups other than 32 / 64 / 128 / K
    for kw in (dict(bits=1), dict(bits=9), dict(g=48, K=240), dict(g=16), dict(g=256, K=512), dict(g=96, K=384)):
        assert _call(lib, ws_bytes=1 << 22, **kw) == _lib.QLLM_ERR_UNSUPPORTED, kw
        assert "bits 2..8" in _lib.last_error() and "32 / 64 / 128 / K" in _lib.last_error()
    with pytest.raises(_lib.QllmUnsupported):
        _lib.check(_call(lib, bits=9))
    # an allowed group that does not divide K
    assert _call(lib, K=224, g=64) == _lib.QLLM_ERR_INVALID and "multiple of group_size" in _lib.last_error()
    assert _call(lib, K=320, g=128) == _lib.QLLM_ERR_INVALID
    # optional pointers may be NULL (perm_k: the identity), group_size == K and a ragged last column block are served: these reach the
    # workspace check, the last one before a launch
    for kw in (dict(u=None), dict(perm=None), dict(u=None, perm=None), dict(wq=None), dict(loss=None), dict(g=256), dict(K=320, g=64),
               dict(dtype=F32), dict(dtype=BF16), dict(bits=2), dict(bits=8), dict(g=32, N=48)):
        assert _call(lib, ws=None, **kw) == _lib.QLLM_ERR_WORKSPACE, kw
    assert _call(lib, w=18, dtype=F32) == _lib.QLLM_ERR_INVALID and "aligned" in _lib.last_error()
    assert _call(lib, codes=18) == _lib.QLLM_ERR_INVALID and _call(lib, perm=18) == _lib.QLLM_ERR_INVALID and "perm_k" in _lib.last_error()
    # U's tiles are read four floats at a time: a 16-byte aligned u_kk, and (reachable with group_size == K only) K % 4 == 0
    assert _call(lib, u=24) == _lib.QLLM_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert _call(lib, K=250, g=250) == _lib.QLLM_ERR_INVALID and "multiple of 4" in _lib.last_error()
    # the workspace is qllm_gptq_quantize's: NULL, misaligned, one byte short
    need = lib.qllm_gptq_quantize_workspace_bytes(64, 256)
    assert _call(lib, ws=None) == _lib.QLLM_ERR_WORKSPACE and "qllm_gptq_quantize_static" in _lib.last_error()
    assert _call(lib, ws=24) == _lib.QLLM_ERR_WORKSPACE and "16-byte aligned" in _lib.last_error()
    assert _call(lib, ws_bytes=need - 1) == _lib.QLLM_ERR_WORKSPACE and str(need) in _lib.last_error()


def test_python_entry_points_refuse_cpu_tensors(lib):
    import torch
    from qllm_amd import ops
    from qllm_amd.quantization import gptq_quantize_weight
    from qllm_amd.quantization.gptq import quantize_linear
    w = torch.zeros(64, 256, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X: qllm_amd ships no CPU quantizer"):
        gptq_quantize_weight(w, None, 4, 128, static_groups=True)
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X"):
        gptq_quantize_weight(w, torch.eye(256), 4, 128, act_order=True, static_groups=True)
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X"):
        quantize_linear(torch.nn.Linear(256, 64, bias=False).half(), None, 4, 128, device="cpu", static_groups=True)
    with pytest.raises(RuntimeError):
        ops.gptq_quantize_static(w, None, None, 4, 128)
    assert "gptq_quantize_static" in ops.__all__


def test_three_kernels_two_blocks_per_cu_without_scratch():
    """The decomposition is gptq_quant.hip's (test_gptq_quant_resources_cpu.py): one 128 x 128 fp32 tile of U and one 16 x (128 + 4)
    tile in LDS, two blocks per CU.  The group table lives in the output arrays, not in LDS; the eight (scale, zero) pairs, the eight
    original columns and everything else a lane carries through a column block stay in registers."""
    res = {n: v for n, v in resources("gptq_static.hip").items() if "gptq_static_kernel" in n}
    assert len(res) == 3, sorted(res)                       # fp16, bf16, fp32
    for n, r in res.items():
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["group_segment_fixed_size"] * 2 <= 160 * 1024, (n, r)
        assert r["vgpr_count"] <= 256, (n, r)


def test_quant_config_round_trips_static_groups(tmp_path):
    import json
    from qllm_amd.modeling import base
    cfg = base.QuantConfig(bits=4, group_size=128, version="GPTQ", quant_method="gptq", desc_act=True, static_groups=True)
    d = cfg.to_dict()
    assert d["static_groups"] is True and d["desc_act"] is True
    json.dump(d, open(tmp_path / "quantize_config.json", "w"))
    back = base.QuantConfig.from_dir(str(tmp_path))
    assert back.static_groups and back.desc_act and back.version == "GPTQ"
    assert "static_groups" not in base.QuantConfig().to_dict()                      # written only when set
    assert "static_groups" not in base.QuantConfig(desc_act=True).to_dict()
    json.dump(base.QuantConfig(desc_act=True).to_dict() | {"version": "GPTQ"}, open(tmp_path / "quantize_config.json", "w"))
    assert not base.QuantConfig.from_dir(str(tmp_path)).static_groups
