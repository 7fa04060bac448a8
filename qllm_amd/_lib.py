"""ctypes binding of libqllm_mi355x.so (the C ABI declared in include/qllm_mi355x.h).

This is the only place the shared library is touched.  There is no CPU / eager fallback: if the library is missing
or the device is not gfx950, every hot-path entry point raises.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libqllm_mi355x.so"
LIB_PATH = os.environ.get("QLLM_MI355X_LIB") or os.path.join(_HERE, LIB_NAME)  # override: A/B-testing kernel builds

QLLM_OK, QLLM_ERR_INVALID, QLLM_ERR_UNSUPPORTED, QLLM_ERR_WORKSPACE, QLLM_ERR_LAUNCH, QLLM_ERR_DEVICE = range(6)
LAYOUT_GPTQ, LAYOUT_AWQ_GEMM, LAYOUT_HQQ, LAYOUT_NATIVE, LAYOUT_NATIVE_F16Z = 0, 1, 2, 3, 4
DT_F16, DT_BF16, DT_F16_IN_BF16_OUT, DT_F32 = 0, 1, 2, 3
ABI_VERSION = 7
BITPANEL_MAX_M_DEFAULT = 256   # QLLM_BITPANEL_MAX_M_DEFAULT of include/qllm_mi355x.h: the measured line of profiles/bitpanel.md (0: modules do not route)
BITGEMM_MIN_M_DEFAULT = 0      # QLLM_BITGEMM_MIN_M_DEFAULT of include/qllm_mi355x.h: the measured line of profiles/bitgemm.md (0: modules do not route)
ATTN_MASK_NONE, ATTN_MASK_BOOL, ATTN_MASK_ADDITIVE = 0, 1, 2   # QLLM_ATTN_MASK_* of include/qllm_mi355x.h (qllm_attn_decode)
ACT_SILU = 0                   # QLLM_ACT_SILU of include/qllm_mi355x.h (qllm_linear_forward_swiglu)
BITGROUP_MAX_M_DEFAULT = 16    # QLLM_BITGROUP_MAX_M_DEFAULT of include/qllm_mi355x.h: the measured line of profiles/bitgemv_group.md (0: sibling groups do not route)


class QllmWeight(C.Structure):
    """struct qllm_weight (include/qllm_mi355x.h)."""
    _fields_ = [
        ("qweight", C.c_void_p), ("scales", C.c_void_p), ("qzeros", C.c_void_p), ("g_idx", C.c_void_p),
        ("bias", C.c_void_p),
        ("K", C.c_int32), ("N", C.c_int32), ("group_size", C.c_int32), ("bits", C.c_int32),
        ("layout", C.c_int32), ("add_zero_bias", C.c_int32),
    ]


class QllmDeviceInfo(C.Structure):
    _fields_ = [
        ("arch", C.c_char * 32), ("compute_units", C.c_int32), ("wavefront_size", C.c_int32),
        ("lds_bytes_per_cu", C.c_int32), ("clock_khz", C.c_int32), ("hbm_bytes", C.c_int64),
    ]


# The C ABI as ctypes sees it: name -> (restype, argtypes).  The ONE list of symbols: EXPORTS (what
# tests/test_capi_symbols.py holds against include/qllm_mi355x.h) is its keys and _declare() walks it, so no symbol can be exported
# without argtypes -- ctypes would pass its 64-bit pointers as C int.
vp, i32, i64, sz = C.c_void_p, C.c_int32, C.c_int64, C.c_size_t
wp = C.POINTER(QllmWeight)
SIGNATURES = {
    "qllm_abi_version": (C.c_int, []),
    "qllm_is_lab_build": (C.c_int, []),
    "qllm_last_error": (C.c_char_p, []),
    "qllm_device_info": (C.c_int, [C.c_int, C.POINTER(QllmDeviceInfo)]),
    "qllm_workspace_bytes": (sz, [wp, i32]),
    "qllm_workspace_bytes_act": (sz, [wp, i32, i32]),
    "qllm_workspace_init": (C.c_int, [vp, sz, vp]),
    "qllm_linear_forward": (C.c_int, [wp, vp, vp, i32, i32, vp, sz, vp]),
    "qllm_linear_forward_grouped": (C.c_int, [wp, C.POINTER(vp), i32, vp, i32, i32, vp, sz, vp]),
    "qllm_dequant": (C.c_int, [wp, vp, i32, i32, vp]),
    "qllm_ort_gemv": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, i32, i32, vp, sz, vp]),
    "qllm_ort_dequant": (C.c_int, [vp, vp, vp, vp, i32, i32, i32, i32, vp, i32, vp]),
    "qllm_awq_gemm_forward": (C.c_int, [vp, vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, vp, sz, vp]),
    "qllm_unpack_qweight": (C.c_int, [vp, i32, i32, i32, i32, vp, vp]),
    "qllm_pack_qweight": (C.c_int, [vp, i32, i32, i32, i32, vp, vp]),
    "qllm_gather_columns": (C.c_int, [vp, vp, vp, i32, i32, i32, vp]),
    "qllm_gather_describe": (C.c_int, [i32, i32, C.c_char_p, sz]),
    "qllm_ort_dequantize4bits": (C.c_int, [vp, vp, vp, i32, vp, i32, i32, i32, vp, vp]),
    "qllm_plan_describe": (C.c_int, [wp, i32, i32, i32, C.c_char_p, sz]),
    "qllm_debug_timeline": (C.c_int, [vp, i32]),
    "qllm_native_sizes": (C.c_int, [wp, C.POINTER(sz), C.POINTER(sz), C.POINTER(sz)]),
    "qllm_repack_native": (C.c_int, [wp, vp, vp, vp, vp]),
    "qllm_unpack_native": (C.c_int, [wp, i32, vp, vp, vp, vp]),
    "qllm_comm_buffer_bytes": (sz, [i32, sz]),
    "qllm_comm_alloc": (C.c_int, [sz, C.POINTER(vp)]),
    "qllm_comm_free": (C.c_int, [vp]),
    "qllm_comm_export": (C.c_int, [vp, vp]),
    "qllm_comm_import": (C.c_int, [vp, C.POINTER(vp)]),
    "qllm_comm_close": (C.c_int, [vp]),
    "qllm_allreduce_oneshot": (C.c_int, [vp, i32, i32, vp, i32, i32, sz, vp, vp]),
    "qllm_linear_forward_allreduce": (C.c_int, [wp, vp, vp, i32, i32, vp, i32, i32, sz, vp, vp]),
    "qllm_convert_bf16_to_f16": (C.c_int, [vp, vp, sz, vp]),
    "qllm_set_knob": (C.c_int, [C.c_char_p, i32]),
    "qllm_get_knob": (C.c_int, [C.c_char_p, C.POINTER(i32), C.POINTER(i32)]),
    "qllm_reset_knobs": (None, []),
    "qllm_hqq_quantize_workspace_bytes": (sz, [i32, i32, i32, i32]),
    "qllm_hqq_quantize": (C.c_int, [vp, i32, i32, i32, i32, i32, i32, C.c_float, C.c_float, C.c_float, vp, vp, vp, vp, vp, sz, vp]),
    "qllm_gptq_quantize_workspace_bytes": (sz, [i32, i32]),
    "qllm_gptq_quantize": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "qllm_gptq_quantize_static": (C.c_int, [vp, i32, vp, vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, sz, vp]),
    "qllm_linear_forward_permuted": (C.c_int, [wp, vp, vp, vp, i32, i32, vp, sz, vp]),
    "qllm_linear_forward_bitpanel": (C.c_int, [wp, vp, vp, i32, i32, vp, sz, vp]),
    "qllm_bitpanel_workspace_bytes": (sz, [wp, i32]),
    "qllm_bitpanel_describe": (C.c_int, [wp, i32, i32, C.c_char_p, sz]),
    "qllm_linear_forward_bitgroup": (C.c_int, [wp, C.POINTER(vp), i32, vp, i32, i32, vp, sz, vp]),
    "qllm_bitgroup_workspace_bytes": (sz, [wp, i32, i32]),
    "qllm_bitgroup_describe": (C.c_int, [wp, i32, i32, i32, C.c_char_p, sz]),
    "qllm_linear_forward_bitgemm": (C.c_int, [wp, vp, vp, i32, i32, vp, sz, vp]),
    "qllm_bitgemm_workspace_bytes": (sz, [wp, i32]),
    "qllm_bitgemm_describe": (C.c_int, [wp, i32, i32, C.c_char_p, sz]),
    "qllm_awq_clip_search_workspace_bytes": (sz, [i32, i32, i32]),
    "qllm_awq_clip_search": (C.c_int, [vp, i32, vp, i32, i32, i32, i32, i32, C.c_float, vp, vp, vp, vp, sz, vp]),
    "qllm_awq_quantize": (C.c_int, [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]),
    "qllm_linear_forward_swiglu": (C.c_int, [wp, vp, vp, vp, i32, i32, i32, vp]),
    "qllm_swiglu_describe": (C.c_int, [wp, i32, C.c_char_p, sz]),
    "qllm_rmsnorm": (C.c_int, [vp, vp, vp, i32, i32, C.c_float, i32, vp, vp]),
    "qllm_linear_forward_rmsnorm": (C.c_int, [wp, C.POINTER(vp), i32, vp, vp, C.c_float, i32, i32, vp, vp]),
    "qllm_rmsnorm_describe": (C.c_int, [wp, i32, i32, C.c_char_p, sz]),
    "qllm_linear_forward_residual": (C.c_int, [wp, vp, vp, vp, vp, i32, i32, i32, vp]),
    "qllm_residual_describe": (C.c_int, [wp, i32, i32, C.c_char_p, sz]),
    "qllm_rope": (C.c_int, [vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, i64, i64, i64, i32, i32, vp]),
    "qllm_attn_decode": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i32, i64, i64,
                                   C.c_float, i32, vp, sz, vp]),
    "qllm_attn_decode_workspace_bytes": (sz, [i32, i32, i32, i32, i64]),
    "qllm_attn_decode_describe": (C.c_int, [i32, i32, i32, i32, i64, C.c_char_p, sz]),
    "qllm_attn_prefill": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, vp, i64, i64, i64, i64, i64, i64, i64, i32, i64, i64, i64, i32,
                                    C.c_float, i32, vp]),
    "qllm_attn_prefill_describe": (C.c_int, [i32, i32, i32, i32, i32, i64, C.c_char_p, sz]),
    "qllm_attn_decode_window": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i32,
                                          i64, i64, C.c_float, i32, vp, sz, vp]),
    "qllm_attn_prefill_window": (C.c_int, [vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, vp, i64, i64, i64, i64, i64, i64, i64, i64, i32, i64, i64, i64,
                                           i32, C.c_float, i32, vp]),
    "qllm_attn_decode_ring": (C.c_int, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i64, vp, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i64, i32,
                                        i64, i64, C.c_float, i32, vp, sz, vp]),
}
EXPORTS = tuple(SIGNATURES)


class QllmError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"qllm_mi355x error {code}: {msg}")
        self.code = code


class QllmUnsupported(QllmError):
    pass


_lib = None
_lock = threading.Lock()


def _declare(lib):
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes


def is_built() -> bool:
    return os.path.exists(LIB_PATH)


def load():
    """dlopen the in-tree library (once).  Raises if it has not been built -- there is no fallback."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise RuntimeError(
                    f"{LIB_NAME} is not built (expected {LIB_PATH}). Run `python -c 'import __graft_entry__ as g; "
                    f"g.build()'` or `make -C qllm_amd/csrc`. qllm_amd has no CPU fallback for the forward path.")
            lib = C.CDLL(LIB_PATH)
            _declare(lib)
            v = lib.qllm_abi_version()
            if v != ABI_VERSION:
                raise RuntimeError(f"{LIB_NAME} ABI version {v} != expected {ABI_VERSION}; rebuild it")
            _lib = lib
    return _lib


def last_error() -> str:
    return (load().qllm_last_error() or b"").decode("utf-8", "replace")


def check(rc: int):
    if rc == QLLM_OK:
        return
    msg = last_error()
    if rc == QLLM_ERR_UNSUPPORTED:
        raise QllmUnsupported(rc, msg)
    raise QllmError(rc, msg)


def device_info(device: int = 0) -> dict:
    info = QllmDeviceInfo()
    check(load().qllm_device_info(int(device), C.byref(info)))
    return dict(arch=info.arch.decode(), compute_units=info.compute_units, wavefront_size=info.wavefront_size,
                lds_bytes_per_cu=info.lds_bytes_per_cu, clock_khz=info.clock_khz, hbm_bytes=info.hbm_bytes)
