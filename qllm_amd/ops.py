"""torch-facing wrappers over the C ABI: pass data_ptr()s + the current HIP stream, allocate outputs and the
split-K workspace with torch's caching allocator (the library itself never allocates).

PyTorch is plumbing here (device memory, streams); all compute is in libqllm_mi355x.so.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (DT_BF16, DT_F16, LAYOUT_AWQ_GEMM, LAYOUT_GPTQ, LAYOUT_HQQ, LAYOUT_NATIVE, LAYOUT_NATIVE_F16Z, QllmError,
                   QllmUnsupported, QllmWeight)

LAYOUTS = {"GPTQ": LAYOUT_GPTQ, "GEMM": LAYOUT_AWQ_GEMM, "AWQ": LAYOUT_AWQ_GEMM, "HQQ": LAYOUT_HQQ, "NATIVE": LAYOUT_NATIVE,
           "NATIVE_F16Z": LAYOUT_NATIVE_F16Z}

_workspaces: dict = {}


def _check_input(t: torch.Tensor, name: str):
    # the reference's CHECK_INPUT (csrc/ort_cuda/ort_ops.cc:6-10): device tensor, contiguous
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a HIP/CUDA tensor (qllm_amd has no CPU forward path)")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def _act_dtype(t: torch.Tensor) -> int:
    if t.dtype == torch.float16:
        return DT_F16
    if t.dtype == torch.bfloat16:
        return DT_BF16
    raise RuntimeError(f"activations must be float16 or bfloat16, got {t.dtype}")


WORKSPACE_BYTES = 64 << 20


def workspace(device: torch.device, nbytes: int) -> torch.Tensor:
    """Per-(device, stream) scratch for split-K slabs + arrival counters; zero-filled once (kernels leave it clean).
    The key uses the CURRENT stream of `device` (not of whatever device happens to be current).

    The persistent buffer is 64 MB and NEVER moves or grows: hipGraphs captured earlier hold its address (arrival counters,
    split-K slabs).  Counters + slabs are bounded by 16 KB + 32 MB for every shape; only the fp16 staging copy of a bf16
    activation (M * K * 2 bytes, dtype-aware sizing: qllm_workspace_bytes_act) can ask for more -- such a call gets a buffer of
    its own from torch's caching allocator (inside a capture: from the graph's private pool, i.e. static for that graph), with
    its counter page zeroed on the call's stream."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    key = (idx, torch.cuda.current_stream(idx).cuda_stream)
    ws = _workspaces.get(key)
    if ws is None:
        ws = _workspaces[key] = torch.zeros(WORKSPACE_BYTES, dtype=torch.uint8, device=device)
    if nbytes <= ws.numel():
        return ws
    big = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
    big[:16384].zero_()
    return big


def make_weight(layout: str, qweight, scales, qzeros, g_idx, bias, in_features: int, out_features: int,
                group_size: int, bits: int, add_zero_bias: int = 0):
    """Build the C descriptor.  Returns (QllmWeight, keepalive tuple of tensors whose pointers it holds)."""
    lay = LAYOUTS[layout.upper()]
    for name, t in (("qweight", qweight), ("scales", scales)):
        _check_input(t, name)
    if scales.dtype != torch.float16:
        raise RuntimeError("scales must be float16 at the C boundary (cast bf16 scales once, like ort_ops.cc:79-90)")
    if qweight.dtype != torch.int32:
        raise RuntimeError("qweight must be int32")
    if qzeros is not None:
        _check_input(qzeros, "qzeros")
        want = torch.float16 if lay in (LAYOUT_HQQ, LAYOUT_NATIVE_F16Z) else torch.int32
        if qzeros.dtype != want:
            raise RuntimeError(f"qzeros must be {want} for layout {layout}")
    if g_idx is not None:
        _check_input(g_idx, "g_idx")
        if g_idx.dtype != torch.int32:
            raise RuntimeError("g_idx must be int32")
    if bias is not None:
        _check_input(bias, "bias")
        if bias.dtype != torch.float16:
            raise RuntimeError("bias must be float16 at the C boundary")
    w = QllmWeight(
        qweight.data_ptr(), scales.data_ptr(), qzeros.data_ptr() if qzeros is not None else None,
        g_idx.data_ptr() if g_idx is not None else None, bias.data_ptr() if bias is not None else None,
        int(in_features), int(out_features), int(group_size), int(bits), lay, int(add_zero_bias))
    return w, (qweight, scales, qzeros, g_idx, bias)


def _check_x(x2d: torch.Tensor, ws_desc: Sequence[QllmWeight]):
    _check_input(x2d, "x")
    if x2d.dim() != 2:
        raise RuntimeError(f"x must be 2-D [M, K], got {tuple(x2d.shape)}")
    for w in ws_desc:
        if x2d.shape[1] != w.K:
            raise RuntimeError(f"x must be [M, {w.K}], got {tuple(x2d.shape)}")


def _check_out(o: torch.Tensor, m: int, n_cols: int, x2d: torch.Tensor):
    if o.device != x2d.device or o.dtype != x2d.dtype or tuple(o.shape) != (m, n_cols) or not o.is_contiguous():
        raise RuntimeError(f"out must be a contiguous [{m}, {n_cols}] {x2d.dtype} tensor on {x2d.device}, "
                           f"got {tuple(o.shape)} {o.dtype} on {o.device}")


def _forward(ws_desc: Sequence[QllmWeight], x2d: torch.Tensor, outs, size, call, many: bool = False, prepare=None):
    """The body every forward wrapper shares.  One descriptor: `outs` is the caller's output or None, and the output is returned; with
    `many`, `outs` is a sequence of outputs, one per descriptor, or None, and a sequence is returned.  The outputs are checked (None:
    allocated, [M, w.N] of x2d's type), zero rows return without a library call, then inside x2d's device the workspace is fetched --
    `size(w_ref, m, dt)` bytes; None: the entry takes no workspace -- and `call(w_ref, y_ref, x, m, dt, ws)` makes the library call,
    whose status is checked.  w_ref / y_ref: `byref(w)` and the output's pointer, or with `many` the descriptor array and the array of
    output pointers; dt: x2d's type for the library.  `prepare()`: what a wrapper does once the outputs are checked and before anything
    is allocated (also at zero rows); it returns the tensor passed as x instead of x2d."""
    m = x2d.shape[0]
    if outs is not None:
        if many and len(outs) != len(ws_desc):
            raise RuntimeError(f"outs must hold {len(ws_desc)} tensors, got {len(outs)}")
        for o, w in zip(outs if many else (outs,), ws_desc):
            _check_out(o, m, w.N, x2d)
    x = x2d if prepare is None else prepare()
    if outs is None:
        outs = [torch.empty((m, w.N), dtype=x2d.dtype, device=x2d.device) for w in ws_desc]
        outs = outs if many else outs[0]
    if m == 0:
        return outs
    if many:
        w_ref, y_ref = _array(ws_desc), (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    else:
        w_ref, y_ref = C.byref(ws_desc[0]), outs.data_ptr()
    dt = _act_dtype(x2d)
    with torch.cuda.device(x2d.device):
        rc = call(w_ref, y_ref, x, m, dt, workspace(x2d.device, size(w_ref, m, dt)) if size is not None else None)
    if rc:
        _lib.check(rc)
    return outs


def _describe(symbol: str, buflen: int, *args) -> str:
    """A *_describe entry's text: `args` are its arguments in front of the buffer."""
    buf = C.create_string_buffer(buflen)
    _lib.check(getattr(_lib.load(), symbol)(*args, buf, buflen))
    return buf.value.decode()


def _array(ws_desc: Sequence[QllmWeight]):
    return (QllmWeight * len(ws_desc))(*ws_desc)


def linear_forward(w: QllmWeight, x2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = x2d[M,K] . dequant(w) (+bias) through the fused HIP kernels.  Raises QllmUnsupported when the
    library has no fused kernel for the configuration (caller may then use dequant() + matmul)."""
    _check_x(x2d, (w,))
    lib = _lib.load()
    return _forward((w,), x2d, out, lib.qllm_workspace_bytes_act,
                    lambda wr, y, x, m, dt, ws: lib.qllm_linear_forward(wr, x.data_ptr(), y, m, dt, ws.data_ptr(), ws.numel(), _stream_ptr()))


def linear_forward_permuted(w: QllmWeight, perm: torch.Tensor, x2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = x2d[:, perm] . dequant(w) (+bias) in ONE launch (qllm_linear_forward_permuted): `w` is a plain descriptor -- the
    row-sorted copy of an act-order layer -- and `perm` the int32 device permutation `gather_columns` takes.  Bit-identical to
    `linear_forward(w, gather_columns(x2d, perm))`, and faster than it at 1-2 rows only (profiles/bitgemv_actorder.md).  Raises QllmUnsupported for every call the bit-stream matvec does not serve
    (more than 16 rows, other layouts, QLLM_BITGEMV = 0): callers then gather and call linear_forward, or dequantise."""
    _check_x(x2d, (w,))
    _check_perm(perm, x2d)
    lib = _lib.load()
    return _forward((w,), x2d, out, lib.qllm_workspace_bytes_act,
                    lambda wr, y, x, m, dt, ws: lib.qllm_linear_forward_permuted(wr, perm.data_ptr(), x.data_ptr(), y, m, dt, ws.data_ptr(),
                                                                                 ws.numel(), _stream_ptr()))


def bitpanel_max_m() -> int:
    """The most rows module code sends to `linear_forward_bitpanel`: the QLLM_BITPANEL_MAX_M knob, else the library's default
    (include/qllm_mi355x.h, profiles/bitpanel.md); 0 -- the modules do not use the entry -- where that default is 0 or QLLM_BITPANEL is
    switched off.  The entry itself takes up to 512 rows whatever this says."""
    v = get_knob("QLLM_BITPANEL_MAX_M")
    m = _lib.BITPANEL_MAX_M_DEFAULT if v is None else v
    if m < 17 or get_knob("QLLM_BITPANEL") == 0:
        return 0
    return m


def linear_forward_bitpanel(w: QllmWeight, x2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = x2d[M,K] . dequant(w) (+bias) through the fused mid-batch kernel (qllm_linear_forward_bitpanel, csrc/bitpanel.hip):
    17..512 rows, GPTQ / HQQ layouts in place, 2..8 bits, no g_idx.  An entry of its own -- `linear_forward` and `plan_describe` keep
    refusing these calls.  Raises QllmUnsupported for everything it does not serve (callers then use dequant() + matmul)."""
    _check_x(x2d, (w,))
    lib = _lib.load()
    return _forward((w,), x2d, out, lambda wr, m, dt: lib.qllm_bitpanel_workspace_bytes(wr, m),
                    lambda wr, y, x, m, dt, ws: lib.qllm_linear_forward_bitpanel(wr, x.data_ptr(), y, m, dt, ws.data_ptr(), ws.numel(),
                                                                                 _stream_ptr()))


def bitpanel_describe(w: QllmWeight, m: int, have_workspace: bool = True) -> str:
    """The geometry `linear_forward_bitpanel` would launch for m rows ("bitpanel bits=.. cols=64 row_tiles=.. row_blocks=.. split_k=.."),
    or "unsupported (...)".  Pure host code."""
    return _describe("qllm_bitpanel_describe", 512, C.byref(w), int(m), 1 if have_workspace else 0)


def bitgemm_min_m() -> int:
    """The fewest rows module code sends to `linear_forward_bitgemm` (above `bitpanel_max_m()`): the QLLM_BITGEMM_MIN_M knob, else the
    library's default (include/qllm_mi355x.h, profiles/bitgemm.md); 0 -- the modules do not use the entry -- where that default is 0
    or QLLM_BITGEMM is switched off.  The entry itself takes 129 rows and up whatever this says."""
    v = get_knob("QLLM_BITGEMM_MIN_M")
    m = _lib.BITGEMM_MIN_M_DEFAULT if v is None else v
    if m < 129 or get_knob("QLLM_BITGEMM") == 0:
        return 0
    return m


def linear_forward_bitgemm(w: QllmWeight, x2d: torch.Tensor, out: Optional[torch.Tensor] = None,
                           key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = x2d[M,K] . dequant(w) (+bias) through the fused 2..8-bit prefill kernel (qllm_linear_forward_bitgemm, csrc/bitgemm.hip):
    129 rows and up, GPTQ / HQQ layouts in place, K % 64 == 0, N % 8 == 0, no g_idx.  An entry of its own -- `linear_forward` and
    `plan_describe` keep refusing these calls.  A bf16 x goes through the shared fp16 copy (`bf16_as_f16(x2d, key)`: siblings convert
    once) and gives a bf16 y, as `linear_forward_bf16_via_f16` does.  Raises QllmUnsupported for everything the entry does not serve
    (callers then use dequant() + matmul) -- decided BEFORE x is converted."""
    _check_x(x2d, (w,))
    lib = _lib.load()
    dt = DT_F16

    def fp16_x():
        nonlocal dt
        if x2d.shape[0] == 0:
            return x2d
        dt = _lib.DT_F16_IN_BF16_OUT if x2d.dtype == torch.bfloat16 else _act_dtype(x2d)
        if dt == DT_F16:
            return x2d
        why = bitgemm_describe(w, x2d.shape[0])   # (nothing is converted for a call the entry refuses)
        if why.startswith("unsupported"):
            raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, why)
        return bf16_as_f16(x2d, key)
    return _forward((w,), x2d, out, lambda wr, m, _: lib.qllm_bitgemm_workspace_bytes(wr, m),
                    lambda wr, y, x, m, _, ws: lib.qllm_linear_forward_bitgemm(wr, x.data_ptr(), y, m, dt, ws.data_ptr(), ws.numel(), _stream_ptr()),
                    prepare=fp16_x)


def bitgemm_describe(w: QllmWeight, m: int, have_workspace: bool = True) -> str:
    """The geometry `linear_forward_bitgemm` would launch for m rows ("bitgemm bits=.. tile=256x128 tiles=.. split_k=.."), or
    "unsupported (...)".  Pure host code."""
    return _describe("qllm_bitgemm_describe", 512, C.byref(w), int(m), 1 if have_workspace else 0)


_LAST_CONVERT: dict = {}


def bf16_as_f16(x2d: torch.Tensor, key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp16 copy of a contiguous bf16 activation matrix (round to nearest even, what `.to(float16)` does), made by the library's
    kernel and REMEMBERED per device for the tensor OBJECT it was made from: q/k/v -- and gate/up -- are called with the same
    tensor one after the other, so three prefill calls convert once.  `key` is that object (module code passes the `x` its forward
    received: `x.reshape(-1, K)` is a fresh object per call and would never hit); it is held weakly and its death drops the copy,
    so the cache never keeps a prefill-sized buffer beyond its input's life.  Inference tensors (no version counter: an in-place
    update could not be seen) are converted every time: the sharing works under `torch.no_grad()`, not under
    `torch.inference_mode()`.  A hit also requires the caller's current stream to be the one the copy was made on."""
    import weakref
    k = x2d if key is None else key
    cacheable = not k.is_inference() and k.device == x2d.device
    dev = x2d.device
    if cacheable:
        hit = _LAST_CONVERT.get(dev)
        # (the copy was produced on ONE stream: a caller on another stream has no ordering with it -- convert again there)
        if hit is not None and hit[0]() is k and hit[1] == k._version and hit[2].shape == x2d.shape and hit[3] == _stream_ptr():
            return hit[2]
    _check_input(x2d, "x")
    out = torch.empty(x2d.shape, dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().qllm_convert_bf16_to_f16(x2d.data_ptr(), out.data_ptr(), x2d.numel(), _stream_ptr()))
    if cacheable:
        def _drop(ref, dev=dev):
            cur = _LAST_CONVERT.get(dev)
            if cur is not None and cur[0] is ref:
                _LAST_CONVERT.pop(dev, None)
        _LAST_CONVERT[dev] = (weakref.ref(k, _drop), k._version, out, _stream_ptr())
    else:
        _LAST_CONVERT.pop(dev, None)
    return out


def linear_forward_bf16_via_f16(w: QllmWeight, x2d: torch.Tensor, key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Prefill-sized bf16 call with the conversion of x hoisted and shared (QLLM_F16_IN_BF16_OUT): bit-identical to
    `linear_forward(w, x2d)` on the 256x128 prefill kernel, which converts x into the workspace on every call.  Raises
    QllmUnsupported where that kernel does not serve the call (callers then use linear_forward) -- decided from the plan BEFORE x is
    converted, so that a call the panel kernel / gemm2 / the fallbacks take does not pay for a copy it cannot use."""
    _check_x(x2d, (w,))
    if x2d.dtype != torch.bfloat16 or x2d.shape[0] <= 64 or x2d.numel() % 8 != 0:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "bf16 prefill calls only")
    if w.bits != 4 or not plan_describe([w], x2d.shape[0]).startswith("gemm3"):
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "not a call of the 256x128 prefill kernel")
    # (the workspace is sized for fp16 activations: the copy the plain bf16 call would stage there is made here, and shared)
    lib = _lib.load()
    return _forward((w,), x2d, None, lambda wr, m, _: lib.qllm_workspace_bytes_act(wr, m, DT_F16),
                    lambda wr, y, xh, m, _, ws: lib.qllm_linear_forward(wr, xh.data_ptr(), y, m, _lib.DT_F16_IN_BF16_OUT, ws.data_ptr(), ws.numel(),
                                                                        _stream_ptr()), prepare=lambda: bf16_as_f16(x2d, key))


def _bf16_native(w: QllmWeight) -> bool:
    """Round 6: the 256x128 prefill kernel takes bf16 activations as they are on the 4-bit row-stream / strip-major layouts (bf16 W,
    bf16 MFMA: csrc/gemm3.hip, BF) -- nothing to convert, nothing to share.  `set_knob("QLLM_GEMM3_BF16", 0)` brings the fp16
    conversion pre-pass (the reference's shim, quant_linear_awq.py:29-36) back."""
    return (w.bits == 4 and w.layout in (LAYOUTS["GPTQ"], LAYOUTS["HQQ"], LAYOUTS["NATIVE"], LAYOUTS["NATIVE_F16Z"])
            and get_knob("QLLM_GEMM3_BF16") != 0)


def linear_forward_shared(w: QllmWeight, x2d: torch.Tensor, key: Optional[torch.Tensor] = None) -> torch.Tensor:
    """linear_forward for module code: bf16 prefill calls go through the shared fp16 copy of x where the kernel allows it.  `key`:
    the tensor object whose identity marks "the same input" across sibling calls (default: x2d itself)."""
    if x2d.dtype == torch.bfloat16 and x2d.shape[0] > 64 and not _bf16_native(w):
        try:
            return linear_forward_bf16_via_f16(w, x2d, key)
        except QllmUnsupported:
            pass
    return linear_forward(w, x2d)


def grouped_workspace_bytes(ws_desc: Sequence[QllmWeight], m: int, act_dtype: int, device: torch.device) -> int:
    """The grouped call's workspace rule (include/qllm_mi355x.h): the sum of the layers' qllm_workspace_bytes_act, and from 384 rows at
    least 16 KB + 128 KB per CU -- a prefill group K-splits the ragged last round of ALL its layers' tiles, which no layer's size bounds."""
    lib = _lib.load()
    nbytes = sum(lib.qllm_workspace_bytes_act(C.byref(w), m, act_dtype) for w in ws_desc)
    if m >= 384:
        nbytes = max(nbytes, 16384 + torch.cuda.get_device_properties(device).multi_processor_count * 256 * 128 * 4)
    return nbytes


def linear_forward_grouped(ws_desc: Sequence[QllmWeight], x2d: torch.Tensor,
                           outs: Optional[Sequence[torch.Tensor]] = None):
    """Several layers sharing x (q/k/v, gate/up) in ONE launch (decode sizes only)."""
    _check_x(x2d, ws_desc)
    lib, n = _lib.load(), len(ws_desc)
    return list(_forward(ws_desc, x2d, outs, lambda arr, m, dt: grouped_workspace_bytes(ws_desc, m, dt, x2d.device),
                         lambda arr, ys, x, m, dt, ws: lib.qllm_linear_forward_grouped(arr, ys, n, x.data_ptr(), m, dt, ws.data_ptr(), ws.numel(),
                                                                                       _stream_ptr()), many=True))


def bitgroup_max_m() -> int:
    """The most rows the sibling groups send to `linear_forward_bitgroup`: the QLLM_BITGROUP_MAX_M knob, else the library's default
    (include/qllm_mi355x.h, profiles/bitgemv_group.md); 0: never.  The entry itself takes up to 16 rows whatever this says."""
    v = get_knob("QLLM_BITGROUP_MAX_M")
    return _lib.BITGROUP_MAX_M_DEFAULT if v is None else v


def linear_forward_bitgroup(ws_desc: Sequence[QllmWeight], x2d: torch.Tensor,
                            outs: Optional[Sequence[torch.Tensor]] = None):
    """1..4 layers of 2..8 bits sharing x (q/k/v, gate/up) in ONE launch of the bit-stream matvec at 1..16 rows
    (qllm_linear_forward_bitgroup, csrc/bitgemv_group.hip).  Every output is bit-identical to `linear_forward` on that layer alone.
    An entry of its own -- `linear_forward_grouped` and `plan_describe` keep refusing these widths.  Raises QllmUnsupported for
    everything it does not serve (callers then run the layers one by one)."""
    _check_x(x2d, ws_desc)
    lib, n = _lib.load(), len(ws_desc)
    return list(_forward(ws_desc, x2d, outs, lambda arr, m, dt: lib.qllm_bitgroup_workspace_bytes(arr, n, m),
                         lambda arr, ys, x, m, dt, ws: lib.qllm_linear_forward_bitgroup(arr, ys, n, x.data_ptr(), m, dt, ws.data_ptr(), ws.numel(),
                                                                                        _stream_ptr()), many=True))


def bitgroup_describe(ws_desc: Sequence[QllmWeight], m: int, have_workspace: bool = True) -> str:
    """The geometry `linear_forward_bitgroup` would launch for m rows ("bitgroup bits=.. cols=32 layers=.. blocks=.. split_k=a,b,c", the
    splits in the order of `ws_desc`), or "unsupported (...)".  Pure host code."""
    return _describe("qllm_bitgroup_describe", 512, _array(ws_desc), len(ws_desc), int(m), 1 if have_workspace else 0)


def linear_forward_swiglu(w: QllmWeight, gate2d: torch.Tensor, up2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[M,N] = (silu(gate2d) * up2d)[M,K] . dequant(w) (+bias) in ONE launch (qllm_linear_forward_swiglu, csrc/strip1_swiglu.hip): the
    down-projection of a SwiGLU MLP with the elementwise product formed while the batch-1 kernel stages its input.  Bit-identical to
    `linear_forward(w, F.silu(gate2d) * up2d)` wherever torch's silu rounds like the kernel's.  Raises QllmUnsupported for every call
    the batch-1 kernel does not serve (callers then run the activation and `linear_forward`)."""
    _check_x(gate2d, (w,))
    _check_input(up2d, "up")
    if up2d.shape != gate2d.shape or up2d.dtype != gate2d.dtype or up2d.device != gate2d.device:
        raise RuntimeError(f"up must match gate: {tuple(gate2d.shape)} {gate2d.dtype} on {gate2d.device}, got {tuple(up2d.shape)} {up2d.dtype} on {up2d.device}")
    lib = _lib.load()
    return _forward((w,), gate2d, out, None,
                    lambda wr, y, gate, m, dt, ws: lib.qllm_linear_forward_swiglu(wr, gate.data_ptr(), up2d.data_ptr(), y, m, dt, _lib.ACT_SILU,
                                                                                  _stream_ptr()))


def swiglu_describe(w: QllmWeight, m: int) -> str:
    """What `linear_forward_swiglu` would launch for m rows: "swiglu " + the plan line of the plain call ("swiglu strip1 nw=.. round=..
    ..."), or "refused: ..." with the entry's refusal text.  Pure host code."""
    return _describe("qllm_swiglu_describe", 640, C.byref(w), int(m))


def _check_residual(residual2d: torch.Tensor, w: QllmWeight, x2d: torch.Tensor):
    _check_input(residual2d, "residual")
    if tuple(residual2d.shape) != (x2d.shape[0], w.N) or residual2d.dtype != x2d.dtype or residual2d.device != x2d.device:
        raise RuntimeError(f"residual must be a [{x2d.shape[0]}, {w.N}] {x2d.dtype} tensor on {x2d.device}, got {tuple(residual2d.shape)} "
                           f"{residual2d.dtype} on {residual2d.device}")


def linear_forward_residual(w: QllmWeight, x2d: torch.Tensor, residual2d: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[1,N] = residual2d + x2d[1,K] . dequant(w) (+bias) in ONE launch (qllm_linear_forward_residual, csrc/strip1_resid.hip): the o_proj
    of a decoder layer with the residual add formed by the threads that store the output.  Bit-identical to
    `residual2d + linear_forward(w, x2d)`.  `out` may be residual2d itself.  One row; raises QllmUnsupported for every call the batch-1
    kernel does not serve (callers then run `linear_forward` and add)."""
    _check_x(x2d, (w,))
    _check_residual(residual2d, w, x2d)
    lib = _lib.load()
    return _forward((w,), x2d, out, None,
                    lambda wr, y, x, m, dt, ws: lib.qllm_linear_forward_residual(wr, x.data_ptr(), None, residual2d.data_ptr(), y, m, dt, _lib.ACT_SILU,
                                                                                 _stream_ptr()))


def linear_forward_swiglu_residual(w: QllmWeight, gate2d: torch.Tensor, up2d: torch.Tensor, residual2d: torch.Tensor,
                                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y[1,N] = residual2d + (silu(gate2d) * up2d)[1,K] . dequant(w) (+bias) in ONE launch (qllm_linear_forward_residual with `up`,
    csrc/strip1_swiglu_resid.hip): the down_proj of a SwiGLU MLP with neither elementwise kernel around it.  Bit-identical to
    `residual2d + linear_forward_swiglu(w, gate2d, up2d)`.  `out` may be residual2d itself.  One row; raises QllmUnsupported for every
    call the batch-1 kernel does not serve."""
    _check_x(gate2d, (w,))
    _check_input(up2d, "up")
    if up2d.shape != gate2d.shape or up2d.dtype != gate2d.dtype or up2d.device != gate2d.device:
        raise RuntimeError(f"up must match gate: {tuple(gate2d.shape)} {gate2d.dtype} on {gate2d.device}, got {tuple(up2d.shape)} {up2d.dtype} on {up2d.device}")
    _check_residual(residual2d, w, gate2d)
    lib = _lib.load()
    return _forward((w,), gate2d, out, None,
                    lambda wr, y, gate, m, dt, ws: lib.qllm_linear_forward_residual(wr, gate.data_ptr(), up2d.data_ptr(), residual2d.data_ptr(), y, m, dt,
                                                                                    _lib.ACT_SILU, _stream_ptr()))


def residual_describe(w: QllmWeight, m: int, swiglu: bool = False) -> str:
    """What `linear_forward_residual` (swiglu: `linear_forward_swiglu_residual`) would launch for m rows: "residual " / "residual swiglu "
    + the plan line of the plain call, or "refused: ..." with the entry's refusal text.  Pure host code."""
    return _describe("qllm_residual_describe", 640, C.byref(w), int(m), 1 if swiglu else 0)


def _rstd_buffer(return_rstd, m: int, x2d: torch.Tensor):
    """return_rstd of the two RMSNorm wrappers: False (None), True (a new fp32 [m] tensor) or the caller's contiguous fp32 [m] tensor."""
    if return_rstd is False or return_rstd is None:
        return None
    if return_rstd is True:
        return torch.empty((m,), dtype=torch.float32, device=x2d.device)
    r = return_rstd
    if r.dtype != torch.float32 or tuple(r.shape) != (m,) or r.device != x2d.device or not r.is_contiguous():
        raise RuntimeError(f"return_rstd must be True or a contiguous float32 [{m}] tensor on {x2d.device}")
    return r


def _check_norm_weight(weight: torch.Tensor, x2d: torch.Tensor):
    _check_input(weight, "weight")
    if weight.dim() != 1 or weight.shape[0] != x2d.shape[1] or weight.dtype != x2d.dtype or weight.device != x2d.device:
        raise RuntimeError(f"weight must be a [{x2d.shape[1]}] {x2d.dtype} tensor on {x2d.device}, got {tuple(weight.shape)} {weight.dtype} on {weight.device}")


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float, out: Optional[torch.Tensor] = None, return_rstd: bool = False):
    """weight * (x.float() * rsqrt(mean(x^2) + eps)).to(dtype) over the last dimension in ONE kernel (qllm_rmsnorm, csrc/rmsnorm.hip): the
    eager LlamaRMSNorm's arithmetic, rounding for rounding.  x: contiguous fp16 / bf16 [..., K] on the device, K % 8 == 0, K <= 65536;
    weight: [K] of x's type; `out` may be x itself.  return_rstd: also the rows' rstd, fp32 [rows] (True, or the caller's tensor to write them into)."""
    _check_input(x, "x")
    if x.dim() < 1:
        raise RuntimeError("x must have at least one dimension")
    x2d = x.view(-1, x.shape[-1])
    _check_norm_weight(weight, x2d)
    m, k = x2d.shape
    if out is None:
        out = torch.empty_like(x)
    elif out.shape != x.shape or out.dtype != x.dtype or out.device != x.device or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous {tuple(x.shape)} {x.dtype} tensor on {x.device}, got {tuple(out.shape)} {out.dtype} on {out.device}")
    rstd = _rstd_buffer(return_rstd, m, x2d)
    if m > 0:
        with torch.cuda.device(x.device):
            rc = _lib.load().qllm_rmsnorm(x2d.data_ptr(), weight.data_ptr(), out.data_ptr(), m, k, float(eps), _act_dtype(x2d),
                                          rstd.data_ptr() if rstd is not None else None, _stream_ptr())
        _lib.check(rc)
    return (out, rstd) if rstd is not None else out


def linear_forward_rmsnorm(ws_desc: Sequence[QllmWeight], x2d: torch.Tensor, weight: torch.Tensor, eps: float,
                           outs: Optional[Sequence[torch.Tensor]] = None, return_rstd: bool = False):
    """[linear(w, RMSNorm(x2d)) for w in ws_desc] in ONE launch (qllm_linear_forward_rmsnorm, csrc/strip1_norm.hip): the grouped launch of
    the layers behind a norm (q/k/v, gate/up) with the norm formed while the batch-1 kernel stages its input.  Bit-identical to
    `linear_forward_grouped(ws_desc, weight * (x2d.float() * rstd).to(x2d.dtype))` with the rstd it reports (return_rstd: fp32 [M]
    behind the outputs).  One row; raises QllmUnsupported for every call the batch-1 kernel does not serve (callers then run `rmsnorm`
    and `linear_forward_grouped`)."""
    _check_x(x2d, ws_desc)
    _check_norm_weight(weight, x2d)
    lib, n, rstd = _lib.load(), len(ws_desc), None

    def rstd_buffer():   # (also at zero rows, where the outputs and rstd come back empty)
        nonlocal rstd
        rstd = _rstd_buffer(return_rstd, x2d.shape[0], x2d)
        return x2d
    outs = list(_forward(ws_desc, x2d, outs, None,
                         lambda arr, ys, x, m, dt, ws: lib.qllm_linear_forward_rmsnorm(arr, ys, n, x.data_ptr(), weight.data_ptr(), float(eps), m, dt,
                                                                                       _ptr(rstd), _stream_ptr()), many=True, prepare=rstd_buffer))
    return (outs, rstd) if rstd is not None else outs


def rmsnorm_describe(ws_desc: Sequence[QllmWeight], m: int) -> str:
    """What `linear_forward_rmsnorm` would launch for m rows: "rmsnorm " + the plan line of the plain grouped call ("rmsnorm strip1 nw=..
    round=.. ..."), or "refused: ..." with the entry's refusal text.  Pure host code."""
    return _describe("qllm_rmsnorm_describe", 768, _array(ws_desc), len(ws_desc), int(m))


ROPE_MAX_HEAD_DIM = 256   # kRopeMaxHeadDim of csrc/kernels.hpp


def _rope_tokens(t: torch.Tensor, unsqueeze_dim: int) -> torch.Tensor:
    """The [B, S, H, D] view of a 4-D q / k: `unsqueeze_dim` 1 says [B, H, S, D], 2 says [B, S, H, D]."""
    return t.transpose(1, 2) if unsqueeze_dim == 1 else t


def _rope_strides(t: torch.Tensor, unsqueeze_dim: int, name: str):
    """(row stride, head stride) in elements of q / k as qllm_rope reads it -- token (b, s) is row b * S + s -- or QllmUnsupported."""
    b, s, h, d = _rope_tokens(t, unsqueeze_dim).shape
    sb, ss, sh, sd = _rope_tokens(t, unsqueeze_dim).stride()
    if sd != 1:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"rope: the last dimension of {name} must have stride 1 (got {sd})")
    if s > 1 and b > 1 and sb != s * ss:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"rope: the tokens of {name} must be rows of one stride (batch stride {sb}, sequence stride {ss} x {s})")
    row = ss if s > 1 else sb if b > 1 else h * d
    head = sh if h > 1 else d
    if row % 8 or head % 8 or row < 0 or head < 0 or t.data_ptr() % 16:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"rope: {name} must be 16-byte aligned with strides that are multiples of 8 (row {row}, head {head})")
    # the eager output keeps its input's dimension order (as torch.empty_like does); the kernel writes [tokens, heads, head_dim]
    order = [st for n, st in zip((b, s, h, d), (sb, ss, sh, sd)) if n > 1]
    if any(x <= y for x, y in zip(order, order[1:])):
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"rope: {name} is not token-major in memory (strides {tuple(t.stride())}): the eager result would not be either")
    return row, head


def rope_plan(q: torch.Tensor, k: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, unsqueeze_dim: int = 1):
    """What `rope` hands to qllm_rope for these tensors -- (rows, q_heads, k_heads, head_dim, q row / head stride, k row / head stride,
    cos_rows) -- or QllmUnsupported with the reason: q / k 4-D of one fp16 / bf16 type with cos / sin, [B, H, S, D] (unsqueeze_dim 1) or
    [B, S, H, D] (2), inner stride 1, tokens at one row stride, 16-byte aligned, strides multiples of 8; D % 16 == 0, 16 <= D <= 256;
    cos / sin contiguous [B or 1, S, D] (the whole head: no partial rotary); and the eager call's output, which keeps its input's
    dimension order, token-major -- a head-major [B, H, S, D] input with H, S > 1 is not served.  Pure host code, any device."""
    def no(why):
        return QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "rope: " + why)
    if unsqueeze_dim not in (1, 2):
        raise no(f"unsqueeze_dim must be 1 ([B, H, S, D]) or 2 ([B, S, H, D]), got {unsqueeze_dim}")
    ts = [("q", q), ("cos", cos), ("sin", sin)] + ([("k", k)] if k is not None else [])
    if q.dtype not in (torch.float16, torch.bfloat16) or any(t.dtype != q.dtype for _, t in ts):
        raise no("q, k, cos and sin must share one type, float16 or bfloat16 (got " + ", ".join(str(t.dtype)[6:] for _, t in ts) + ")")
    if any(t.device != q.device for _, t in ts):
        raise no("q, k, cos and sin must be on one device")
    if q.dim() != 4 or (k is not None and (k.dim() != 4 or _rope_tokens(k, unsqueeze_dim).shape[:2] != _rope_tokens(q, unsqueeze_dim).shape[:2] or k.shape[3] != q.shape[3])):
        raise no("q and k must be 4-D with the same batch, sequence and head sizes")
    b, s, hq, d = _rope_tokens(q, unsqueeze_dim).shape
    hk = _rope_tokens(k, unsqueeze_dim).shape[2] if k is not None else 0
    if d % 16 or d < 16 or d > ROPE_MAX_HEAD_DIM:
        raise no(f"head_dim % 16 == 0, 16 <= head_dim <= {ROPE_MAX_HEAD_DIM} (got {d})")
    if b * s == 0 or hq == 0 or (k is not None and hk == 0):
        raise no("empty q / k")
    if cos.shape != sin.shape or cos.dim() != 3 or cos.shape[0] not in (1, b) or tuple(cos.shape[1:]) != (s, d):
        raise no(f"cos and sin must be [{b} or 1, {s}, {d}] (got {tuple(cos.shape)}, {tuple(sin.shape)})")
    if not cos.is_contiguous() or not sin.is_contiguous() or cos.data_ptr() % 16 or sin.data_ptr() % 16:
        raise no("cos and sin must be contiguous and 16-byte aligned")
    strides = _rope_strides(q, unsqueeze_dim, "q") + (_rope_strides(k, unsqueeze_dim, "k") if k is not None else (0, 0))
    return (b * s, hq, hk, d) + strides + (cos.shape[0] * s,)


def _rope_outputs(op: str, q, k, cos, sin, unsqueeze_dim: int, out):
    """(q_out, k_out) of `rope` / `rope_qknorm` for inputs their plan serves: new tensors as the eager call would return them, or the
    caller's `out`, checked.  Device tensors only."""
    for t in (q, cos, sin) + ((k,) if k is not None else ()):
        if not t.is_cuda:
            raise RuntimeError(f"{op}: q, k, cos and sin must be HIP/CUDA tensors (qllm_amd has no CPU forward path)")
    if out is None:
        q_out, k_out = torch.empty_like(q), torch.empty_like(k) if k is not None else None
        if not all(o is None or _rope_tokens(o, unsqueeze_dim).is_contiguous() for o in (q_out, k_out)):
            raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"{op}: the eager result of these inputs is not token-major in memory")
        return q_out, k_out
    q_out, k_out = out
    for name, o, t in (("q_out", q_out, q), ("k_out", k_out, k)):
        if (o is None) != (t is None):
            raise RuntimeError(f"{op}: {name} must be given exactly when its input is")
        if t is not None and (o.shape != t.shape or o.dtype != t.dtype or o.device != t.device or not _rope_tokens(o, unsqueeze_dim).is_contiguous()):
            raise RuntimeError(f"{op}: {name} must be a {tuple(t.shape)} {t.dtype} tensor on {t.device} that is dense and token-major in memory")
    return q_out, k_out


def rope(q: torch.Tensor, k: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, unsqueeze_dim: int = 1, *, out=None, plan=None):
    """(q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin) with cos / sin unsqueezed at `unsqueeze_dim`: transformers'
    apply_rotary_pos_emb (Llama, Mistral, Qwen2) for both tensors in ONE kernel (qllm_rope, csrc/rope.hip), bit for bit, returning tensors
    of the shape and strides the eager call returns -- for the usual view(B, S, H, D).transpose(1, 2) inputs logical [B, H, S, D] over
    [B, S, H, D] memory.  `rope_plan` says what is served; everything else raises QllmUnsupported before anything is launched.  k may be
    None (q alone: returns (q_out, None)).  out: (q_out, k_out) to write into, each of its input's shape, type and device, laid out as
    the result would be (token-major, dense); an output may be its input when that one is laid out so.  plan: what `rope_plan` returned
    for these very arguments, for a caller that has asked already."""
    rows, hq, hk, d, q_row, q_head, k_row, k_head, cos_rows = plan if plan is not None else rope_plan(q, k, cos, sin, unsqueeze_dim)
    q_out, k_out = _rope_outputs("rope", q, k, cos, sin, unsqueeze_dim, out)
    with torch.cuda.device(q.device):
        rc = _lib.load().qllm_rope(q.data_ptr(), _ptr(k), cos.data_ptr(), sin.data_ptr(), q_out.data_ptr(), _ptr(k_out), rows, hq, hk, d,
                                   q_row, q_head, k_row, k_head, cos_rows, _act_dtype(q), _stream_ptr())
    _lib.check(rc)
    return q_out, k_out


ROPE_QKNORM_HEAD_DIMS = (64, 128)   # what csrc/rope_qknorm.hip is built for (rope_qknorm_head_dim of csrc/kernels.hpp)


def rope_qknorm_plan(q: torch.Tensor, k: Optional[torch.Tensor], q_weight: torch.Tensor, k_weight: Optional[torch.Tensor], eps: float, cos: torch.Tensor,
                     sin: torch.Tensor, unsqueeze_dim: int = 1):
    """What `rope_qknorm` hands to qllm_rope_qknorm for these tensors -- `rope_plan`'s answer, by `rope_plan`'s rules -- or QllmUnsupported
    with the reason; on top of those rules: head_dim 64 or 128, each weight a contiguous, 16-byte aligned [head_dim] tensor of q's type on
    q's device (k_weight exactly when k is given), eps finite and > 0.  Pure host code, any device."""
    plan = rope_plan(q, k, cos, sin, unsqueeze_dim)
    d = plan[3]

    def no(why):
        return QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "rope_qknorm: " + why)
    if d not in ROPE_QKNORM_HEAD_DIMS:
        raise no(f"head_dim must be 64 or 128 (got {d})")
    if (k is None) != (k_weight is None):
        raise no("k_weight must be given exactly when k is")
    for name, w in (("q_weight", q_weight),) + ((("k_weight", k_weight),) if k is not None else ()):
        if not isinstance(w, torch.Tensor) or w.dim() != 1 or w.shape[0] != d:
            raise no(f"{name} must be a [{d}] tensor (got {tuple(w.shape) if isinstance(w, torch.Tensor) else type(w).__name__})")
        if w.dtype != q.dtype or w.device != q.device:
            raise no(f"{name} must be of q's type and device, {q.dtype} on {q.device} (got {w.dtype} on {w.device})")
        if not w.is_contiguous() or w.data_ptr() % 16:
            raise no(f"{name} must be contiguous and 16-byte aligned")
    if not (eps > 0 and math.isfinite(eps)):
        raise no(f"eps must be finite and > 0 (got {eps})")
    return plan


def rope_qknorm(q: torch.Tensor, k: Optional[torch.Tensor], q_weight: torch.Tensor, k_weight: Optional[torch.Tensor], eps: float, cos: torch.Tensor,
                sin: torch.Tensor, unsqueeze_dim: int = 1, *, out=None, plan=None):
    """`rope(norm(q, q_weight), norm(k, k_weight), cos, sin, unsqueeze_dim)` with norm the RMSNorm over head_dim of every (token, head) --
    what Qwen3's attention computes between its q / k projections and the attention core (q_norm, k_norm, apply_rotary_pos_emb) -- in
    ONE kernel (qllm_rope_qknorm, csrc/rope_qknorm.hip).  Bit for bit `rope(rmsnorm(q_c, q_weight, eps), rmsnorm(k_c, k_weight, eps), ...)`
    on contiguous [B, S, H, D] copies, with every rounding of the eager modules.  Shapes, strides, `out` and `plan` are `rope`'s:
    `rope_qknorm_plan` says what is served, everything else raises QllmUnsupported before anything is launched."""
    rows, hq, hk, d, q_row, q_head, k_row, k_head, cos_rows = plan if plan is not None else rope_qknorm_plan(q, k, q_weight, k_weight, eps, cos, sin,
                                                                                                             unsqueeze_dim)
    q_out, k_out = _rope_outputs("rope_qknorm", q, k, cos, sin, unsqueeze_dim, out)
    with torch.cuda.device(q.device):
        rc = _lib.load().qllm_rope_qknorm(q.data_ptr(), _ptr(k), cos.data_ptr(), sin.data_ptr(), q_out.data_ptr(), _ptr(k_out), q_weight.data_ptr(),
                                          _ptr(k_weight), float(eps), rows, hq, hk, d, q_row, q_head, k_row, k_head, cos_rows, _act_dtype(q), _stream_ptr())
    _lib.check(rc)
    return q_out, k_out


MOE_MAX_TOKENS, MOE_MAX_TOP_K, MOE_MAX_H = 4, 8, 16384   # kMoeMaxTokens, kMoeMaxTopK, kMoeMaxH of csrc/kernels.hpp


def _moe_no(why):
    return QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "moe_decode: " + why)


def _moe_stack(name: str, stack, device):
    """(E, K, N) of one stack of expert layers -- (qweight int32 [E, N/16, K/8, 16], scales float16 [E, N/16, K/128, 16], qzeros int32
    [E, N/16, K/128, 2] or None): the native strip-major layout of 4-bit, 128-wide-group layers, expert after expert -- or QllmUnsupported."""
    if not isinstance(stack, (tuple, list)) or len(stack) != 3 or not all(isinstance(t, torch.Tensor) for t in stack[:2]):
        raise _moe_no(f"{name} must be (qweight, scales, qzeros or None) tensors")
    qw, sc, qz = stack
    if qw.dim() != 4 or qw.shape[3] != 16 or qw.dtype != torch.int32:
        raise _moe_no(f"{name} qweight must be int32 [E, N/16, K/8, 16] (got {qw.dtype} {tuple(qw.shape)})")
    e, ns, k8 = qw.shape[:3]
    if k8 % 16 or e == 0 or ns == 0 or k8 == 0:
        raise _moe_no(f"{name}: K must be a positive multiple of 128 (4 bits, 128-wide groups; got K={8 * k8})")
    if sc.dtype != torch.float16 or tuple(sc.shape) != (e, ns, k8 // 16, 16):
        raise _moe_no(f"{name} scales must be float16 {(e, ns, k8 // 16, 16)} (got {sc.dtype} {tuple(sc.shape)})")
    if qz is not None and (not isinstance(qz, torch.Tensor) or qz.dtype != torch.int32 or tuple(qz.shape) != (e, ns, k8 // 16, 2)):
        raise _moe_no(f"{name} qzeros must be None or int32 {(e, ns, k8 // 16, 2)}")
    for t in (qw, sc) + ((qz,) if qz is not None else ()):
        if t.device != device or not t.is_contiguous() or t.data_ptr() % 16:
            raise _moe_no(f"{name}: the stack must be contiguous, 16-byte aligned and on {device}")
    return e, 8 * k8, 16 * ns


def _moe_routing(ids, weights, t: int, act_dtype, device):
    """top_k of ids [T, top_k] (int64, as torch.topk leaves them) and, when given, weights [T, top_k] (float32 or the activation type)."""
    if not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.shape[0] != t or ids.dtype != torch.int64 or not ids.is_contiguous() or ids.device != device:
        raise _moe_no(f"ids must be a contiguous int64 [{t}, top_k] tensor on {device}")
    top_k = ids.shape[1]
    if not 1 <= top_k <= MOE_MAX_TOP_K:
        raise _moe_no(f"top_k 1..{MOE_MAX_TOP_K} (got {top_k})")
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.shape != ids.shape or weights.dtype not in (torch.float32, act_dtype)
                                or not weights.is_contiguous() or weights.device != device):
        raise _moe_no(f"weights must be a contiguous float32 or {act_dtype} {tuple(ids.shape)} tensor on {device}")
    return top_k


def _moe_act(name: str, x, rows, cols):
    if (not isinstance(x, torch.Tensor) or x.dim() != 2 or x.dtype not in (torch.float16, torch.bfloat16) or not x.is_contiguous() or x.data_ptr() % 16
            or (rows is not None and x.shape[0] != rows) or (cols is not None and x.shape[1] != cols)):
        raise _moe_no(f"{name} must be a contiguous, 16-byte aligned float16 / bfloat16 [{rows if rows is not None else 'T'}, {cols if cols is not None else 'H'}] tensor")
    return x.shape


def _moe_sizes(t: int, h: int, i: int):
    if not 1 <= t <= MOE_MAX_TOKENS:
        raise _moe_no(f"1..{MOE_MAX_TOKENS} tokens (got {t}): more rows are the modules' loop")
    if h % 128 or i % 128 or h > MOE_MAX_H:
        raise _moe_no(f"H % 128 == 0, I % 128 == 0 and H <= {MOE_MAX_H} (got H={h} I={i})")


def moe_plan(x: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, gate, up, down):
    """What `moe_gate_up` and `moe_down` are launched with for these tensors -- (T, top_k, E, H, I) -- or QllmUnsupported with the reason:
    the ONE place that says whether a routed-experts call is served.  x [T, H] float16 / bfloat16, contiguous, T = 1..4; ids int64
    [T, top_k], top_k = 1..8; weights [T, top_k] float32 or x's type; gate / up / down: stacks of E experts (`_moe_stack`) of shapes
    [H -> I], [H -> I], [I -> H] with H % 128 == 0, I % 128 == 0, H <= 16384, packed zero points in all three or in none; everything on
    one device; and, measured, one token or 2 * T * top_k <= E (below that many experts the tokens share them, and the loop, which
    reads a shared expert once, wins).  The two launchers themselves take every T <= 4.  Pure host code, any device."""
    t, h = _moe_act("x", x, None, None)
    top_k = _moe_routing(ids, weights, t, x.dtype, x.device)
    if weights is None:
        raise _moe_no("weights must be given")
    (e, kg, ng), (eu, ku, nu), (ed, kd, nd) = (_moe_stack(n, s, x.device) for n, s in (("gate", gate), ("up", up), ("down", down)))
    if (eu, ku, nu) != (e, kg, ng) or (ed, kd, nd) != (e, ng, kg) or kg != h:
        raise _moe_no(f"gate and up must be [{h} -> I] and down [I -> {h}] stacks of one expert count (got {(e, kg, ng)}, {(eu, ku, nu)}, {(ed, kd, nd)})")
    if len({s[2] is None for s in (gate, up, down)}) != 1:
        raise _moe_no("the three stacks must all have packed zero points or all be symmetric")
    _moe_sizes(t, h, ng)
    if t > 1 and 2 * t * top_k > e:
        # measured (profiles/moe_decode.md): the launches read one expert per SLOT, the loop each hit expert once for all its tokens; at
        # Mixtral's E = 8, top_k = 2 the pair wins at 2 tokens (x1.30), ties at 3 and loses at 4 (x0.85); at Qwen3-30B-A3B's E = 128 it wins 14-16-fold
        raise _moe_no(f"with {t} tokens x top_k {top_k} slots over {e} experts the loop reads each hit expert once and is faster (served: T == 1 or 2 * T * top_k <= E)")
    return t, top_k, e, h, ng


def moe_describe(t: int, top_k: int, e: int, h: int, i: int) -> str:
    """The launch shapes of the pair ("moe_decode gate_up grid=896x2 waves=8 ... | down grid=256x1 waves=16 ..."), or "refused: ...".
    Pure host code."""
    return _describe("qllm_moe_describe", 256, int(t), int(top_k), int(e), int(h), int(i))


def _moe_out(name: str, out, shape, like: torch.Tensor):
    if out is None:
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if tuple(out.shape) != tuple(shape) or out.dtype != like.dtype or out.device != like.device or not out.is_contiguous() or out.data_ptr() % 16:
        raise RuntimeError(f"{name} must be a contiguous, 16-byte aligned {tuple(shape)} {like.dtype} tensor on {like.device}")
    return out


def moe_gate_up(x: torch.Tensor, ids: torch.Tensor, gate, up, *, add_zero_bias: int = 0, out=None) -> torch.Tensor:
    """h[t * top_k + j] = act_fn(x[t] . Wgate[e]) * (x[t] . Wup[e]) with e = ids[t, j], SiLU and the eager roundings, for every slot in ONE
    launch (qllm_moe_gate_up, csrc/moe_decode.hip): [T * top_k, I].  The expert ids are read on the device; the row of a slot whose id is
    outside [0, E) is left unwritten.  `moe_plan` says what is served; everything else raises QllmUnsupported before anything is launched."""
    t, h = _moe_act("x", x, None, None)
    top_k = _moe_routing(ids, None, t, x.dtype, x.device)
    (e, kg, ng), (eu, ku, nu) = _moe_stack("gate", gate, x.device), _moe_stack("up", up, x.device)
    if (eu, ku, nu) != (e, kg, ng) or kg != h or (gate[2] is None) != (up[2] is None):
        raise _moe_no(f"gate and up must be [{h} -> I] stacks of one expert count and one kind of zero point")
    _moe_sizes(t, h, ng)
    if not x.is_cuda:
        raise RuntimeError("moe_gate_up: x must be a HIP/CUDA tensor (qllm_amd has no CPU forward path)")
    out = _moe_out("out", out, (t * top_k, ng), x)
    with torch.cuda.device(x.device):
        rc = _lib.load().qllm_moe_gate_up(x.data_ptr(), ids.data_ptr(), gate[0].data_ptr(), gate[1].data_ptr(), _ptr(gate[2]), up[0].data_ptr(),
                                          up[1].data_ptr(), _ptr(up[2]), out.data_ptr(), t, top_k, e, h, ng, int(add_zero_bias), _act_dtype(x), _stream_ptr())
    _lib.check(rc)
    return out


def moe_down(h: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, down, *, add_zero_bias: int = 0, out=None) -> torch.Tensor:
    """y[t] = sum_j ((h[t * top_k + j] . Wdown[e]) * weights[t, j]) with e = ids[t, j]: the down projections of every slot and the routed
    sum in ONE launch (qllm_moe_down, csrc/moe_decode.hip): [T, H].  Each projection is rounded to the activation type, its product with
    the weight again, and the products are added in ascending expert id with one rounding per add -- transformers' index_add_ loop,
    rounding for rounding; the same bits on every call.  Slots whose id is outside [0, E) add nothing.  `moe_plan` says what is served."""
    e, i, hh = _moe_stack("down", down, h.device)
    top_k = _moe_routing(ids, weights, ids.shape[0] if isinstance(ids, torch.Tensor) and ids.dim() == 2 else 0, h.dtype, h.device)
    if weights is None:
        raise _moe_no("weights must be given")
    t = ids.shape[0]
    _moe_act("h", h, t * top_k, i)
    _moe_sizes(t, hh, i)
    if not h.is_cuda:
        raise RuntimeError("moe_down: h must be a HIP/CUDA tensor (qllm_amd has no CPU forward path)")
    out = _moe_out("out", out, (t, hh), h)
    wdt = _lib.DT_F32 if weights.dtype == torch.float32 else _act_dtype(h)
    with torch.cuda.device(h.device):
        rc = _lib.load().qllm_moe_down(h.data_ptr(), ids.data_ptr(), weights.data_ptr(), down[0].data_ptr(), down[1].data_ptr(), _ptr(down[2]),
                                       out.data_ptr(), t, top_k, e, hh, i, int(add_zero_bias), wdt, _act_dtype(h), _stream_ptr())
    _lib.check(rc)
    return out


MOE_PREFILL_MAX_SLOTS, MOE_PREFILL_MAX_EXPERTS, MOE_PREFILL_TILES = 65536, 1024, (16, 64)   # kMoePrefill* of csrc/kernels.hpp


def _moe_pre_no(why):
    return QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "moe_prefill: " + why)


class MoeRoute:
    """What `moe_route` made: the workspace whose head holds the routing table on the device, and the sizes it was made for."""
    __slots__ = ("workspace", "tokens", "top_k", "num_experts", "tile_rows")

    def __init__(self, workspace, tokens, top_k, num_experts, tile_rows):
        self.workspace, self.tokens, self.top_k, self.num_experts, self.tile_rows = workspace, tokens, top_k, num_experts, tile_rows

    def table(self):
        """(tiles, counts [E], sorted slots of the tiles' rows [tiles * tile_rows] with -1 in padding rows, tile_expert [tiles], tile_row0
        [tiles]) read back from the device -- for tests and tools; nothing on the forward path calls it."""
        s, e = self.tokens * self.top_k, self.num_experts
        lo, hi = MOE_PREFILL_TILES
        max_tiles = s // lo + min(e, s)
        ints = self.workspace.view(torch.int32)
        tiles = int(ints[0])
        c0, te, t0 = 16, 16 + e, 16 + e + max_tiles
        srt = t0 + max_tiles
        return (tiles, ints[c0:c0 + e].cpu(), ints[srt:srt + tiles * self.tile_rows].cpu(), ints[te:te + tiles].cpu(), ints[t0:t0 + tiles].cpu())


def _moe_prefill_sizes(t: int, top_k: int, e: int, h: int, i: int, tile_rows):
    if not 1 <= top_k <= MOE_MAX_TOP_K:
        raise _moe_pre_no(f"top_k 1..{MOE_MAX_TOP_K} (got {top_k})")
    if t < 1 or t * top_k > MOE_PREFILL_MAX_SLOTS:
        raise _moe_pre_no(f"1..{MOE_PREFILL_MAX_SLOTS} slots T * top_k per call (got {t} x {top_k}): cut the rows into chunks")
    if not 1 <= e <= MOE_PREFILL_MAX_EXPERTS:
        raise _moe_pre_no(f"1..{MOE_PREFILL_MAX_EXPERTS} experts (got {e})")
    if h % 128 or i % 128 or h < 128 or i < 128:
        raise _moe_pre_no(f"H % 128 == 0 and I % 128 == 0 (got H={h} I={i})")
    if tile_rows is not None and tile_rows not in MOE_PREFILL_TILES:
        raise _moe_pre_no(f"tile_rows must be None or one of the built heights {MOE_PREFILL_TILES} (got {tile_rows})")
    return tile_rows if tile_rows is not None else (MOE_PREFILL_TILES[1] if t * top_k // e >= 32 else MOE_PREFILL_TILES[0])


def _moe_ids(ids, device=None):
    if (not isinstance(ids, torch.Tensor) or ids.dim() != 2 or ids.dtype != torch.int64 or not ids.is_contiguous()
            or (device is not None and ids.device != device)):
        raise _moe_pre_no(f"ids must be a contiguous int64 [T, top_k] tensor{'' if device is None else f' on {device}'}")
    return ids.shape


def moe_prefill_workspace_bytes(t: int, top_k: int, e: int, h: int, i: int) -> int:
    """Bytes of the workspace of one routed-experts call: the routing table and the [T * top_k, H] product rows (0: refused sizes)."""
    return int(_lib.load().qllm_moe_prefill_workspace_bytes(int(t), int(top_k), int(e), int(h), int(i)))


def moe_prefill_plan(x: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, gate, up, down, *, tile_rows=None):
    """What `moe_route`, `moe_prefill_gate_up` and `moe_prefill_down` are launched with for these tensors -- (T, top_k, E, H, I, tile_rows)
    -- or QllmUnsupported with the reason.  As `moe_plan`, but any T with T * top_k <= 65536, E <= 1024 and no bound on H; tile_rows None:
    64 where T * top_k / E >= 32, else 16; and, measured, T <= 512 or T * top_k <= 128 * E (beyond, the loop's GEMMs can win).  The three
    launchers themselves take every size up to their limits.  Pure host code, any device."""
    t, h = _moe_act("x", x, None, None)
    try:
        top_k = _moe_routing(ids, weights, t, x.dtype, x.device)
        if weights is None:
            raise _moe_no("weights must be given")
        (e, kg, ng), (eu, ku, nu), (ed, kd, nd) = (_moe_stack(n, s, x.device) for n, s in (("gate", gate), ("up", up), ("down", down)))
    except QllmUnsupported as err:
        raise _moe_pre_no(str(err).split("moe_decode: ", 1)[-1]) from None
    if (eu, ku, nu) != (e, kg, ng) or (ed, kd, nd) != (e, ng, kg) or kg != h:
        raise _moe_pre_no(f"gate and up must be [{h} -> I] and down [I -> {h}] stacks of one expert count (got {(e, kg, ng)}, {(eu, ku, nu)}, {(ed, kd, nd)})")
    if len({s[2] is None for s in (gate, up, down)}) != 1:
        raise _moe_pre_no("the three stacks must all have packed zero points or all be symmetric")
    bm = _moe_prefill_sizes(t, top_k, e, h, ng, tile_rows)
    if t > 512 and t * top_k > 128 * e:
        # measured (profiles/moe_prefill.md): at Mixtral's sizes and 2048 tokens the launches win x1.30 under uniform routing and LOSE x0.89
        # with every token on two experts -- the loop's GEMMs read an expert once for thousands of rows, a 64-row tile re-reads its panel;
        # 512 tokens win under both routings.  The routing is not known on the host, so the whole region is the loop's.
        raise _moe_pre_no(f"with {t} tokens and {t * top_k // e} rows per expert on average the loop's GEMMs can be faster (served: T <= 512 or T * top_k <= 128 * E)")
    return t, top_k, e, h, ng, bm


def moe_prefill_describe(t: int, top_k: int, e: int, h: int, i: int, tile_rows=None) -> str:
    """Tile height, grids and LDS of the four launches ("moe_prefill tile_rows=16 route grid=1 ... | combine grid=1x16"), or "refused: ...".
    Pure host code."""
    return _describe("qllm_moe_prefill_describe", 384, int(t), int(top_k), int(e), int(h), int(i), int(tile_rows or 0))


def moe_route(ids: torch.Tensor, num_experts: int, *, tile_rows=None, workspace=None) -> MoeRoute:
    """The routing table of ids [T, top_k] (int64, on the device) in ONE launch (qllm_moe_route, csrc/moe_prefill.hip): per-expert counts,
    the slots sorted by expert (stable), every expert's segment padded to row tiles of `tile_rows` rows, per tile its expert and first row.
    Ids outside [0, num_experts) are dropped.  `workspace`: a uint8 tensor of at least `moe_prefill_workspace_bytes` bytes (the down
    projection keeps its per-slot rows there); None: the table alone is allocated, enough for `moe_prefill_gate_up`."""
    t, top_k = _moe_ids(ids)
    e = int(num_experts)
    bm = _moe_prefill_sizes(t, top_k, e, 128, 128, tile_rows)
    if not ids.is_cuda:
        raise RuntimeError("moe_route: ids must be a HIP/CUDA tensor (qllm_amd has no CPU forward path)")
    if workspace is None:
        workspace = torch.empty(moe_prefill_workspace_bytes(t, top_k, e, 128, 128), dtype=torch.uint8, device=ids.device)
    elif workspace.dtype != torch.uint8 or workspace.device != ids.device or not workspace.is_contiguous() or workspace.data_ptr() % 256:
        raise RuntimeError(f"workspace must be a contiguous, 256-byte aligned uint8 tensor on {ids.device}")
    with torch.cuda.device(ids.device):
        rc = _lib.load().qllm_moe_route(ids.data_ptr(), workspace.data_ptr(), workspace.numel(), t, top_k, e, bm, _stream_ptr())
    _lib.check(rc)
    return MoeRoute(workspace, t, top_k, e, bm)


def _moe_route_for(route, ids, e):
    if not isinstance(route, MoeRoute) or (route.tokens, route.top_k) != tuple(ids.shape) or route.num_experts != e or route.workspace.device != ids.device:
        raise _moe_pre_no(f"route must be moe_route's result for ids {tuple(ids.shape)} over {e} experts on {ids.device}")


def moe_prefill_gate_up(x: torch.Tensor, ids: torch.Tensor, route: MoeRoute, gate, up, *, add_zero_bias: int = 0, out=None) -> torch.Tensor:
    """`moe_gate_up`'s h [T * top_k, I] for any number of tokens: a grouped MFMA GEMM over the row tiles of `route`
    (qllm_moe_prefill_gate_up, csrc/moe_prefill.hip), the eager roundings, rows of dropped slots left unwritten."""
    t, h = _moe_act("x", x, None, None)
    _moe_ids(ids, x.device)
    try:
        (e, kg, ng), (eu, ku, nu) = _moe_stack("gate", gate, x.device), _moe_stack("up", up, x.device)
    except QllmUnsupported as err:
        raise _moe_pre_no(str(err).split("moe_decode: ", 1)[-1]) from None
    if (eu, ku, nu) != (e, kg, ng) or kg != h or (gate[2] is None) != (up[2] is None) or ids.shape[0] != t:
        raise _moe_pre_no(f"gate and up must be [{h} -> I] stacks of one expert count and one kind of zero point, ids [{t}, top_k]")
    _moe_route_for(route, ids, e)
    top_k = ids.shape[1]
    _moe_prefill_sizes(t, top_k, e, h, ng, route.tile_rows)
    if not x.is_cuda:
        raise RuntimeError("moe_prefill_gate_up: x must be a HIP/CUDA tensor (qllm_amd has no CPU forward path)")
    out = _moe_out("out", out, (t * top_k, ng), x)
    ws = route.workspace
    with torch.cuda.device(x.device):
        rc = _lib.load().qllm_moe_prefill_gate_up(x.data_ptr(), ws.data_ptr(), ws.numel(), gate[0].data_ptr(), gate[1].data_ptr(), _ptr(gate[2]),
                                                  up[0].data_ptr(), up[1].data_ptr(), _ptr(up[2]), out.data_ptr(), t, top_k, e, h, ng, route.tile_rows,
                                                  int(add_zero_bias), _act_dtype(x), _stream_ptr())
    _lib.check(rc)
    return out


def moe_prefill_down(h: torch.Tensor, ids: torch.Tensor, weights: torch.Tensor, route: MoeRoute, down, *, add_zero_bias: int = 0, out=None) -> torch.Tensor:
    """`moe_down`'s y [T, H] for any number of tokens, in two launches of one call (qllm_moe_prefill_down): the grouped down projection
    writes round(round(d) * w) per slot into the route's workspace, the combine adds a token's rows in ascending expert id with one
    rounding per add.  The route's workspace must have `moe_prefill_workspace_bytes` bytes."""
    _moe_ids(ids, h.device if isinstance(h, torch.Tensor) else None)
    t, top_k = ids.shape
    try:
        e, i, hh = _moe_stack("down", down, h.device)
        _moe_routing(ids, weights, t, h.dtype, h.device)
        if weights is None:
            raise _moe_no("weights must be given")
        _moe_act("h", h, t * top_k, i)
    except QllmUnsupported as err:
        raise _moe_pre_no(str(err).split("moe_decode: ", 1)[-1]) from None
    _moe_route_for(route, ids, e)
    _moe_prefill_sizes(t, top_k, e, hh, i, route.tile_rows)
    if not h.is_cuda:
        raise RuntimeError("moe_prefill_down: h must be a HIP/CUDA tensor (qllm_amd has no CPU forward path)")
    out = _moe_out("out", out, (t, hh), h)
    ws = route.workspace
    wdt = _lib.DT_F32 if weights.dtype == torch.float32 else _act_dtype(h)
    with torch.cuda.device(h.device):
        rc = _lib.load().qllm_moe_prefill_down(h.data_ptr(), ids.data_ptr(), weights.data_ptr(), ws.data_ptr(), ws.numel(), down[0].data_ptr(),
                                               down[1].data_ptr(), _ptr(down[2]), out.data_ptr(), t, top_k, e, hh, i, route.tile_rows, int(add_zero_bias),
                                               wdt, _act_dtype(h), _stream_ptr())
    _lib.check(rc)
    return out


ATTN_DECODE_HEAD_DIMS = (64, 128)   # what csrc/attn_decode.hip is built for
ATTN_DECODE_MAX_GROUP = 8           # kAttnDecodeMaxGroup of csrc/kernels.hpp
ATTN_DECODE_COUNTERS = 4096         # kCounterBytes / sizeof(int) of csrc/planner.hpp: attn_decode takes one arrival counter per (sequence, kv
                                    # head) from the counter page at the head of the workspace


def _attn_heads(t: torch.Tensor, name: str):
    """(batch, heads, head_dim, row stride, head stride) of a one-token q / k_new / v_new given as [B, H, 1, D] or [B, 1, H, D]."""
    if t.dim() != 4 or (t.shape[2] != 1 and t.shape[1] != 1):
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"attn_decode: {name} must be one token, [B, H, 1, D] or [B, 1, H, D] (got {tuple(t.shape)})")
    hd = 1 if t.shape[2] == 1 else 2
    b, h, d = t.shape[0], t.shape[hd], t.shape[3]
    if b == 0 or h == 0 or d == 0:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"attn_decode: empty {name}")
    if d > 1 and t.stride(3) != 1:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"attn_decode: the last dimension of {name} must have stride 1 (got {t.stride(3)})")
    row = t.stride(0) if b > 1 else h * d
    head = t.stride(hd) if h > 1 else d
    if row % 8 or head % 8 or row < 0 or head < 0 or t.data_ptr() % 16:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"attn_decode: {name} must be 16-byte aligned with strides that are multiples of 8 (row {row}, head {head})")
    return b, h, d, row, head


def _attn_window(window, name: str) -> int:
    """The `window` keyword of attn_decode / attn_prefill as the C entries take it: None -> 0 (no window), an int >= 1 -> itself;
    anything else is refused."""
    if window is None:
        return 0
    if isinstance(window, bool) or not isinstance(window, int) or window < 1:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, f"{name}: window must be None or an int >= 1 (got {window!r})")
    return window


# ---- the rules attn_decode_plan and attn_prefill_plan share, each written once; `no(why)` makes the caller's QllmUnsupported ----------------
def _attn_refusal(name: str):
    return lambda why: QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, name + ": " + why)


def _attn_one_type_and_device(no, who: str, ts, mask):
    """q (ts[0]) and the other tensors of `ts` -- `who` names them -- have one fp16 / bf16 type, and with the mask one device."""
    dtype, device = ts[0].dtype, ts[0].device
    if dtype not in (torch.float16, torch.bfloat16) or [t.dtype for t in ts].count(dtype) != len(ts):
        raise no(who + " must share one type, float16 or bfloat16 (got " + ", ".join(str(t.dtype)[6:] for t in ts) + ")")
    if [t.device for t in ts].count(device) != len(ts) or (mask is not None and mask.device != device):
        raise no("every tensor must be on one device")


def _attn_cache_shape(no, k_cache, v_cache, b: int, d: int):
    """(kv heads, positions) of two [B, Hkv, L, D] caches of one shape and layout that go with q's B and D."""
    shape = k_cache.shape
    if len(shape) != 4 or shape != v_cache.shape or k_cache.stride() != v_cache.stride() or shape[0] != b or shape[3] != d:
        raise no(f"the caches must be two [B, Hkv, L, D] tensors of one shape and layout with q's B and D (got {tuple(shape)}, {tuple(v_cache.shape)})")
    if shape[1] == 0 or shape[2] == 0:
        raise no("empty caches")
    return shape[1], shape[2]


def _attn_served_heads(no, hq: int, hkv: int, d: int):
    if hq % hkv:
        raise no(f"the kv heads must divide the query heads (got {hq}, {hkv})")
    if d not in ATTN_DECODE_HEAD_DIMS:
        raise no(f"head_dim 64 or 128 (got {d})")
    if hq // hkv > ATTN_DECODE_MAX_GROUP:
        raise no(f"at most {ATTN_DECODE_MAX_GROUP} query heads per kv head (got {hq // hkv})")


def _attn_cache_strides(no, k_cache, v_cache):
    """The caches' batch, head and position strides (0 for a dimension of one entry); behind the head rules, as the refusals are ordered."""
    shape, strides = k_cache.shape, k_cache.stride()
    cs = tuple([strides[i] if shape[i] > 1 else 0 for i in range(3)])
    if strides[3] != 1 or [x for x in cs if x % 8 or x < 0] or k_cache.data_ptr() % 16 or v_cache.data_ptr() % 16:
        raise no(f"the caches must have contiguous head rows, 16-byte aligned, with strides that are multiples of 8 (got {strides})")
    return cs


def _attn_length_on_device(no, length, q) -> bool:
    """Whether `length` is a tensor the kernel reads: then a 0-d int64 one on q's device."""
    if not isinstance(length, torch.Tensor):
        return False
    if length.dim() != 0 or length.dtype != torch.int64 or length.device != q.device:
        raise no("a length on the device must be a 0-d int64 tensor on q's device")
    return True


def _attn_mask_kind(no, mask, q, mask_len: int, need: int, *strides) -> int:
    """The kind of a mask whose form the caller has accepted: bool, or additive in q's type; it covers the `need` positions the call may reach."""
    if mask.dtype == torch.bool:
        kind = _lib.ATTN_MASK_BOOL
    elif mask.dtype == q.dtype and mask.data_ptr() % 2 == 0:
        kind = _lib.ATTN_MASK_ADDITIVE
    else:
        raise no(f"the mask must be bool or additive in {str(q.dtype)[6:]} (got {str(mask.dtype)[6:]})")
    if mask_len < need or min(strides) < 0:
        raise no(f"the mask must cover {need} positions (got {mask_len})")
    return kind


def _attn_call(name: str, q, k_cache, v_cache, length, scaling, out, shape, d: int):
    """What attn_decode and attn_prefill settle behind the plan: device tensors, `out` (made when None), and (out, kv_len, kv_len_dev,
    scaling) as the C entries take them."""
    for t in (q, k_cache, v_cache):
        if not t.is_cuda:
            raise RuntimeError(f"{name}: q and the caches must be HIP/CUDA tensors (qllm_amd has no CPU forward path)")
    if out is None:
        out = torch.empty(shape, dtype=q.dtype, device=q.device)
    elif out.shape != shape or out.dtype != q.dtype or out.device != q.device or not out.is_contiguous():
        raise RuntimeError(f"{name}: out must be a contiguous {shape} {q.dtype} tensor on {q.device}")
    on_device = isinstance(length, torch.Tensor)
    return out, 0 if on_device else int(length), length.data_ptr() if on_device else None, float(d ** -0.5 if scaling is None else scaling)


def attn_decode_plan(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, k_new: Optional[torch.Tensor] = None,
                     v_new: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """What `attn_decode` hands to qllm_attn_decode for these tensors -- (batch, q_heads, kv_heads, head_dim, max_len, q row / head stride,
    k_new row / head stride, v_new row / head stride, cache batch / head / position stride, mask_kind, mask_len, mask batch stride) -- or
    QllmUnsupported with the reason.  q (and k_new / v_new, both or neither): one token, [B, H, 1, D] or [B, 1, H, D] views of one fp16 /
    bf16 type, inner stride 1, 16-byte aligned, strides multiples of 8; caches [B, Hkv, L, D] of that type with contiguous D and the same
    strides; Hkv divides Hq, at most 8 query heads per kv head; D 64 or 128; mask None, [B, 1, 1, L'] or [B, L'] (B or 1 rows), bool or of
    the activation type, inner stride 1; `length` an int (0..L, L - 1 at most with an append; the mask covers it) or a 0-d int64 tensor on
    the device (the mask then covers L).  Pure host code, any device."""
    no = _attn_refusal("attn_decode")
    if (k_new is None) != (v_new is None):
        raise no("k_new and v_new must be given together or not at all")
    _attn_one_type_and_device(no, "q, the caches and k_new / v_new", (q, k_cache, v_cache) + ((k_new, v_new) if k_new is not None else ()), mask)
    b, hq, d, q_row, q_head = _attn_heads(q, "q")
    hkv, max_len = _attn_cache_shape(no, k_cache, v_cache, b, d)
    _attn_served_heads(no, hq, hkv, d)
    if b * hkv > ATTN_DECODE_COUNTERS or b > 65535:
        raise no(f"batch * kv_heads <= {ATTN_DECODE_COUNTERS} (got {b * hkv})")
    cs = _attn_cache_strides(no, k_cache, v_cache)
    new = (0, 0, 0, 0)
    if k_new is not None:
        kb, kh, kd, k_row, k_head = _attn_heads(k_new, "k_new")
        vb, vh, vd, v_row, v_head = _attn_heads(v_new, "v_new")
        if (kb, kh, kd) != (b, hkv, d) or (vb, vh, vd) != (b, hkv, d):
            raise no(f"k_new and v_new must be one token of [{b}, {hkv}, {d}] (got {tuple(k_new.shape)}, {tuple(v_new.shape)})")
        new = (k_row, k_head, v_row, v_head)
    need = max_len
    if not _attn_length_on_device(no, length, q):
        length = int(length)
        need = length + (1 if k_new is not None else 0)
        if length < 0 or need > max_len:
            raise no(f"the length{' + 1 (append)' if k_new is not None else ''} must lie in 0..{max_len} (got {length})")
    kind, mask_len, mask_batch = _lib.ATTN_MASK_NONE, 0, 0
    if mask is not None:
        m2 = mask[:, 0, 0] if mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1 else mask
        if m2.dim() != 2 or m2.shape[0] not in (1, b) or (m2.shape[1] > 1 and m2.stride(1) != 1):
            raise no(f"the mask must be [B, 1, 1, L] or [B, L] with B = {b} or 1 and inner stride 1 (got {tuple(mask.shape)}, strides {tuple(mask.stride())})")
        mask_len, mask_batch = m2.shape[1], (m2.stride(0) if m2.shape[0] > 1 else 0)
        kind = _attn_mask_kind(no, mask, q, mask_len, need, mask_batch)
    return (b, hq, hkv, d, max_len, q_row, q_head) + new + cs + (kind, mask_len, mask_batch)


def attn_decode_describe(batch: int, q_heads: int, kv_heads: int, head_dim: int, max_len: int) -> str:
    """The launch `attn_decode` makes for these shapes ("attn_decode tile=64 splits=16 chunk=256 grid=16x32x1 group=1 combine=last-block"), or
    "refused: ...".  Pure host code: a function of the shapes and the device's CU count, never of the length."""
    return _describe("qllm_attn_decode_describe", 256, int(batch), int(q_heads), int(kv_heads), int(head_dim), int(max_len))


def attn_decode(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, k_new: Optional[torch.Tensor] = None,
                v_new: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, scaling: Optional[float] = None, *, out=None, plan=None,
                window: Optional[int] = None):
    """softmax(scaling * q K^T + mask) V for one query token per sequence over the first `length` positions of the caches [B, Hkv, L, D], as
    ONE kernel (qllm_attn_decode, csrc/attn_decode.hip): a K / V row is read once for all query heads of its kv head, positions >= length
    are never loaded, fp32 scores and softmax, one rounding at the store.  Returns [B, Hq, D] (contiguous: the row o_proj takes).
    `length`: an int, or a 0-d int64 tensor on the device that the kernel reads (a captured call then serves every length).  k_new / v_new:
    the new token's rows; the kernel stores them at position `length` of the caches and attends over length + 1 positions (with the
    length on the device and length + 1 > L it stores nothing and attends over the first L positions).  mask: [B, 1, 1, L'] or [B, L'],
    bool (True = visible) or additive; a row with no visible key gives zeros.  scaling: D ** -0.5 when None.  `attn_decode_plan` says what
    is served; everything else raises QllmUnsupported before anything is launched.  plan: what it returned for these very arguments.
    window: None, or an int W >= 1 -- a sliding window on the linear cache: the query (the last counted position, the appended token
    included) sees the last W counted positions only, in addition to length and mask; earlier positions are never loaded, and with the
    length on the device the lower end follows it.  The plan does not depend on the window; None gives the bits of a call without it."""
    window = _attn_window(window, "attn_decode")
    if plan is None:
        plan = attn_decode_plan(q, k_cache, v_cache, length, k_new, v_new, mask)
    b, hq, hkv, d, max_len = plan[:5]
    out, kv_len, kv_len_dev, scaling = _attn_call("attn_decode", q, k_cache, v_cache, length, scaling, out, (b, hq, d), d)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        nbytes = lib.qllm_attn_decode_workspace_bytes(b, hq, hkv, d, max_len)
        ws = workspace(q.device, nbytes)
        rc = lib.qllm_attn_decode_window(q.data_ptr(), _ptr(k_new), _ptr(v_new), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(mask), out.data_ptr(),
                                         b, hq, hkv, d, kv_len, kv_len_dev, max_len, window, *plan[5:], scaling, _act_dtype(q), ws.data_ptr(), ws.numel(),
                                         _stream_ptr())
    _lib.check(rc)
    return out


def attn_decode_ring_plan(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, total, window, k_new: Optional[torch.Tensor] = None,
                          v_new: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """What `attn_decode_ring` hands to qllm_attn_decode_ring for these tensors -- (batch, q_heads, kv_heads, head_dim, slots, window, q row /
    head stride, k_new row / head stride, v_new row / head stride, cache batch / head / position stride, mask_kind, mask_len, mask batch
    stride) -- or QllmUnsupported with the reason.  Tensors as `attn_decode_plan` takes them, the caches [B, Hkv, C, D] with C slots;
    `window` an int W with 1 <= W <= C; `total` an int >= 0 with no upper end (the mask covers min(total, + 1 with an append; W) columns)
    or a 0-d int64 tensor on the device (the mask then covers W).  Pure host code, any device."""
    no = _attn_refusal("attn_decode_ring")
    if (k_new is None) != (v_new is None):
        raise no("k_new and v_new must be given together or not at all")
    _attn_one_type_and_device(no, "q, the caches and k_new / v_new", (q, k_cache, v_cache) + ((k_new, v_new) if k_new is not None else ()), mask)
    b, hq, d, q_row, q_head = _attn_heads(q, "q")
    hkv, slots = _attn_cache_shape(no, k_cache, v_cache, b, d)
    if isinstance(window, bool) or not isinstance(window, int) or window < 1 or window > slots:
        raise no(f"window must be an int in 1..{slots}, the caches' slots (got {window!r})")
    _attn_served_heads(no, hq, hkv, d)
    if b * hkv > ATTN_DECODE_COUNTERS or b > 65535:
        raise no(f"batch * kv_heads <= {ATTN_DECODE_COUNTERS} (got {b * hkv})")
    cs = _attn_cache_strides(no, k_cache, v_cache)
    new = (0, 0, 0, 0)
    if k_new is not None:
        kb, kh, kd, k_row, k_head = _attn_heads(k_new, "k_new")
        vb, vh, vd, v_row, v_head = _attn_heads(v_new, "v_new")
        if (kb, kh, kd) != (b, hkv, d) or (vb, vh, vd) != (b, hkv, d):
            raise no(f"k_new and v_new must be one token of [{b}, {hkv}, {d}] (got {tuple(k_new.shape)}, {tuple(v_new.shape)})")
        new = (k_row, k_head, v_row, v_head)
    need = window
    if not _attn_length_on_device(no, total, q):
        total = int(total)
        if total < 0:
            raise no(f"the total must be >= 0 (got {total})")
        need = min(total + (1 if k_new is not None else 0), window)
    kind, mask_len, mask_batch = _lib.ATTN_MASK_NONE, 0, 0
    if mask is not None:
        m2 = mask[:, 0, 0] if mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1 else mask
        if m2.dim() != 2 or m2.shape[0] not in (1, b) or (m2.shape[1] > 1 and m2.stride(1) != 1):
            raise no(f"the mask must be [B, 1, 1, L] or [B, L] with B = {b} or 1 and inner stride 1 (got {tuple(mask.shape)}, strides {tuple(mask.stride())})")
        mask_len, mask_batch = m2.shape[1], (m2.stride(0) if m2.shape[0] > 1 else 0)
        kind = _attn_mask_kind(no, mask, q, mask_len, need, mask_batch)
    return (b, hq, hkv, d, slots, window, q_row, q_head) + new + cs + (kind, mask_len, mask_batch)


def attn_decode_ring(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, total, window, k_new: Optional[torch.Tensor] = None,
                     v_new: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, scaling: Optional[float] = None, *, out=None, plan=None):
    """`attn_decode` over a RING-BUFFER cache [B, Hkv, C, D] in which position j lives in slot j mod C, as ONE kernel
    (qllm_attn_decode_ring, csrc/attn_decode_ring.hip): what a sliding-window layer needs past its window without moving a row.  `total`:
    the tokens counted before the call, an int or a 0-d int64 tensor on the device that the kernel reads; it has no upper end.  With
    k_new / v_new the call appends: n = total + 1 and the kernel stores the rows in slot (n - 1) mod C; without, n = total.  The query
    sits at n - 1 and sees positions lo = max(0, n - W) .. n - 1 (`window` = W, 1 <= W <= C); no other slot is loaded.  mask: as
    `attn_decode`'s, with column r standing for position lo + r (the mask transformers builds for a sliding layer).  Returns [B, Hq, D]:
    bit for bit what `attn_decode` gives on a linear copy [B, Hkv, W, D] of the visible positions.  The launch is that of
    `attn_decode_describe(B, Hq, Hkv, D, W)` and never depends on the total: one captured call serves every length.
    `attn_decode_ring_plan` says what is served; everything else raises QllmUnsupported before anything is launched."""
    if plan is None:
        plan = attn_decode_ring_plan(q, k_cache, v_cache, total, window, k_new, v_new, mask)
    b, hq, hkv, d, slots, window = plan[:6]
    out, total, total_dev, scaling = _attn_call("attn_decode_ring", q, k_cache, v_cache, total, scaling, out, (b, hq, d), d)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        nbytes = lib.qllm_attn_decode_workspace_bytes(b, hq, hkv, d, window)
        ws = workspace(q.device, nbytes)
        rc = lib.qllm_attn_decode_ring(q.data_ptr(), _ptr(k_new), _ptr(v_new), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(mask), out.data_ptr(),
                                       b, hq, hkv, d, total, total_dev, slots, window, *plan[6:], scaling, _act_dtype(q), ws.data_ptr(), ws.numel(),
                                       _stream_ptr())
    _lib.check(rc)
    return out


# ---- the quantized KV cache (csrc/kv_quant.hpp has the format; csrc/attn_decode_quant.hip, csrc/kv_quant.hip) --------------------------------
KV_QUANT_BITS = (8, 4)


def kv_quant_shapes(head_dim: int, bits: int):
    """(bytes of codes, number of params) per cached row: D * bits / 8 and D / 32 scales at 8 bits, D / 16 scales-then-zeros at 4."""
    return head_dim * bits // 8, head_dim // 32 * (2 if bits == 4 else 1)


def _kvq_strides(t):
    return tuple([t.stride(i) if t.shape[i] > 1 else 0 for i in range(3)])


def _kvq_cache(no, codes, params, bits, b: int, hkv, d: int, dtype, device):
    """(kv heads, positions, codes strides in bytes, params strides in elements) of one cache's two tensors."""
    if isinstance(bits, bool) or bits not in KV_QUANT_BITS:
        raise no(f"bits must be 8 or 4 (got {bits!r})")
    if d not in ATTN_DECODE_HEAD_DIMS:
        raise no(f"head_dim 64 or 128 (got {d})")
    cb, np_ = kv_quant_shapes(d, bits)
    if codes.dtype != torch.uint8 or params.dtype != dtype or codes.device != device or params.device != device:
        raise no(f"codes must be uint8 and params {str(dtype)[6:]}, on one device (got {str(codes.dtype)[6:]}, {str(params.dtype)[6:]})")
    if codes.dim() != 4 or params.dim() != 4 or codes.shape[:3] != params.shape[:3] or codes.shape[0] != b or codes.shape[3] != cb or params.shape[3] != np_ \
            or (hkv is not None and codes.shape[1] != hkv) or codes.shape[1] == 0 or codes.shape[2] == 0:
        raise no(f"codes must be [B, Hkv, L, {cb}] and params [B, Hkv, L, {np_}] with B = {b} (got {tuple(codes.shape)}, {tuple(params.shape)})")
    cs, ps = _kvq_strides(codes), _kvq_strides(params)
    if codes.stride(3) != 1 or params.stride(3) != 1 or [x for x in cs if x % 8 or x < 0] or [x for x in ps if x % 2 or x < 0] or codes.data_ptr() % 16 \
            or params.data_ptr() % 4:
        raise no(f"codes must be 16-byte aligned with strides that are multiples of 8, params 4-byte aligned with strides that are multiples of 2 "
                 f"(got {tuple(codes.stride())}, {tuple(params.stride())})")
    return codes.shape[1], codes.shape[2], cs, ps


def _kvq_count(count):
    on_device = isinstance(count, torch.Tensor)
    return (0, count.data_ptr()) if on_device else (int(count), None)


def _kvq_rows(no, t: torch.Tensor, name: str):
    """(batch, kv heads, rows, head_dim, batch / head / row stride) of act rows [B, Hkv, S, D]: any view with a contiguous D."""
    if t.dim() != 4 or t.dtype not in (torch.float16, torch.bfloat16) or 0 in t.shape[:2] or t.shape[3] == 0:
        raise no(f"{name} must be a float16 / bfloat16 [B, Hkv, S, D] tensor (got {tuple(t.shape)} {str(t.dtype)[6:]})")
    st = _kvq_strides(t)
    if (t.shape[3] > 1 and t.stride(3) != 1) or [x for x in st if x % 8 or x < 0] or t.data_ptr() % 16:
        raise no(f"{name} must be 16-byte aligned with a contiguous last dimension and strides that are multiples of 8 (got {tuple(t.stride())})")
    return t.shape[0], t.shape[1], t.shape[2], t.shape[3], st


def kv_quantize(src: torch.Tensor, codes: torch.Tensor, params: torch.Tensor, bits: int, pos0=0):
    """Quantise the act rows `src` [B, Hkv, S, D] (any strided view with a contiguous D: the transposed [B, S, H, D] projection output is
    read in place) into positions pos0 .. pos0 + S - 1 of a quantized cache (qllm_kv_quantize, csrc/kv_quant.hip).  pos0: an int, or a 0-d
    int64 tensor on the device that the kernel reads.  No byte outside those positions is written.  QllmUnsupported before any launch."""
    no = _attn_refusal("kv_quantize")
    b, hkv, rows, d, st = _kvq_rows(no, src, "src")
    _, max_len, cs, ps = _kvq_cache(no, codes, params, bits, b, hkv, d, src.dtype, src.device)
    on_device = _attn_length_on_device(no, pos0, src)
    if not on_device and (int(pos0) < 0 or int(pos0) + rows > max_len):
        raise no(f"pos0 .. pos0 + {rows} must lie in 0..{max_len} (got {int(pos0)})")
    if not src.is_cuda:
        raise RuntimeError("kv_quantize: the tensors must be HIP/CUDA tensors (qllm_amd has no CPU forward path)")
    pos, pos_dev = _kvq_count(pos0)
    with torch.cuda.device(src.device):
        rc = _lib.load().qllm_kv_quantize(src.data_ptr(), codes.data_ptr(), params.data_ptr(), b, hkv, rows, d, bits, pos, pos_dev, max_len, *st, *cs, *ps,
                                          _act_dtype(src), _stream_ptr())
    _lib.check(rc)


def kv_dequantize(codes: torch.Tensor, params: torch.Tensor, bits: int, n, out: torch.Tensor):
    """Positions 0 .. n - 1 of a quantized cache into `out`, act [B, Hkv, L', D] (qllm_kv_dequantize): each value s * code / fma(code, s,
    z) in fp32, rounded once.  n: an int in 0..min(L, L'), or a 0-d int64 tensor on the device (clamped to that range).  Positions of `out`
    at or beyond n are not written.  Returns `out`."""
    no = _attn_refusal("kv_dequantize")
    b, hkv, dst_len, d, st = _kvq_rows(no, out, "out")
    _, max_len, cs, ps = _kvq_cache(no, codes, params, bits, b, hkv, d, out.dtype, out.device)
    on_device = _attn_length_on_device(no, n, out)
    if not on_device and not 0 <= int(n) <= min(max_len, dst_len):
        raise no(f"n must lie in 0..{min(max_len, dst_len)} (got {int(n)})")
    if not out.is_cuda:
        raise RuntimeError("kv_dequantize: the tensors must be HIP/CUDA tensors (qllm_amd has no CPU forward path)")
    cnt, cnt_dev = _kvq_count(n)
    with torch.cuda.device(out.device):
        rc = _lib.load().qllm_kv_dequantize(codes.data_ptr(), params.data_ptr(), out.data_ptr(), b, hkv, d, bits, cnt, cnt_dev, max_len, dst_len, *cs, *ps, *st,
                                            _act_dtype(out), _stream_ptr())
    _lib.check(rc)
    return out


def attn_decode_quant_plan(q: torch.Tensor, k_codes: torch.Tensor, k_params: torch.Tensor, v_codes: torch.Tensor, v_params: torch.Tensor, bits: int, length,
                           k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
    """What `attn_decode_quant` hands to qllm_attn_decode_quant -- (batch, q_heads, kv_heads, head_dim, bits, max_len, q row / head stride,
    k_new and v_new row / head strides, codes batch / head / position stride in bytes, params likewise in elements, mask_kind, mask_len,
    mask batch stride) -- or QllmUnsupported with the reason.  q, k_new / v_new, mask and length as `attn_decode_plan` takes them; codes
    uint8 [B, Hkv, L, D * bits / 8] and params [B, Hkv, L, P] of q's type, K and V of one shape and layout.  Pure host code, any device."""
    no = _attn_refusal("attn_decode_quant")
    if (k_new is None) != (v_new is None):
        raise no("k_new and v_new must be given together or not at all")
    _attn_one_type_and_device(no, "q and k_new / v_new", (q,) + ((k_new, v_new) if k_new is not None else ()), mask)
    b, hq, d, q_row, q_head = _attn_heads(q, "q")
    hkv, max_len, cs, ps = _kvq_cache(no, k_codes, k_params, bits, b, None, d, q.dtype, q.device)
    if _kvq_cache(no, v_codes, v_params, bits, b, hkv, d, q.dtype, q.device) != (hkv, max_len, cs, ps):
        raise no("the K and the V cache must have one shape and layout")
    _attn_served_heads(no, hq, hkv, d)
    if b * hkv > ATTN_DECODE_COUNTERS or b > 65535:
        raise no(f"batch * kv_heads <= {ATTN_DECODE_COUNTERS} (got {b * hkv})")
    new = (0, 0, 0, 0)
    if k_new is not None:
        kb, kh, kd, k_row, k_head = _attn_heads(k_new, "k_new")
        vb, vh, vd, v_row, v_head = _attn_heads(v_new, "v_new")
        if (kb, kh, kd) != (b, hkv, d) or (vb, vh, vd) != (b, hkv, d):
            raise no(f"k_new and v_new must be one token of [{b}, {hkv}, {d}] (got {tuple(k_new.shape)}, {tuple(v_new.shape)})")
        new = (k_row, k_head, v_row, v_head)
    need = max_len
    if not _attn_length_on_device(no, length, q):
        length = int(length)
        need = length + (1 if k_new is not None else 0)
        if length < 0 or need > max_len:
            raise no(f"the length{' + 1 (append)' if k_new is not None else ''} must lie in 0..{max_len} (got {length})")
    kind, mask_len, mask_batch = _lib.ATTN_MASK_NONE, 0, 0
    if mask is not None:
        m2 = mask[:, 0, 0] if mask.dim() == 4 and mask.shape[1] == 1 and mask.shape[2] == 1 else mask
        if m2.dim() != 2 or m2.shape[0] not in (1, b) or (m2.shape[1] > 1 and m2.stride(1) != 1):
            raise no(f"the mask must be [B, 1, 1, L] or [B, L] with B = {b} or 1 and inner stride 1 (got {tuple(mask.shape)}, strides {tuple(mask.stride())})")
        mask_len, mask_batch = m2.shape[1], (m2.stride(0) if m2.shape[0] > 1 else 0)
        kind = _attn_mask_kind(no, mask, q, mask_len, need, mask_batch)
    return (b, hq, hkv, d, bits, max_len, q_row, q_head) + new + cs + ps + (kind, mask_len, mask_batch)


def attn_decode_quant_describe(batch: int, q_heads: int, kv_heads: int, head_dim: int, bits: int, max_len: int) -> str:
    """The launch `attn_decode_quant` makes ("attn_decode_quant bits=8 tile=64 splits=16 chunk=256 grid=16x32x1 group=1 combine=last-block"),
    or "refused: ...".  Pure host code; the geometry is `attn_decode_describe`'s for the same shapes."""
    return _describe("qllm_attn_decode_quant_describe", 256, int(batch), int(q_heads), int(kv_heads), int(head_dim), int(bits), int(max_len))


def attn_decode_quant(q: torch.Tensor, k_codes: torch.Tensor, k_params: torch.Tensor, v_codes: torch.Tensor, v_params: torch.Tensor, bits: int, length,
                      k_new: Optional[torch.Tensor] = None, v_new: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None,
                      scaling: Optional[float] = None, *, out=None, plan=None):
    """`attn_decode` over a QUANTIZED cache, read in place, as ONE kernel (qllm_attn_decode_quant, csrc/attn_decode_quant.hip): 8-bit
    symmetric or 4-bit asymmetric codes with one scale (and zero) per 32 elements (`kv_quantize` writes the format).  q, length, mask,
    scaling and the result [B, Hq, D] are `attn_decode`'s.  k_new / v_new: the new token's rows; the kernel quantises them, stores codes
    and params at position `length` and attends over the dequantised row -- always attention over what the cache now holds (no
    full-precision residual).  `attn_decode_quant_plan` says what is served; everything else raises QllmUnsupported before any launch."""
    if plan is None:
        plan = attn_decode_quant_plan(q, k_codes, k_params, v_codes, v_params, bits, length, k_new, v_new, mask)
    b, hq, hkv, d, bits, max_len = plan[:6]
    out, kv_len, kv_len_dev, scaling = _attn_call("attn_decode_quant", q, k_codes, v_codes, length, scaling, out, (b, hq, d), d)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        nbytes = lib.qllm_attn_decode_workspace_bytes(b, hq, hkv, d, max_len)
        ws = workspace(q.device, nbytes)
        rc = lib.qllm_attn_decode_quant(q.data_ptr(), _ptr(k_new), _ptr(v_new), k_codes.data_ptr(), k_params.data_ptr(), v_codes.data_ptr(), v_params.data_ptr(),
                                        _ptr(mask), out.data_ptr(), b, hq, hkv, d, bits, kv_len, kv_len_dev, max_len, *plan[6:], scaling, _act_dtype(q),
                                        ws.data_ptr(), ws.numel(), _stream_ptr())
    _lib.check(rc)
    return out


def attn_prefill_plan(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, mask: Optional[torch.Tensor] = None):
    """What `attn_prefill` hands to qllm_attn_prefill for these tensors -- (batch, q_heads, kv_heads, head_dim, q_len, max_len, q batch /
    head / row stride, cache batch / head / position stride, mask_kind, mask_len, mask batch / row stride) -- or QllmUnsupported with the
    reason.  q: [B, Hq, S, D] (any strides: the transposed view of the [B, S, Hq, D] projection output is served in place), S >= 2, fp16 /
    bf16, inner stride 1, 16-byte aligned, strides multiples of 8; caches [B, Hkv, L, D] of that type with contiguous D and the same
    strides, already holding the S new rows; Hkv divides Hq, at most 8 query heads per kv head; D 64 or 128; mask None, [B, 1, S, L'] or
    [B, S, L'] (B or 1 batch rows, expanded views included), bool or of the activation type, inner stride 1; `length` an int (S..L; the mask
    covers it) or a 0-d int64 tensor on the device (the mask then covers L).  Pure host code, any device."""
    def grid(no, b, hq, hkv, s, d):
        if b > 65535 or hq > 65535:
            raise no(f"batch <= 65535 and q_heads <= 65535 (got {b}, {hq})")
    return _attn_rows_plan("attn_prefill", grid, q, k_cache, v_cache, length, mask)


def _attn_rows_plan(name: str, served, q, k_cache, v_cache, length, mask, quant=None):
    """The plan tuple attn_prefill_plan and attn_chunk_plan share, with the refusals under `name`; `served(no, b, hq, hkv, s, d)` raises what
    only that kernel refuses, in the place of the grid's bound.  `quant`: None, or (k_params, v_params, bits) of a quantized cache whose
    codes k_cache / v_cache are -- `_kvq_cache`'s rules on both in the place of the act caches' shape and strides, and the codes' strides
    (bytes) followed by the params' (elements) in the place of the cache strides."""
    no = _attn_refusal(name)
    _attn_one_type_and_device(no, "q and the caches", (q, k_cache, v_cache) if quant is None else (q,), mask)
    if q.dim() != 4 or 0 in q.shape:
        raise no(f"q must be a non-empty [B, Hq, S, D] tensor or view (got {tuple(q.shape)})")
    b, hq, s, d = q.shape
    if s < 2:
        raise no(f"q must hold at least two rows per sequence (got {s}); one token is attn_decode's")
    if q.stride(3) != 1:
        raise no(f"the last dimension of q must have stride 1 (got {q.stride(3)})")
    qs = tuple(q.stride(i) if q.shape[i] > 1 else 0 for i in range(3))
    if any(x % 8 or x < 0 for x in qs) or q.data_ptr() % 16:
        raise no(f"q must be 16-byte aligned with strides that are non-negative multiples of 8 (got {tuple(q.stride())})")
    if quant is None:
        hkv, max_len = _attn_cache_shape(no, k_cache, v_cache, b, d)
    else:
        hkv, max_len, cs, ps = _kvq_cache(no, k_cache, quant[0], quant[2], b, None, d, q.dtype, q.device)
        if _kvq_cache(no, v_cache, quant[1], quant[2], b, hkv, d, q.dtype, q.device) != (hkv, max_len, cs, ps):
            raise no("the K and the V cache must have one shape and layout")
    _attn_served_heads(no, hq, hkv, d)
    served(no, b, hq, hkv, s, d)
    if s > max_len:
        raise no(f"the caches must hold the {s} query rows (got {max_len} positions)")
    cs = _attn_cache_strides(no, k_cache, v_cache) if quant is None else cs + ps
    need = max_len
    if not _attn_length_on_device(no, length, q):
        need = int(length)
        if need < s or need > max_len:
            raise no(f"the length must lie in {s}..{max_len} (got {need})")
    kind, mask_len, mask_batch, mask_row = _lib.ATTN_MASK_NONE, 0, 0, 0
    if mask is not None:
        m3 = mask[:, 0] if mask.dim() == 4 and mask.shape[1] == 1 else mask
        if m3.dim() != 3 or m3.shape[0] not in (1, b) or m3.shape[1] != s or (m3.shape[2] > 1 and m3.stride(2) != 1):
            raise no(f"the mask must be [B, 1, S, L] or [B, S, L] with B = {b} or 1, S = {s} and inner stride 1 (got {tuple(mask.shape)}, strides {tuple(mask.stride())})")
        mask_len, mask_batch, mask_row = m3.shape[2], (m3.stride(0) if m3.shape[0] > 1 else 0), m3.stride(1)
        kind = _attn_mask_kind(no, mask, q, mask_len, need, mask_batch, mask_row)
    return (b, hq, hkv, d, s, max_len) + qs + cs + (kind, mask_len, mask_batch, mask_row)


def attn_prefill_describe(batch: int, q_heads: int, kv_heads: int, head_dim: int, q_len: int, max_len: int) -> str:
    """The launch `attn_prefill` makes for these shapes ("attn_prefill q_tile=128 kv_tile=64 grid=2x32x1 group=4"), or "refused: ...".
    Pure host code: a function of the shapes alone, never of the length."""
    return _describe("qllm_attn_prefill_describe", 256, int(batch), int(q_heads), int(kv_heads), int(head_dim), int(q_len), int(max_len))


def attn_prefill(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, mask: Optional[torch.Tensor] = None, causal: bool = True,
                 scaling: Optional[float] = None, *, out=None, plan=None, window: Optional[int] = None):
    """softmax(scaling * q K^T + mask) V for S >= 2 query rows per sequence over the first `length` positions of the caches [B, Hkv, L, D],
    which already hold the S new rows, as ONE kernel (qllm_attn_prefill, csrc/attn_prefill.hip): flash attention forward on MFMA, fp32
    scores and softmax, one rounding at the store.  q: [B, Hq, S, D], any strides; returns [B, S, Hq, D] (contiguous: the rows o_proj
    takes).  Query row i sits at position length - S + i; causal: key j counts for row i only if j <= length - S + i.  `length`: an int,
    or a 0-d int64 tensor on the device that the kernel reads and clamps to S..L (a captured call then serves every length).  mask:
    [B, 1, S, L'] or [B, S, L'], bool (True = visible) or additive, applied in addition to causality; a row with no visible key gives
    zeros.  scaling: D ** -0.5 when None.  `attn_prefill_plan` says what is served; everything else raises QllmUnsupported before anything
    is launched.  plan: what it returned for these very arguments.  window: None, or an int W >= 1 -- a sliding window on the linear
    cache: row i at position p = length - S + i sees key j only if p - W < j <= p, in addition to length, causality and mask; key tiles
    wholly below the window of a block's first row are never read.  Needs causal=True (QllmUnsupported otherwise).  The plan does not
    depend on the window; None gives the bits of a call without it."""
    window = _attn_window(window, "attn_prefill")
    if window and not causal:
        raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "attn_prefill: a sliding window is served on causal calls only")
    if plan is None:
        plan = attn_prefill_plan(q, k_cache, v_cache, length, mask)
    b, hq, hkv, d, s, max_len = plan[:6]
    out, kv_len, kv_len_dev, scaling = _attn_call("attn_prefill", q, k_cache, v_cache, length, scaling, out, (b, s, hq, d), d)
    with torch.cuda.device(q.device):
        rc = _lib.load().qllm_attn_prefill_window(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(mask), out.data_ptr(), b, hq, hkv, d, s,
                                                  kv_len, kv_len_dev, max_len, window, *plan[6:16], 1 if causal else 0, scaling, _act_dtype(q), _stream_ptr())
    _lib.check(rc)
    return out


ATTN_CHUNK_MAX_ROWS = 128   # kAttnChunkMaxRows of csrc/kernels.hpp: the query rows of one kv head, (Hq / Hkv) * S, that a block holds


def attn_chunk_plan(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, mask: Optional[torch.Tensor] = None):
    """What `attn_chunk` hands to qllm_attn_chunk for these tensors: `attn_prefill_plan`'s tuple under its rules, or QllmUnsupported with
    the reason.  In the place of attn_prefill's bound on the grid: (Hq / Hkv) * S <= 128 rows per kv head, batch * kv_heads <= 4096 (one
    arrival counter each); and, last, a workspace (qllm_attn_chunk_workspace_bytes) within ops.WORKSPACE_BYTES.  Pure host code, any
    device."""
    return _attn_chunk_plan("attn_chunk", q, k_cache, v_cache, length, mask)


def _attn_chunk_plan(name: str, q, k_cache, v_cache, length, mask, quant=None):
    """attn_chunk_plan's rules under `name`, over act caches or (`quant`, `_attn_rows_plan`'s) over a quantized one."""
    def served(no, b, hq, hkv, s, d):
        if hq // hkv * s > ATTN_CHUNK_MAX_ROWS:
            raise no(f"at most {ATTN_CHUNK_MAX_ROWS} query rows per kv head, (Hq / Hkv) * S (got {hq // hkv * s})")
        if b * hkv > ATTN_DECODE_COUNTERS or b > 65535:
            raise no(f"batch * kv_heads <= {ATTN_DECODE_COUNTERS} (got {b * hkv})")
    plan = _attn_rows_plan(name, served, q, k_cache, v_cache, length, mask, quant)
    nbytes = _lib.load().qllm_attn_chunk_workspace_bytes(*plan[:6])
    if nbytes > WORKSPACE_BYTES:
        raise _attn_refusal(name)(f"a workspace of at most {WORKSPACE_BYTES} bytes (these shapes need {nbytes})")
    return plan


def attn_chunk_describe(batch: int, q_heads: int, kv_heads: int, head_dim: int, q_len: int, max_len: int) -> str:
    """The launch `attn_chunk` makes for these shapes ("attn_chunk rows=64 row_tiles=2 kv_tile=64 splits=32 chunk=128 grid=32x8x1"), or
    "refused: ...".  Pure host code: a function of the shapes and the device's CU count, never of the length."""
    return _describe("qllm_attn_chunk_describe", 256, int(batch), int(q_heads), int(kv_heads), int(head_dim), int(q_len), int(max_len))


def attn_chunk(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, mask: Optional[torch.Tensor] = None, causal: bool = True,
               scaling: Optional[float] = None, *, out=None, plan=None):
    """`attn_prefill` without a window -- the same arguments, the same [B, S, Hq, D] output -- for a FEW query rows behind a long cache (the
    verify step of assisted generation, a continuation chunk), as ONE kernel (qllm_attn_chunk, csrc/attn_chunk.hip): a block holds all
    (Hq / Hkv) * S <= 128 query rows of one kv head, so a K / V tile is staged once for the whole group, and the key positions are split
    over about two blocks per compute unit, combined by the last block to arrive in split order (the same bits on every call).  The
    launch follows the shapes alone: with `length` a 0-d int64 tensor on the device a captured call serves every length.
    `attn_chunk_plan` says what is served; everything else raises QllmUnsupported before anything is launched.  plan: what it returned for
    these very arguments.  The workspace is ops.workspace's, one per (device, stream)."""
    if plan is None:
        plan = attn_chunk_plan(q, k_cache, v_cache, length, mask)
    b, hq, hkv, d, s, max_len = plan[:6]
    out, kv_len, kv_len_dev, scaling = _attn_call("attn_chunk", q, k_cache, v_cache, length, scaling, out, (b, s, hq, d), d)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        ws = workspace(q.device, lib.qllm_attn_chunk_workspace_bytes(b, hq, hkv, d, s, max_len))
        rc = lib.qllm_attn_chunk(q.data_ptr(), k_cache.data_ptr(), v_cache.data_ptr(), _ptr(mask), out.data_ptr(), b, hq, hkv, d, s, kv_len, kv_len_dev,
                                 max_len, *plan[6:16], 1 if causal else 0, scaling, _act_dtype(q), ws.data_ptr(), ws.numel(), _stream_ptr())
    _lib.check(rc)
    return out


def attn_chunk_quant_plan(q: torch.Tensor, k_codes: torch.Tensor, k_params: torch.Tensor, v_codes: torch.Tensor, v_params: torch.Tensor, bits: int, length,
                          mask: Optional[torch.Tensor] = None):
    """What `attn_chunk_quant` hands to qllm_attn_chunk_quant -- (batch, q_heads, kv_heads, head_dim, bits, q_len, max_len, q batch / head /
    row stride, codes batch / head / position stride in bytes, params likewise in elements, mask_kind, mask_len, mask batch / row stride)
    -- or QllmUnsupported with the reason: `attn_chunk_plan`'s rules on q, length and mask, `attn_decode_quant_plan`'s on the two caches
    (codes uint8 [B, Hkv, L, D * bits / 8] and params [B, Hkv, L, P] of q's type, K and V of one shape and layout).  Pure host code, any
    device."""
    plan = _attn_chunk_plan("attn_chunk_quant", q, k_codes, v_codes, length, mask, (k_params, v_params, bits))
    return plan[:4] + (bits,) + plan[4:]


def attn_chunk_quant_describe(batch: int, q_heads: int, kv_heads: int, head_dim: int, bits: int, q_len: int, max_len: int) -> str:
    """The launch `attn_chunk_quant` makes ("attn_chunk_quant bits=8 rows=64 row_tiles=2 kv_tile=64 splits=32 chunk=128 grid=32x8x1"), or
    "refused: ...".  Pure host code; the geometry is `attn_chunk_describe`'s for the same shapes."""
    return _describe("qllm_attn_chunk_quant_describe", 256, int(batch), int(q_heads), int(kv_heads), int(head_dim), int(bits), int(q_len), int(max_len))


def attn_chunk_quant(q: torch.Tensor, k_codes: torch.Tensor, k_params: torch.Tensor, v_codes: torch.Tensor, v_params: torch.Tensor, bits: int, length,
                     mask: Optional[torch.Tensor] = None, causal: bool = True, scaling: Optional[float] = None, *, out=None, plan=None):
    """`attn_chunk` over a QUANTIZED cache, read in place and never written, as ONE kernel (qllm_attn_chunk_quant,
    csrc/attn_chunk_quant.hip): codes and params go to registers and are dequantised, by `kv_dequantize`'s arithmetic, on their way into
    LDS -- the bits of `attn_chunk` over what `kv_dequantize` writes, with no dequantised row in memory.  The caller has already put the S
    new rows in with `kv_quantize`, and `length` counts them.  q, length, mask, causal, scaling and the [B, S, Hq, D] result are
    `attn_chunk`'s.  `attn_chunk_quant_plan` says what is served; everything else raises QllmUnsupported before anything is launched."""
    if plan is None:
        plan = attn_chunk_quant_plan(q, k_codes, k_params, v_codes, v_params, bits, length, mask)
    b, hq, hkv, d, bits, s, max_len = plan[:7]
    out, kv_len, kv_len_dev, scaling = _attn_call("attn_chunk_quant", q, k_codes, v_codes, length, scaling, out, (b, s, hq, d), d)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        ws = workspace(q.device, lib.qllm_attn_chunk_workspace_bytes(b, hq, hkv, d, s, max_len))
        rc = lib.qllm_attn_chunk_quant(q.data_ptr(), k_codes.data_ptr(), k_params.data_ptr(), v_codes.data_ptr(), v_params.data_ptr(), _ptr(mask),
                                       out.data_ptr(), b, hq, hkv, d, bits, s, kv_len, kv_len_dev, max_len, *plan[7:], 1 if causal else 0, scaling,
                                       _act_dtype(q), ws.data_ptr(), ws.numel(), _stream_ptr())
    _lib.check(rc)
    return out


def attn_prefill_quant_plan(q: torch.Tensor, k_codes: torch.Tensor, k_params: torch.Tensor, v_codes: torch.Tensor, v_params: torch.Tensor, bits: int, length,
                            mask: Optional[torch.Tensor] = None):
    """What `attn_prefill_quant` hands to qllm_attn_prefill_quant -- `attn_chunk_quant_plan`'s tuple -- or QllmUnsupported with the reason:
    `attn_prefill_plan`'s rules on q, length and mask, `attn_decode_quant_plan`'s on the two caches.  In the place of attn_prefill's bound
    on the grid: batch and kv_heads <= 65535, (Hq / Hkv) * S <= 2^30.  No bound on the rows per kv head, no workspace.  Pure host code,
    any device."""
    def grid(no, b, hq, hkv, s, d):
        if b > 65535 or hkv > 65535 or hq // hkv * s > 1 << 30:
            raise no(f"batch <= 65535, kv_heads <= 65535 and (Hq / Hkv) * S <= 2^30 (got {b}, {hkv}, {hq // hkv * s})")
    plan = _attn_rows_plan("attn_prefill_quant", grid, q, k_codes, v_codes, length, mask, (k_params, v_params, bits))
    return plan[:4] + (bits,) + plan[4:]


def attn_prefill_quant_describe(batch: int, q_heads: int, kv_heads: int, head_dim: int, bits: int, q_len: int, max_len: int) -> str:
    """The launch `attn_prefill_quant` makes ("attn_prefill_quant bits=8 tile=64 grid=4x8x1 group=4": row tiles of 128 packed rows x kv
    heads x batch), or "refused: ...".  Pure host code: a function of the shapes alone, never of the length."""
    return _describe("qllm_attn_prefill_quant_describe", 256, int(batch), int(q_heads), int(kv_heads), int(head_dim), int(bits), int(q_len), int(max_len))


def attn_prefill_quant(q: torch.Tensor, k_codes: torch.Tensor, k_params: torch.Tensor, v_codes: torch.Tensor, v_params: torch.Tensor, bits: int, length,
                       mask: Optional[torch.Tensor] = None, causal: bool = True, scaling: Optional[float] = None, *, out=None, plan=None):
    """`attn_prefill` without a window over a QUANTIZED cache, read in place and never written, as ONE kernel (qllm_attn_prefill_quant,
    csrc/attn_prefill_quant.hip) for any S >= 2: the query rows of a kv head are packed token-major and cut into tiles of 128, so a K / V
    tile of codes, dequantised by `kv_dequantize`'s arithmetic on its way into LDS, serves all heads of a group in a block; no dequantised
    row reaches memory.  The caller has already put the S new rows in with `kv_quantize`, and `length` counts them.  q, length, mask,
    causal, scaling and the [B, S, Hq, D] result are `attn_prefill`'s.  `attn_prefill_quant_plan` says what is served; everything else
    raises QllmUnsupported before anything is launched."""
    if plan is None:
        plan = attn_prefill_quant_plan(q, k_codes, k_params, v_codes, v_params, bits, length, mask)
    b, hq, hkv, d, bits, s, max_len = plan[:7]
    out, kv_len, kv_len_dev, scaling = _attn_call("attn_prefill_quant", q, k_codes, v_codes, length, scaling, out, (b, s, hq, d), d)
    with torch.cuda.device(q.device):
        rc = _lib.load().qllm_attn_prefill_quant(q.data_ptr(), k_codes.data_ptr(), k_params.data_ptr(), v_codes.data_ptr(), v_params.data_ptr(), _ptr(mask),
                                                 out.data_ptr(), b, hq, hkv, d, bits, s, kv_len, kv_len_dev, max_len, *plan[7:], 1 if causal else 0, scaling,
                                                 _act_dtype(q), _stream_ptr())
    _lib.check(rc)
    return out


def dequant(w: QllmWeight, device: torch.device, dtype=torch.float16, transposed: bool = False) -> torch.Tensor:
    """W[K,N] (or [N,K]) bit-identical to the reference's DequantizeLinearBlockWise / unpack()."""
    lib = _lib.load()
    shape = (w.N, w.K) if transposed else (w.K, w.N)
    out = torch.empty(shape, dtype=dtype, device=device)
    dt = DT_F16 if dtype == torch.float16 else DT_BF16
    if dtype not in (torch.float16, torch.bfloat16):
        raise RuntimeError("dequant output must be float16 or bfloat16")
    with torch.cuda.device(device):
        rc = lib.qllm_dequant(C.byref(w), out.data_ptr(), dt, 1 if transposed else 0, _stream_ptr())
    _lib.check(rc)
    return out


def plan_describe(ws_desc: Sequence[QllmWeight], m: int, have_workspace: bool = True) -> str:
    """Which kernel `linear_forward` (one descriptor) / `linear_forward_grouped` (several) would run for m rows."""
    return _describe("qllm_plan_describe", 256, _array(ws_desc), len(ws_desc), int(m), 1 if have_workspace else 0)


def set_knob(name: str, value: int) -> None:
    """Move one of the planner's thresholds (include/qllm_mi355x.h, qllm_set_knob: e.g. QLLM_GEMM3_MIN_M, QLLM_PANEL_GROUP_MIN_M) for
    this process; `plan_describe` reflects it.  Raises for names / values the release library does not accept."""
    _lib.check(_lib.load().qllm_set_knob(name.encode(), int(value)))


def get_knob(name: str) -> Optional[int]:
    """The override set for `name`, or None when the planner uses its measured default."""
    v, is_set = C.c_int32(0), C.c_int32(0)
    _lib.check(_lib.load().qllm_get_knob(name.encode(), C.byref(v), C.byref(is_set)))
    return int(v.value) if is_set.value else None


def reset_knobs() -> None:
    _lib.load().qllm_reset_knobs()


def ort_dequantize4bits(qweight: torch.Tensor, scales: torch.Tensor, qzeros: torch.Tensor, g_idx: Optional[torch.Tensor],
                        block_size: int, in_features: int, out_features: int) -> torch.Tensor:
    """ORT / MatMulNBits blob -> W[N,K] in the scales' dtype (ort_ops.Dequantize4Bits, ort_ops.cc:161-197)."""
    for name, t in (("qweight", qweight), ("scales", scales), ("qzeros", qzeros)):
        _check_input(t, name)
    if qweight.dtype != torch.uint8:
        raise RuntimeError("qweight must be uint8 (ORT blob layout)")
    zf = qzeros.dtype != torch.uint8
    s16 = scales if scales.dtype == torch.float16 else scales.to(torch.float16)
    z = qzeros if (not zf or qzeros.dtype == torch.float16) else qzeros.to(torch.float16)
    gi = None
    if g_idx is not None:
        gi = g_idx.to(device=qweight.device, dtype=torch.int32).contiguous()
    out = torch.empty((out_features, in_features), dtype=torch.float16, device=qweight.device)
    with torch.cuda.device(qweight.device):
        rc = _lib.load().qllm_ort_dequantize4bits(qweight.data_ptr(), s16.data_ptr(), z.data_ptr(), 1 if zf else 0,
                                                  gi.data_ptr() if gi is not None else None, block_size, in_features,
                                                  out_features, out.data_ptr(), _stream_ptr())
    _lib.check(rc)
    return out if scales.dtype == torch.float16 else out.to(scales.dtype)


def _check_perm(perm: torch.Tensor, x2d: torch.Tensor):
    if perm.dtype != torch.int32 or perm.device != x2d.device or perm.numel() != x2d.shape[1] or not perm.is_contiguous():
        raise RuntimeError("perm must be a contiguous int32 tensor of K entries on x's device")


def gather_columns(x2d: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """x2d[:, perm] for a contiguous [M, K] fp16 / bf16 matrix and an int32 device permutation (act-order layers: the
    activation side of the row-sorted weight copy).  The library's LDS-staged gather; shapes it does not take
    (K % 8, K > 28672) fall back to index_select."""
    _check_x(x2d, ())
    _check_perm(perm, x2d)
    out = torch.empty_like(x2d)
    if x2d.shape[0] == 0:
        return out
    with torch.cuda.device(x2d.device):
        rc = _lib.load().qllm_gather_columns(x2d.data_ptr(), perm.data_ptr(), out.data_ptr(), x2d.shape[0], x2d.shape[1],
                                             _act_dtype(x2d), _stream_ptr())
    if rc == _lib.QLLM_ERR_UNSUPPORTED:
        return x2d.index_select(1, perm.long())
    _lib.check(rc)
    return out


def gather_describe(m: int, k: int) -> str:
    """The launch `gather_columns` makes for an [m, k] matrix ("gather rows=2 cpt=4 grid=33 lds=57344", "gather columns chunks=4 parts=2
    rows_per_block=2 grid=32x2 lds=44032"), or "unsupported (...)".  Pure host code: the rule the launcher executes."""
    return _describe("qllm_gather_describe", 256, int(m), int(k))


def unpack_qweight(qweight: torch.Tensor, layout: str, bits: int, in_features: int, out_features: int) -> torch.Tensor:
    _check_input(qweight, "qweight")
    q = torch.empty((in_features, out_features), dtype=torch.int32, device=qweight.device)
    with torch.cuda.device(qweight.device):
        rc = _lib.load().qllm_unpack_qweight(qweight.data_ptr(), LAYOUTS[layout.upper()], bits, in_features,
                                             out_features, q.data_ptr(), _stream_ptr())
    _lib.check(rc)
    return q


def pack_qweight(q_kn: torch.Tensor, layout: str, bits: int) -> torch.Tensor:
    _check_input(q_kn, "q_kn")
    if q_kn.dtype != torch.int32:
        raise RuntimeError("q_kn must be int32")
    k, n = q_kn.shape
    lay = LAYOUTS[layout.upper()]
    shape = (k, n // 8) if lay == LAYOUT_AWQ_GEMM else (k * bits // 32, n)
    out = torch.empty(shape, dtype=torch.int32, device=q_kn.device)
    with torch.cuda.device(q_kn.device):
        rc = _lib.load().qllm_pack_qweight(q_kn.data_ptr(), lay, bits, k, n, out.data_ptr(), _stream_ptr())
    _lib.check(rc)
    return out


_W_DTYPES = {torch.float16: DT_F16, torch.bfloat16: DT_BF16, torch.float32: _lib.DT_F32}


def _check_weight(weight: torch.Tensor):
    """The quantizers' input: a contiguous 2-D fp16 / bf16 / fp32 device tensor -> (N, K, the library's code of its dtype)."""
    _check_input(weight, "weight")
    if weight.dim() != 2 or weight.dtype not in _W_DTYPES:
        raise RuntimeError(f"weight must be a 2-D float16 / bfloat16 / float32 tensor, got {tuple(weight.shape)} {weight.dtype}")
    return weight.shape[0], weight.shape[1], _W_DTYPES[weight.dtype]


def _outputs(spec, out, want, dev, optional=()):
    """A quantizer's output tuple.  spec: ((name, shape, dtype), ..).  out None: the outputs named in `want` are allocated on dev, the
    others are None; else `out` is the caller's tuple, where only the names in `optional` may be None.  Every tensor is checked."""
    if out is None:
        unknown = set(want) - {name for name, _, _ in spec}
        if unknown:
            raise TypeError(f"unknown outputs {sorted(unknown)}")
        out = tuple(torch.empty(shape, dtype=dtype, device=dev) if name in want else None for name, shape, dtype in spec)
    for (name, shape, dtype), t in zip(spec, out):
        if t is None and name in optional:
            continue
        _check_input(t, name)
        if tuple(t.shape) != shape or t.dtype != dtype or t.device != dev:
            raise RuntimeError(f"{name} must be a contiguous {dtype} {shape} tensor on {dev}")
    return tuple(out)


def _ptr(t: Optional[torch.Tensor]):
    return t.data_ptr() if t is not None else None


def hqq_quantize(weight: torch.Tensor, bits: int, group_size: int = 64, iters: int = 20, lp_norm: float = 0.7, beta: float = 10.0,
                 kappa: float = 1.01, debug: bool = False):
    """weight [N, K] (fp16 / bf16 / fp32, on the device) -> the HQQ layer buffers, by the library's fused proximal solver
    (qllm_hqq_quantize, include/qllm_mi355x.h): (qweight i32 [K*bits/32, N], scales f16 [K/g, N], zeros f16 [K/g, N], rounds_run i32 [1]
    on the device).  `debug` appends the solver's own fp32 (s [K/g, N], z [K/g, N], per-round tensor-wide mean errors [iters])."""
    n, k, code = _check_weight(weight)
    lib = _lib.load()
    g = k if group_size == -1 else int(group_size)
    dev = weight.device
    need = lib.qllm_hqq_quantize_workspace_bytes(n, k, g, int(iters))
    groups = n * (k // g) if g > 0 and k % g == 0 else 0
    dbg_at = (need + 255) // 256 * 256
    ws = torch.empty(max(dbg_at + (8 * groups if debug else 0), 16), dtype=torch.uint8, device=dev)
    rows = max(k // max(g, 1), 1)
    spec = (((max(k * bits // 32, 0), n), torch.int32), ((rows, n), torch.float16), ((rows, n), torch.float16), ((1,), torch.int32))
    out = tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in spec)   # qweight, scales, zeros, rounds
    with torch.cuda.device(dev):
        rc = lib.qllm_hqq_quantize(weight.data_ptr(), code, n, k, int(bits), g, int(iters), float(lp_norm), float(beta), float(kappa),
                                   *(t.data_ptr() for t in out), ws.data_ptr(), ws.numel() if debug else need, _stream_ptr())
    _lib.check(rc)
    if not debug:
        return out
    f = ws[dbg_at:dbg_at + 8 * groups].view(torch.float32)
    return out + (f[:groups].view(k // g, n).clone(), f[groups:].view(k // g, n).clone(), ws[256:256 + 4 * int(iters)].view(torch.float32).clone())


def gptq_quantize(weight: torch.Tensor, u: Optional[torch.Tensor], bits: int, group_size: int = 128, sym: bool = False,
                  want_wq: bool = True, out=None, workspace: Optional[torch.Tensor] = None):
    """weight [N, K] (fp16 / bf16 / fp32 on the device, columns in processing order) and u [K, K] fp32, the upper Cholesky factor of
    the inverse Hessian (None: identity = round-to-nearest), through the library's fused GPTQ column solver (qllm_gptq_quantize,
    include/qllm_mi355x.h): (codes i32 [K, N], scales f32 [N, K/g], zeros f32 [N, K/g], wq [N, K] in weight's dtype or None,
    loss f32 [N]).  `out`: that tuple preallocated (wq may be None); `workspace`: a uint8 tensor of at least
    qllm_gptq_quantize_workspace_bytes -- both for callers that capture the call in a graph or own the memory."""
    return _gptq_call("qllm_gptq_quantize", weight, u, (), bits, group_size, sym, want_wq, out, workspace)


def _gptq_call(entry, weight, u, perm_args, bits, group_size, sym, want_wq, out, workspace):
    """gptq_quantize / gptq_quantize_static: the checks, outputs and workspace both share; perm_args goes between u and N."""
    n, k, code = _check_weight(weight)
    lib = _lib.load()
    g = k if group_size == -1 else int(group_size)
    dev = weight.device
    if u is not None:
        _check_input(u, "u")
        if u.dtype != torch.float32 or tuple(u.shape) != (k, k) or u.device != dev:
            raise RuntimeError(f"u must be a float32 [{k}, {k}] tensor on {dev}, got {tuple(u.shape)} {u.dtype} on {u.device}")
    groups = max(k // max(g, 1), 1)
    spec = (("codes", (k, n), torch.int32), ("scales", (n, groups), torch.float32), ("zeros", (n, groups), torch.float32),
            ("wq", (n, k), weight.dtype), ("loss", (n,), torch.float32))
    out = _outputs(spec, out, [name for name, _, _ in spec if want_wq or name != "wq"], dev, optional=("wq", "loss"))
    need = lib.qllm_gptq_quantize_workspace_bytes(n, k)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev) if workspace is None else workspace
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(weight.data_ptr(), code, _ptr(u), *perm_args, n, k, int(bits), g, 1 if sym else 0, *(_ptr(t) for t in out),
                                 ws.data_ptr(), ws.numel(), _stream_ptr())
    _lib.check(rc)
    return out


def gptq_quantize_static(weight: torch.Tensor, u: Optional[torch.Tensor], perm: Optional[torch.Tensor], bits: int, group_size: int = 128,
                         sym: bool = False, want_wq: bool = True, out=None, workspace: Optional[torch.Tensor] = None,
                         check_perm: bool = True):
    """gptq_quantize with static groups (qllm_gptq_quantize_static, include/qllm_mi355x.h): weight [N, K] in the ORIGINAL column order,
    u [K, K] fp32 in processing order (None: round-to-nearest), perm [K] (int32 or int64 on the device; None: identity) with processing
    position j -> original column perm[j].  Every group's scale / zero comes from `weight` itself; the columns are walked in perm's
    order.  Same outputs, `out` and `workspace` as gptq_quantize, but codes and wq are already in the original column order and scales /
    zeros in the original group numbering.  perm is checked on the device to be a permutation of 0..K-1 (ValueError otherwise; this
    reads one flag back, so a caller that captures the call in a graph passes check_perm=False and vouches for it)."""
    perm32 = None
    if perm is not None:
        k = weight.shape[-1]
        if perm.dtype not in (torch.int32, torch.int64) or tuple(perm.shape) != (k,) or perm.device != weight.device:
            raise RuntimeError(f"perm must be an int32 / int64 [{k}] tensor on {weight.device}, got {tuple(perm.shape)} {perm.dtype} on {perm.device}")
        if check_perm:
            p64 = perm.long()
            inside = (p64 >= 0) & (p64 < k)
            seen = torch.zeros(k, dtype=torch.bool, device=perm.device)
            seen[p64.clamp(0, k - 1)] = True
            if not bool((inside.all() & seen.all()).item()):
                raise ValueError(f"perm must be a permutation of 0..{k - 1}")
        perm32 = perm.to(torch.int32).contiguous()
    return _gptq_call("qllm_gptq_quantize_static", weight, u, (_ptr(perm32),), bits, group_size, sym, want_wq, out, workspace)


def _awq_f32(t: Optional[torch.Tensor], name: str, shape, dev):
    if t is None:
        return None
    _check_input(t, name)
    if t.dtype != torch.float32 or tuple(t.shape) != tuple(shape) or t.device != dev:
        raise RuntimeError(f"{name} must be a contiguous float32 {tuple(shape)} tensor on {dev}, got {tuple(t.shape)} {t.dtype} on {t.device}")
    return t.data_ptr()


def awq_quantize(weight: torch.Tensor, bits: int, group_size: int = 128, col_scale: Optional[torch.Tensor] = None,
                 clip: Optional[torch.Tensor] = None, want=("codes", "scales", "zeros", "wq"), out=None):
    """weight [N, K] (fp16 / bf16 / fp32 on the device) through the library's AWQ pseudo-quantizer (qllm_awq_quantize,
    include/qllm_mi355x.h): v = weight * col_scale [K] (None: 1), clamped to +-clip [N, K/g] (None: not), on the asymmetric min/max grid
    of every (row, group) -> (codes i32 [K, N], scales f32 [N, K/g], zeros f32 [N, K/g], wq [N, K] = dequantized / col_scale in
    weight's dtype).  `want` names the outputs to produce, the others come back None (the scale search wants wq alone); `out`: that
    tuple preallocated, None where an output is not wanted."""
    n, k, code = _check_weight(weight)
    g = int(group_size)
    groups = max(k // max(g, 1), 1)
    lib = _lib.load()
    dev = weight.device
    spec = (("codes", (k, n), torch.int32), ("scales", (n, groups), torch.float32), ("zeros", (n, groups), torch.float32),
            ("wq", (n, k), weight.dtype))
    out = _outputs(spec, out, want, dev, optional=[name for name, _, _ in spec])
    s_ptr, c_ptr = _awq_f32(col_scale, "col_scale", (k,), dev), _awq_f32(clip, "clip", (n, groups), dev)
    with torch.cuda.device(dev):
        rc = lib.qllm_awq_quantize(weight.data_ptr(), code, s_ptr, c_ptr, n, k, int(bits), g, *(_ptr(t) for t in out), _stream_ptr())
    _lib.check(rc)
    return out


def awq_clip_search(weight: torch.Tensor, gram: torch.Tensor, bits: int, group_size: int = 128, n_grid: int = 20, max_shrink: float = 0.5,
                    out=None, workspace: Optional[torch.Tensor] = None):
    """weight [N, K] (fp16 / bf16 / fp32 on the device) and gram f32 [K/g, g, g], the per-group Gram matrices X^T X / tokens of the
    layer's input, through the library's clip search (qllm_awq_clip_search, include/qllm_mi355x.h): per (row, group) the clip
    org * (1 - i / n_grid), i < int(max_shrink * n_grid), whose pseudo-quantized weights change the group's output least ->
    (best_max f32 [N, K/g], best_idx i32 [N, K/g], err f32 [N, K/g, 2]: unclipped and chosen).  `out`: that tuple preallocated;
    `workspace`: a uint8 tensor of at least qllm_awq_clip_search_workspace_bytes."""
    n, k, code = _check_weight(weight)
    g = int(group_size)
    groups = max(k // max(g, 1), 1)
    lib = _lib.load()
    dev = weight.device
    g_ptr = _awq_f32(gram, "gram", (groups, g, g), dev)
    if g_ptr is None:
        raise RuntimeError("gram must not be None")
    spec = (("best_max", (n, groups), torch.float32), ("best_idx", (n, groups), torch.int32), ("err", (n, groups, 2), torch.float32))
    out = _outputs(spec, out, [name for name, _, _ in spec], dev)
    need = lib.qllm_awq_clip_search_workspace_bytes(n, k, g)
    ws = workspace if workspace is not None else (torch.empty(need, dtype=torch.uint8, device=dev) if need else None)
    with torch.cuda.device(dev):
        rc = lib.qllm_awq_clip_search(weight.data_ptr(), code, g_ptr, n, k, int(bits), g, int(n_grid), float(max_shrink),
                                      *(t.data_ptr() for t in out), _ptr(ws), ws.numel() if ws is not None else 0, _stream_ptr())
    _lib.check(rc)
    return out


def repack_native(w: QllmWeight, keep):
    """The layer behind descriptor `w` (GPTQ / AWQ GEMM / HQQ buffers, no g_idx) re-laid-out into the library's strip-major native
    layout (include/qllm_mi355x.h, "native layout") on its device: returns (QllmWeight, keepalive) like make_weight.  A pure integer
    permutation (qllm_repack_native); the bias tensor is shared.  Raises QllmUnsupported for shapes the layout cannot hold."""
    lib = _lib.load()
    qweight, scales, qzeros, _g, bias = keep
    dev = qweight.device
    sz = [C.c_size_t(0) for _ in range(3)]
    _lib.check(lib.qllm_native_sizes(C.byref(w), C.byref(sz[0]), C.byref(sz[1]), C.byref(sz[2])))
    nq = torch.empty(sz[0].value // 4, dtype=torch.int32, device=dev)
    ns = torch.empty(sz[1].value // 2, dtype=torch.float16, device=dev)
    f16z = w.layout == LAYOUT_HQQ
    nz = None
    if sz[2].value:
        nz = torch.empty(sz[2].value // 2, dtype=torch.float16, device=dev) if f16z else torch.empty(sz[2].value // 4, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.qllm_repack_native(C.byref(w), nq.data_ptr(), ns.data_ptr(), nz.data_ptr() if nz is not None else None, _stream_ptr())
    _lib.check(rc)
    out = QllmWeight(nq.data_ptr(), ns.data_ptr(), nz.data_ptr() if nz is not None else None, None,
                     bias.data_ptr() if bias is not None else None, w.K, w.N, w.group_size, w.bits,
                     LAYOUT_NATIVE_F16Z if f16z else LAYOUT_NATIVE, w.add_zero_bias)
    return out, (nq, ns, nz, None, bias)


def unpack_native(w: QllmWeight, keep, layout: str):
    """Inverse of repack_native: the reference buffers (qweight, scales, qzeros) of `layout` ("GPTQ", "GEMM" or "HQQ"), bit-exact."""
    lib = _lib.load()
    nq = keep[0]
    dev = nq.device
    lay = LAYOUTS[layout.upper()]
    groups = (w.K + w.group_size - 1) // w.group_size
    qshape = (w.K, w.N // 8) if lay == LAYOUT_AWQ_GEMM else (w.K * w.bits // 32, w.N)
    qweight = torch.empty(qshape, dtype=torch.int32, device=dev)
    scales = torch.empty((groups, w.N), dtype=torch.float16, device=dev)
    qzeros = None
    if keep[2] is not None:
        qzeros = (torch.empty((groups, w.N), dtype=torch.float16, device=dev) if lay == LAYOUT_HQQ
                  else torch.empty((groups, w.N * w.bits // 32), dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        rc = lib.qllm_unpack_native(C.byref(w), lay, qweight.data_ptr(), scales.data_ptr(),
                                    qzeros.data_ptr() if qzeros is not None else None, _stream_ptr())
    _lib.check(rc)
    return qweight, scales, qzeros


__all__ = ["make_weight", "linear_forward", "linear_forward_grouped", "linear_forward_permuted", "linear_forward_bitpanel", "bitpanel_describe", "linear_forward_bitgemm", "bitgemm_describe", "bitgemm_min_m", "linear_forward_bitgroup", "bitgroup_describe", "linear_forward_swiglu", "swiglu_describe", "linear_forward_residual", "linear_forward_swiglu_residual", "residual_describe", "rmsnorm", "linear_forward_rmsnorm", "rmsnorm_describe", "linear_forward_shared", "dequant", "gather_columns", "gather_describe", "unpack_qweight", "pack_qweight",
           "workspace", "QllmUnsupported", "LAYOUTS", "plan_describe", "repack_native", "unpack_native", "hqq_quantize", "gptq_quantize",
           "gptq_quantize_static", "awq_quantize", "awq_clip_search", "attn_chunk_quant", "attn_chunk_quant_plan", "attn_chunk_quant_describe",
           "attn_prefill_quant", "attn_prefill_quant_plan", "attn_prefill_quant_describe", "rope_qknorm", "rope_qknorm_plan", "moe_gate_up", "moe_down", "moe_plan", "moe_describe",
           "moe_route", "moe_prefill_gate_up", "moe_prefill_down", "moe_prefill_plan", "moe_prefill_describe", "moe_prefill_workspace_bytes", "MoeRoute"]
