"""torch-facing wrappers over the C ABI: pass data_ptr()s + the current HIP stream, allocate outputs and the
split-K workspace with torch's caching allocator (the library itself never allocates).

PyTorch is plumbing here (device memory, streams); all compute is in libqllm_mi355x.so.
"""
from __future__ import annotations

import ctypes as C
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


def rope(q: torch.Tensor, k: Optional[torch.Tensor], cos: torch.Tensor, sin: torch.Tensor, unsqueeze_dim: int = 1, *, out=None, plan=None):
    """(q * cos + rotate_half(q) * sin, k * cos + rotate_half(k) * sin) with cos / sin unsqueezed at `unsqueeze_dim`: transformers'
    apply_rotary_pos_emb (Llama, Mistral, Qwen2) for both tensors in ONE kernel (qllm_rope, csrc/rope.hip), bit for bit, returning tensors
    of the shape and strides the eager call returns -- for the usual view(B, S, H, D).transpose(1, 2) inputs logical [B, H, S, D] over
    [B, S, H, D] memory.  `rope_plan` says what is served; everything else raises QllmUnsupported before anything is launched.  k may be
    None (q alone: returns (q_out, None)).  out: (q_out, k_out) to write into, each of its input's shape, type and device, laid out as
    the result would be (token-major, dense); an output may be its input when that one is laid out so.  plan: what `rope_plan` returned
    for these very arguments, for a caller that has asked already."""
    rows, hq, hk, d, q_row, q_head, k_row, k_head, cos_rows = plan if plan is not None else rope_plan(q, k, cos, sin, unsqueeze_dim)
    for t in (q, cos, sin) + ((k,) if k is not None else ()):
        if not t.is_cuda:
            raise RuntimeError("rope: q, k, cos and sin must be HIP/CUDA tensors (qllm_amd has no CPU forward path)")
    if out is None:
        q_out, k_out = torch.empty_like(q), torch.empty_like(k) if k is not None else None
        if not all(o is None or _rope_tokens(o, unsqueeze_dim).is_contiguous() for o in (q_out, k_out)):
            raise QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "rope: the eager result of these inputs is not token-major in memory")
    else:
        q_out, k_out = out
        for name, o, t in (("q_out", q_out, q), ("k_out", k_out, k)):
            if (o is None) != (t is None):
                raise RuntimeError(f"rope: {name} must be given exactly when its input is")
            if t is not None and (o.shape != t.shape or o.dtype != t.dtype or o.device != t.device or not _rope_tokens(o, unsqueeze_dim).is_contiguous()):
                raise RuntimeError(f"rope: {name} must be a {tuple(t.shape)} {t.dtype} tensor on {t.device} that is dense and token-major in memory")
    with torch.cuda.device(q.device):
        rc = _lib.load().qllm_rope(q.data_ptr(), _ptr(k), cos.data_ptr(), sin.data_ptr(), q_out.data_ptr(), _ptr(k_out), rows, hq, hk, d,
                                   q_row, q_head, k_row, k_head, cos_rows, _act_dtype(q), _stream_ptr())
    _lib.check(rc)
    return q_out, k_out


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


def attn_prefill_plan(q: torch.Tensor, k_cache: torch.Tensor, v_cache: torch.Tensor, length, mask: Optional[torch.Tensor] = None):
    """What `attn_prefill` hands to qllm_attn_prefill for these tensors -- (batch, q_heads, kv_heads, head_dim, q_len, max_len, q batch /
    head / row stride, cache batch / head / position stride, mask_kind, mask_len, mask batch / row stride) -- or QllmUnsupported with the
    reason.  q: [B, Hq, S, D] (any strides: the transposed view of the [B, S, Hq, D] projection output is served in place), S >= 2, fp16 /
    bf16, inner stride 1, 16-byte aligned, strides multiples of 8; caches [B, Hkv, L, D] of that type with contiguous D and the same
    strides, already holding the S new rows; Hkv divides Hq, at most 8 query heads per kv head; D 64 or 128; mask None, [B, 1, S, L'] or
    [B, S, L'] (B or 1 batch rows, expanded views included), bool or of the activation type, inner stride 1; `length` an int (S..L; the mask
    covers it) or a 0-d int64 tensor on the device (the mask then covers L).  Pure host code, any device."""
    no = _attn_refusal("attn_prefill")
    _attn_one_type_and_device(no, "q and the caches", (q, k_cache, v_cache), mask)
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
    hkv, max_len = _attn_cache_shape(no, k_cache, v_cache, b, d)
    _attn_served_heads(no, hq, hkv, d)
    if b > 65535 or hq > 65535:
        raise no(f"batch <= 65535 and q_heads <= 65535 (got {b}, {hq})")
    if s > max_len:
        raise no(f"the caches must hold the {s} query rows (got {max_len} positions)")
    cs = _attn_cache_strides(no, k_cache, v_cache)
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
           "gptq_quantize_static", "awq_quantize", "awq_clip_search"]
