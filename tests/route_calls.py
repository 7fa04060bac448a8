"""What the tests that run every row of the route matrix (tests/route_matrix.py) through the C ABI share: the descriptor a row's call
streams, taken from the module; the call itself (qllm_linear_forward, or qllm_linear_forward_grouped for a sibling group); and the
workspace the contract states.  Used by test_route_memory_gpu.py and test_exact_routes_gpu.py."""
import ctypes as C

import torch

import route_matrix as RM

DEV = "cuda:0"
COUNTERS = 16384
POISON_PAST = 64 << 10      # poisoned bytes past workspace B's stated end


def _lib():
    from qllm_amd import _lib as L
    return L, L.load()


def _layer_keys(r):
    return [(RM.SOURCE_LAYOUT[r.kind], r.bits, r.g, r.K, n, r.zk, r.bias, r.act_order, i) for i, n in enumerate(RM.widths(r))]


def _descriptor(r, layer):
    """(descriptor, keepalive) the row's call streams, taken from the module: its native copy or its reference buffers in place"""
    if r.kind in ("NATIVE", "NATIVE_F16Z"):
        w = layer.native_descriptor(0)
        assert w is not None, r.id
        keep = layer._native[1]
    else:
        g = None
        if r.act_order:
            assert layer._resolve_act_order()
            g = layer.g_idx
        w = layer._descriptor(g, 0)
        keep = layer._desc_keep
    assert w.layout == RM.KIND_LAYOUT[r.kind], (r.id, w.layout)
    assert (w.g_idx is not None) == r.act_order
    return w, keep


def _workspace_b(nbytes, stream):
    """exactly `nbytes` at the 256-byte aligned start of a buffer of 0xFF, counter page zeroed by qllm_workspace_init"""
    L, lib = _lib()
    buf = torch.full((nbytes + POISON_PAST,), 0xFF, dtype=torch.uint8, device=DEV)
    assert buf.data_ptr() % 256 == 0
    assert lib.qllm_workspace_init(buf.data_ptr(), nbytes, stream) == 0, L.last_error()
    return buf


def _call(ws_desc, x, outs, ws_ptr, ws_bytes):
    L, lib = _lib()
    from qllm_amd import ops
    dt = L.DT_BF16 if x.dtype == torch.bfloat16 else L.DT_F16
    M = x.shape[0]
    if len(ws_desc) == 1:
        rc = lib.qllm_linear_forward(C.byref(ws_desc[0]), x.data_ptr(), outs[0].data_ptr(), M, dt, ws_ptr, ws_bytes, ops._stream_ptr())
    else:
        arr = (L.QllmWeight * len(ws_desc))(*ws_desc)
        ys = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        rc = lib.qllm_linear_forward_grouped(arr, ys, len(ws_desc), x.data_ptr(), M, dt, ws_ptr, ws_bytes, ops._stream_ptr())
    assert rc == 0, (rc, L.last_error())


def _stated_bytes(r, ws_desc):
    """what the contract tells a caller to provide: qllm_workspace_bytes_act, or the grouped rule"""
    L, lib = _lib()
    from qllm_amd import ops
    if len(ws_desc) > 1:
        return ops.grouped_workspace_bytes(ws_desc, r.M, RM.act_dtype(r), torch.device(DEV))
    return lib.qllm_workspace_bytes_act(C.byref(ws_desc[0]), r.M, RM.act_dtype(r))
