"""-m gpu: every row of the route matrix (tests/route_matrix.py) under hostile memory, through the C ABI on torch's current stream.

The layers are built through the modules (synth + to_layer), so the native copies are the production ones.  Each row runs twice:
  A  -- the reference call: a fresh, fully zeroed workspace of at least 64 MB;
  B  -- exactly the bytes the contract states (qllm_workspace_bytes_act; for groups the grouped rule, ops.grouped_workspace_bytes), at
        the start of a larger buffer that is 0xFF (fp32 NaN) everywhere but the counter page qllm_workspace_init zeroes.
x, scales, fp16 zero points and bias sit between bands of NaN (gpu_util.guarded): a read past any of them puts NaN into y.  qweight,
packed zero points and g_idx are integers with no NaN pattern and stay unguarded.  y (all of a group's outputs) sits in one buffer of
sentinel halves with bands on both sides and gaps between layers: every band must be bit-unchanged, y must hold no sentinel.  B must
equal A bit for bit (the same split, no garbage from the dirty slabs), and again on a second call over the still-dirty workspace; the
counter page of both is zero after every call.  A row sample is checked against the oracle."""
import ctypes as C
import zlib
from collections import OrderedDict

import numpy as np
import pytest
import torch

import route_matrix as RM
from gpu_util import Ref, guarded, randx, synth, to_layer
from oracle import ref_cpu as O
from route_calls import COUNTERS, DEV, POISON_PAST, _call, _descriptor, _layer_keys, _lib, _stated_bytes, _workspace_b

pytestmark = pytest.mark.gpu
BAND = 4096                 # bytes of guard band around every input and output
SENTINEL = 0x7E5A           # an fp16 NaN nobody computes: marks y's bytes no kernel wrote
WS_A = 64 << 20

_modules = {}               # layer key -> module (kept for the cross-route sequence)
_refs = OrderedDict()       # layer key -> Ref (a few at a time: the float64 copies are large)
_y_ref = {}                 # row id -> [y] of the reference call (workspace A)


def _synth(key):
    layout, bits, g, K, N, zk, bias, act, i = key
    d = synth(layout, bits, g, K, N, zk, act, bias, seed=zlib.crc32(repr(key).encode()) % 100000)
    d["scales"] = (d["scales"].astype(np.float32) * (16.0 / 2 ** bits) * (1024 / K) ** 0.5).astype(np.float16)
    return d


def _module(key):
    if key not in _modules:
        d = _synth(key)
        _modules[key] = (d, to_layer(d, DEV))
    return _modules[key]


def _ref(key):
    if key not in _refs:
        _refs[key] = Ref(_module(key)[0])
        while len(_refs) > 3:
            _refs.popitem(last=False)
    return _refs[key]


def _guarded_descriptor(w, keep, hold):
    """w with its fp16 tables (scales, fp16 zero points, bias) moved between NaN bands"""
    from qllm_amd import ops
    _qw, sc, qz, _gi, b = keep
    gs = guarded(sc, BAND)[1]
    gz = guarded(qz, BAND)[1] if qz is not None and qz.dtype == torch.float16 else qz
    gb = guarded(b, BAND)[1] if b is not None else None
    hold += [gs, gz, gb]
    return ops.QllmWeight(w.qweight, gs.data_ptr(), gz.data_ptr() if gz is not None else None, w.g_idx,
                          gb.data_ptr() if gb is not None else None, w.K, w.N, w.group_size, w.bits, w.layout, w.add_zero_bias)


class Outputs:
    """All of a call's y in ONE buffer of sentinel halves: a band, y[0], a 16-byte gap, y[1], ..., a band; 16-byte aligned starts"""

    def __init__(self, M, widths, dtype):
        band, gap = BAND // 2, 8
        self.spans, at = [], band
        for n in widths:
            self.spans.append((at, M * n, n))
            at += -(-(M * n) // 8) * 8 + gap
        self.buf = torch.full((at - gap + band,), SENTINEL, dtype=torch.int16, device=DEV)
        self.ys = [self.buf[a:a + c].view(dtype).view(M, n) for a, c, n in self.spans]

    def check(self, what):
        mask = torch.ones_like(self.buf, dtype=torch.bool)
        for a, c, _ in self.spans:
            mask[a:a + c] = False
        outside = self.buf[mask]
        assert bool((outside == SENTINEL).all()), (what, "a store outside y", int((outside != SENTINEL).sum()))
        for i, (a, c, _) in enumerate(self.spans):
            inside = self.buf[a:a + c]
            assert not bool((inside == SENTINEL).any()), (what, f"y[{i}] not fully written", int((inside == SENTINEL).sum()))
            assert bool(torch.isfinite(self.ys[i]).all()), (what, f"y[{i}] not finite")


def _x(r):
    x = randx(r.M, r.K, seed=zlib.crc32(r.id.encode()) % 100000)
    xt = torch.from_numpy(x).to(DEV)
    if r.dtype == "bf16":
        xt = xt.to(torch.bfloat16)
        x = xt.float().cpu().numpy().astype(np.float16)      # the oracle's input: the bf16 values as fp16 (as the route fuzzer)
    return x, xt


def _sample_rows(M, seed):
    if M <= 64:
        return np.arange(M)
    rng = np.random.default_rng(seed)
    rows = [np.arange(16), np.arange(M - 16, M)]
    rows += [np.array([b - 1, b]) for b in range(256, M, 256)]
    rows += [rng.integers(t, min(t + 16, M), size=1) for t in range(0, M, 16)]
    return np.unique(np.concatenate(rows))


def _check_oracle(r, keys, x, ys):
    tol64, tol16 = (1.2e-2, 2e-2) if r.dtype == "bf16" else (2e-3, 1e-2)
    rows = _sample_rows(r.M, seed=len(r.id))
    ri = torch.from_numpy(rows).to(DEV)
    for key, y in zip(keys, ys):
        ref = _ref(key)
        got = y[ri].float().cpu().numpy()
        assert O.rel_err(got.astype(np.float64), ref.y64(x[rows])) <= tol64, (r.id, key)
        assert O.rel_err(got, ref.y16(x[rows])) <= tol16, (r.id, key)


def _counters_clean(buf, what):
    assert bool((buf[:COUNTERS] == 0).all()), (what, "counter page left dirty")


def _run_row(r):
    from qllm_amd import ops
    keys = _layer_keys(r)
    descs, hold = [], []
    for key in keys:
        w, keep = _descriptor(r, _module(key)[1])
        descs.append(_guarded_descriptor(w, keep, hold))
    try:
        for k, v in r.knobs.items():
            ops.set_knob(k, v)
        assert ops.plan_describe(descs, r.M) == r.plan, r.id
        x, xt = _x(r)
        gx = guarded(xt, BAND)[1]
        stream = ops._stream_ptr()

        need = _stated_bytes(r, descs)
        ws_a = torch.zeros(max(WS_A, need), dtype=torch.uint8, device=DEV)
        out_a = Outputs(r.M, RM.widths(r), xt.dtype)
        _call(descs, gx, out_a.ys, ws_a.data_ptr(), ws_a.numel())
        torch.cuda.synchronize()
        out_a.check("workspace A")
        _counters_clean(ws_a, "workspace A")

        ws_b = _workspace_b(need, stream)
        for call in ("workspace B", "workspace B, second call"):
            out_b = Outputs(r.M, RM.widths(r), xt.dtype)
            _call(descs, gx, out_b.ys, ws_b.data_ptr(), need)
            torch.cuda.synchronize()
            out_b.check(call)
            _counters_clean(ws_b, call)
            assert bool((ws_b[need:] == 0xFF).all()), (call, "a store past the stated workspace size")
            for i, (ya, yb) in enumerate(zip(out_a.ys, out_b.ys)):
                assert torch.equal(ya.view(torch.int16), yb.view(torch.int16)), (r.id, call, i, "differs from workspace A")
    finally:
        ops.reset_knobs()
    _y_ref[r.id] = [y.clone() for y in out_a.ys]
    _check_oracle(r, keys, x, out_a.ys)


@pytest.mark.parametrize("r", RM.ROWS, ids=[r.id for r in RM.ROWS])
def test_route_under_guard_bands_and_a_poisoned_workspace(r):
    _run_row(r)


def test_cross_route_sequence_through_one_dirty_workspace():
    """All rows back to back through ONE poisoned workspace sized for the largest row, in matrix order and then reversed: every y must
    equal that row's own reference y bit for bit (counters re-armed by every route, no slab leaking from one route into the next)."""
    from qllm_amd import ops
    for r in RM.ROWS:
        if r.id not in _y_ref:
            _run_row(r)
    plain = {}
    for r in RM.ROWS:
        ws_desc = [_descriptor(r, _module(key)[1])[0] for key in _layer_keys(r)]
        plain[r.id] = (ws_desc, _x(r)[1])
    need = max(_stated_bytes(r, plain[r.id][0]) for r in RM.ROWS)
    ws = _workspace_b(need, ops._stream_ptr())
    for order in (RM.ROWS, RM.ROWS[::-1]):
        for r in order:
            ws_desc, xt = plain[r.id]
            outs = [torch.empty(r.M, n, dtype=xt.dtype, device=DEV) for n in RM.widths(r)]
            try:
                for k, v in r.knobs.items():
                    ops.set_knob(k, v)
                _call(ws_desc, xt, outs, ws.data_ptr(), need)
            finally:
                ops.reset_knobs()
            for i, (y, want) in enumerate(zip(outs, _y_ref[r.id])):
                assert torch.equal(y.view(torch.int16), want.view(torch.int16)), (r.id, i)
    torch.cuda.synchronize()
    _counters_clean(ws, "cross-route sequence")
    assert bool((ws[need:] == 0xFF).all())


def test_module_bf16_prefill_beyond_the_persistent_workspace():
    """A bf16 prefill call whose stated workspace exceeds ops' persistent 64 MB takes ops.workspace's `big` branch: torch.empty with only
    the counter page zeroed -- its slabs hold whatever the allocator's memory held.  Through the module, against the oracle."""
    from qllm_amd import _lib as L
    from qllm_amd import ops
    K, N, M = 4096, 256, 8200
    d = synth("GPTQ", 4, 128, K, N, "asym", False, True, seed=77)
    layer = to_layer(d, DEV)
    w = layer.decode_descriptor(None, 0)
    assert L.load().qllm_workspace_bytes_act(C.byref(w), M, L.DT_BF16) > ops.WORKSPACE_BYTES
    assert "split_k=" in ops.plan_describe([w], M), ops.plan_describe([w], M)
    torch.empty(256 << 20, dtype=torch.uint8, device=DEV).fill_(0xFF)   # (the allocator's next blocks: previously NaN bytes)
    x = randx(M, K, seed=78)
    xt = torch.from_numpy(x).to(DEV).to(torch.bfloat16)
    y = layer(xt)
    assert y.dtype == torch.bfloat16 and bool(torch.isfinite(y).all())
    rows = _sample_rows(M, seed=5)
    xin = xt[torch.from_numpy(rows).to(DEV)].float().cpu().numpy().astype(np.float16)
    got = y[torch.from_numpy(rows).to(DEV)].float().cpu().numpy()
    ref = Ref(d)
    assert O.rel_err(got.astype(np.float64), ref.y64(xin)) <= 1.2e-2
    assert O.rel_err(got, ref.y16(xin)) <= 2e-2
