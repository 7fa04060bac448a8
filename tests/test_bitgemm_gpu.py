"""-m gpu: the fused 2..8-bit prefill kernel (csrc/bitgemm.hip, qllm_linear_forward_bitgemm) -- 129 rows and up on the GPTQ / HQQ
row-stream layouts in place -- against the oracle within the project's contract (1e-2 of the reference's fp16 CPU path, 2e-3 of float64
on the reference's own W), element for element against the oracle's W (identity activations), against the path it replaces, bit for
bit against itself (determinism, a dirty workspace, a graph), under guard bands, and through the modules (plain, HQQ, bf16 and
act-order layers) that used to dequantise and call a dense GEMM here."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from gpu_util import Ref, guarded, randx, synth, to_layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, TOL64 = 1e-2, 2e-3
ROWS = (129, 256, 257, 300, 513)   # the first row count served, one full row tile, a row tile of one row, a ragged one, three row tiles
BITS = [2, 3, 4, 5, 6, 7, 8]
# name -> (layout, group, K, N, zero kind, bias)
CASES = {
    "g32_bias": ("GPTQ", 32, 512, 992, "asym", True),         # two groups per k-tile, 96 live columns in the last column tile
    "hqq_ragged": ("HQQ", 64, 1024, 1000, "f16", False),      # 104 live columns, fp16 zero points
    "sym_split": ("GPTQ", 128, 4096, 128, "sym", False),      # S = 8
    "gK": ("GPTQ", 576, 576, 256, "asym", False),             # 9 k-tiles, one group that is no power of two
    "g96_split": ("GPTQ", 96, 1152, 128, "asym", False),      # groups of 3 units against k-tiles of 2 + a split
    "k1216_split": ("GPTQ", 32, 1216, 128, "asym", False),    # 19 k-tiles: a split of 9 + 10
    "k64": ("GPTQ", 32, 64, 128, "asym", False),              # one k-tile: the pipeline's prologue alone
    "k128": ("GPTQ", 64, 128, 256, "sym", False),             # two k-tiles
    "plain": ("GPTQ", 128, 1024, 1024, "asym", False),        # (the modules' layer)
    "k1056": ("GPTQ", 32, 1056, 192, "asym", True),           # (K % 64 == 32: not served)
}
KERNEL_CASES = [n for n in CASES if n not in ("plain", "k1056")]
SPLITS = {"sym_split": 8, "g96_split": 2, "k1216_split": 2, "hqq_ragged": 2}   # (K = 1024: 16 k-tiles, two blocks of 8)
COUNTERS = 16384
SENTINEL = 0x7E5A   # an fp16 NaN nobody computes


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _synth(bits, name, act_order=False):
    layout, g, K, N, zk, bias = CASES[name]
    d = synth(layout, bits, g, K, N, zk, act_order, bias, seed=K + N + 10 * bits)
    d["scales"] = (d["scales"].astype(np.float32) * (16.0 / 2 ** bits) * (1024 / K) ** 0.5).astype(np.float16)   # outputs of a few units
    return d


@functools.lru_cache(maxsize=None)
def _x(K):
    x = randx(max(ROWS), K, seed=K)
    return x, _dev(x)


def _weight(d, name, with_bias=True):
    from qllm_amd import ops
    layout, g, K, N, zk, _bias = CASES[name]
    qz = None if zk == "sym" else _dev(d["qzeros"])   # symmetric: NULL qzeros (the packed zeros synth made are all 2^(bits-1))
    b = _dev(d["bias"]) if with_bias and d["bias"] is not None else None
    return ops.make_weight(layout, _dev(d["qweight"]), _dev(d["scales"]), qz, None, b, K, N, g, d["bits"], 0)


@functools.lru_cache(maxsize=None)
def _case(bits, name):
    """(descriptor, keepalive, oracle y in fp16 and float64 for the 513 shared rows, Ref) of one synthetic layer; computed once"""
    d = _synth(bits, name)
    ref = Ref(d)
    w, keep = _weight(d, name)
    x = _x(CASES[name][2])[0]
    return w, keep, ref.y16(x), ref.y64(x), ref


def _check(y, y16, y64, tag):
    y = y.float().cpu().numpy()
    m = y.shape[0]
    e16, e64 = O.rel_err(y, y16[:m]), O.rel_err(y.astype(np.float64), y64[:m])
    print(f"{tag}: rel_err vs fp16 oracle {e16:.2e}, vs float64 {e64:.2e}")
    assert np.isfinite(y).all() and e16 <= TOL and e64 <= TOL64, tag


def _raw(w, xt, ws=None, nbytes=0, out=None, bf16_out=False):
    """The C entry with the caller's workspace (None: NULL -> no K split)"""
    from qllm_amd import _lib, ops
    assert xt.dtype == torch.float16
    y = torch.empty((xt.shape[0], w.N), dtype=torch.bfloat16 if bf16_out else torch.float16, device=xt.device) if out is None else out
    rc = _lib.load().qllm_linear_forward_bitgemm(C.byref(w), xt.data_ptr(), y.data_ptr(), xt.shape[0],
                                                 _lib.DT_F16_IN_BF16_OUT if bf16_out else _lib.DT_F16,
                                                 None if ws is None else ws.data_ptr(), nbytes, ops._stream_ptr())
    _lib.check(rc)
    return y


def _split(w, m, have_workspace=True):
    from qllm_amd import ops
    return int(ops.bitgemm_describe(w, m, have_workspace).rsplit("split_k=", 1)[1])


# ---- 1. parity ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KERNEL_CASES)
@pytest.mark.parametrize("bits", BITS)
def test_matches_the_oracle_at_every_row_count(bits, name):
    from qllm_amd import ops
    w, _keep, y16, y64, ref = _case(bits, name)
    xt = _x(w.K)[1]
    for m in ROWS:
        if torch.cuda.get_device_properties(0).multi_processor_count >= 128:   # (the split rule counts the device's CUs)
            assert _split(w, m) == SPLITS.get(name, 1), (name, m, ops.bitgemm_describe(w, m))
        assert _split(w, m, have_workspace=False) == 1
        y = ops.linear_forward_bitgemm(w, xt[:m])
        assert y.shape == (m, w.N) and y.dtype == torch.float16
        _check(y, y16, y64, (bits, name, m))
        _check(_raw(w, xt[:m]), y16, y64, (bits, name, m, "no workspace"))   # no split, the same bounds
    # a bf16 y from an fp16 x (QLLM_F16_IN_BF16_OUT), and a bf16 x through the wrapper (the oracle sees the bf16 values as fp16)
    yb = _raw(w, xt[:300], bf16_out=True)
    err = O.rel_err(yb.float().cpu().numpy().astype(np.float64), y64[:300])
    xb = xt[:300].to(torch.bfloat16)
    yo = ops.linear_forward_bitgemm(w, xb)
    assert yb.dtype == torch.bfloat16 and yo.dtype == torch.bfloat16 and yo.shape == (300, w.N)
    erro = O.rel_err(yo.float().cpu().numpy().astype(np.float64), ref.y64(xb.float().cpu().numpy().astype(np.float16)))
    print(f"{(bits, name)} bf16 y: rel_err vs float64 {err:.2e}; bf16 x: {erro:.2e}")
    assert err <= TOL and erro <= TOL


# ---- 2. identity probe ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32_bias", "hqq_ragged", "g96_split"])
@pytest.mark.parametrize("bits", BITS)
def test_identity_activations_return_the_oracles_w(bits, name):
    """x = I: every sum is one product plus zeros, so y is the B tile the dequant waves wrote -- W, element for element, or some wave
    disagrees with qllm_dequant (and the oracle) in at least one bit."""
    from qllm_amd import ops
    d = _synth(bits, name)
    w, _keep = _weight(d, name, with_bias=False)
    want = _case(bits, name)[4].w
    eye = torch.eye(w.K, dtype=torch.float16, device=DEV)
    if name == "g96_split" and torch.cuda.get_device_properties(0).multi_processor_count >= 128:
        assert _split(w, w.K) == 2
    y = ops.linear_forward_bitgemm(w, eye).cpu().numpy()
    bad = np.argwhere(y != want)
    assert bad.size == 0, (bits, name, len(bad), bad[:4].tolist(), [(float(y[tuple(i)]), float(want[tuple(i)])) for i in bad[:4]])
    assert np.array_equal(ops.dequant(w, torch.device(DEV)).cpu().numpy(), want)
    assert np.array_equal(_raw(w, eye).cpu().numpy(), want)   # and without a split


# ---- 3. against the path it replaces --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32_bias", "hqq_ragged", "sym_split", "k1216_split"])
@pytest.mark.parametrize("bits", BITS)
def test_agrees_with_dequant_plus_gemm_and_with_the_mid_batch_kernel(bits, name):
    from qllm_amd import ops
    w, keep, _y16, _y64, _ref = _case(bits, name)
    xt = _x(w.K)[1]
    wt = ops.dequant(w, torch.device(DEV))
    bias = keep[4]
    for m in (257, 513):
        old = torch.matmul(xt[:m], wt)
        if bias is not None:
            old = old + bias
        err = O.rel_err(ops.linear_forward_bitgemm(w, xt[:m]).float().cpu().numpy(), old.float().cpu().numpy())
        print(f"{(bits, name, m)}: rel_err vs dequant + GEMM {err:.2e}")
        assert err <= TOL64, (bits, name, m)
    ops.set_knob("QLLM_BITPANEL_MAX_M", 512)
    try:
        err = O.rel_err(ops.linear_forward_bitgemm(w, xt[:257]).float().cpu().numpy(), ops.linear_forward_bitpanel(w, xt[:257]).float().cpu().numpy())
    finally:
        ops.reset_knobs()
    print(f"{(bits, name, 257)}: rel_err vs the mid-batch kernel {err:.2e}")
    assert err <= TOL64, (bits, name)


# ---- 4. determinism and hygiene ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,name,m", [(8, "sym_split", 300), (5, "g96_split", 257), (7, "k1216_split", 513)])
def test_repeated_split_calls_are_bit_equal_and_leave_the_counters_zero(bits, name, m):
    from qllm_amd import ops
    w, _keep, _y16, _y64, _ref = _case(bits, name)
    xt = _x(w.K)[1]
    ws = ops.workspace(torch.device(DEV), 0)
    small = ops.linear_forward(w, xt[:4])   # the bit-stream matvec and the mid-batch kernel through the same workspace, before ...
    assert ops.plan_describe([w], 4).startswith("bitgemv ")
    mid = ops.linear_forward_bitpanel(w, xt[:64])
    if torch.cuda.get_device_properties(0).multi_processor_count >= 128:
        assert _split(w, m) > 1
    y = ops.linear_forward_bitgemm(w, xt[:m])
    assert torch.equal(y, ops.linear_forward_bitgemm(w, xt[:m]))
    torch.cuda.synchronize()
    assert bool((ws[:COUNTERS] == 0).all())
    assert torch.equal(small, ops.linear_forward(w, xt[:4])) and torch.equal(mid, ops.linear_forward_bitpanel(w, xt[:64]))   # ... and right after
    assert torch.equal(y, ops.linear_forward_bitgemm(w, xt[:m]))


@pytest.mark.parametrize("bits,name,m", [(5, "g32_bias", 300), (7, "hqq_ragged", 257), (8, "sym_split", 513), (6, "k1216_split", 300)])
def test_guard_bands_and_a_poisoned_workspace(bits, name, m):
    from qllm_amd import _lib, ops
    lib = _lib.load()
    w, keep, y16, y64, _ref = _case(bits, name)
    _qw, sc, qz, _gi, b = keep
    gs = guarded(sc)[1]
    gz = guarded(qz)[1] if qz is not None and qz.dtype == torch.float16 else qz
    gb = guarded(b)[1] if b is not None else None
    gw = ops.QllmWeight(w.qweight, gs.data_ptr(), gz.data_ptr() if gz is not None else None, None, gb.data_ptr() if gb is not None else None,
                        w.K, w.N, w.group_size, w.bits, w.layout, 0)
    gx = guarded(_x(w.K)[1][:m].contiguous())[1]
    need = lib.qllm_bitgemm_workspace_bytes(C.byref(gw), m)
    assert need == COUNTERS + (((m + 255) // 256) * ((w.N + 127) // 128) * _split(gw, m) * 256 * 128 * 4 if _split(gw, m) > 1 else 0)
    clean = torch.zeros(need, dtype=torch.uint8, device=DEV)
    want = _raw(gw, gx, clean, need)
    _check(want, y16, y64, (bits, name, m, "guarded"))
    # the slab region filled with the fp16-NaN sentinel, the counter page zero, 0xFF past the stated size
    past = 64 << 10
    dirty = torch.full((need + past,), 0xFF, dtype=torch.uint8, device=DEV)
    assert dirty.data_ptr() % 256 == 0
    dirty[COUNTERS:need].view(torch.int16).fill_(SENTINEL)
    assert lib.qllm_workspace_init(dirty.data_ptr(), need, ops._stream_ptr()) == 0
    for call in ("first call", "second call"):
        ybuf, yv = guarded(torch.zeros((m, w.N), dtype=torch.float16, device=DEV))
        lead = (ybuf.numel() - m * w.N) // 2
        ybuf[lead:lead + m * w.N].view(torch.int16).fill_(SENTINEL)
        _raw(gw, gx, dirty, need, out=yv)
        torch.cuda.synchronize()
        assert bool(torch.isnan(ybuf[:lead]).all()) and bool(torch.isnan(ybuf[lead + m * w.N:]).all()), (call, "a store outside y")
        assert bool(torch.isfinite(yv).all()), (call, "y not fully written, or a read outside x / scales / bias")
        assert torch.equal(yv, want), (call, "differs from the clean workspace")
        assert bool((dirty[:COUNTERS] == 0).all()), (call, "counter page left dirty")
        assert bool((dirty[need:] == 0xFF).all()), (call, "a store past the stated workspace size")
    assert bool((clean[:COUNTERS] == 0).all())


def test_two_calls_in_a_graph_replay_bit_equal():
    from qllm_amd import ops
    wa = _case(8, "sym_split")[0]
    wb = _case(5, "g32_bias")[0]
    xa, xb = _x(wa.K)[1][:300].contiguous(), _x(wb.K)[1][:257].contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ea, eb = ops.linear_forward_bitgemm(wa, xa).clone(), ops.linear_forward_bitgemm(wb, xb).clone()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ya, yb = ops.linear_forward_bitgemm(wa, xa), ops.linear_forward_bitgemm(wb, xb)
    for _ in range(3):
        ya.zero_()
        yb.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ya, ea) and torch.equal(yb, eb)


# ---- 5. the modules --------------------------------------------------------------------------------------------------------------------
def _no_dequant(monkeypatch):
    from qllm_amd import ops

    def boom(*a, **k):
        raise AssertionError("ops.dequant was called: a W was materialised")
    monkeypatch.setattr(ops, "dequant", boom)


@pytest.fixture
def routed():
    """The modules send 257 rows and up to the kernel, whatever the library's default line is (QLLM_BITGEMM_MIN_M: a measured line that
    moves with the kernel; 0 = the modules do not use the entry); `routed()` puts that state back after a test has moved a knob."""
    from qllm_amd import ops

    def route():
        ops.reset_knobs()
        ops.set_knob("QLLM_BITGEMM_MIN_M", 257)
    route()
    yield route
    ops.reset_knobs()


@pytest.mark.parametrize("bits", [8, 5])
def test_module_runs_prefill_without_a_w(bits, monkeypatch, routed):
    """The test that fails without the feature: 300 rows of a 5- / 8-bit layer used to call ops.dequant."""
    from qllm_amd import ops
    d = _synth(bits, "plain")
    _w, _keep, y16, y64, _ref = _case(bits, "plain")
    layer = to_layer(d, DEV)
    xt = _x(d["K"])[1]
    assert ops.bitgemm_min_m() == 257 and ops.bitpanel_max_m() <= 256
    eager = layer(xt[:300])   # (unpatched)
    with monkeypatch.context() as mp:
        _no_dequant(mp)
        y = layer(xt[:300])
        _check(y, y16, y64, (bits, "module", 300))
        assert torch.equal(y, eager)
        out = torch.empty_like(y)
        assert torch.equal(layer.forward_into(xt[:300], out), y)   # forward_into gets the kernel through forward
        # switched off: the old path runs -- and asks for W
        ops.set_knob("QLLM_BITGEMM", 0)
        try:
            with pytest.raises(AssertionError, match="ops.dequant was called"):
                layer(xt[:300])
        finally:
            routed()
        # below the module's line: the old path as well
        ops.set_knob("QLLM_BITGEMM_MIN_M", 301)
        try:
            with pytest.raises(AssertionError, match="ops.dequant was called"):
                layer(xt[:300])
            _check(layer(xt[:301]), y16, y64, (bits, "module, line 301", 301))
        finally:
            routed()
    # unpatched and switched off: dequant + GEMM agrees with the fused call
    ops.set_knob("QLLM_BITGEMM", 0)
    try:
        old = layer(xt[:300])
    finally:
        routed()
    assert O.rel_err(eager.float().cpu().numpy(), old.float().cpu().numpy()) <= TOL64


def test_default_knobs_change_no_route_up_to_256_rows(monkeypatch):
    """With default knobs nothing at or below 256 rows reaches the entry, whatever its default line is."""
    from qllm_amd import _lib, ops
    ops.reset_knobs()
    assert _lib.BITGEMM_MIN_M_DEFAULT == 0 or _lib.BITGEMM_MIN_M_DEFAULT >= 257
    d = _synth(8, "plain")
    layer = to_layer(d, DEV)
    xt = _x(d["K"])[1]

    def boom(*a, **k):
        raise AssertionError("ops.linear_forward_bitgemm was called")
    monkeypatch.setattr(ops, "linear_forward_bitgemm", boom)
    for m in (129, 256):
        layer(xt[:m])
    ops.set_knob("QLLM_BITPANEL_MAX_M", 64)   # the mid-batch cutoff moved down: the rows above it keep dequant + GEMM
    try:
        layer(xt[:65])
    finally:
        ops.reset_knobs()


def test_hqq_and_bf16_modules_run_prefill_without_a_w(monkeypatch, routed):
    _no_dequant(monkeypatch)
    # HQQ, ragged width, fp16 zero points
    d = _synth(5, "hqq_ragged")
    _w, _keep, y16, y64, _ref = _case(5, "hqq_ragged")
    _check(to_layer(d, DEV)(_x(d["K"])[1][:300]), y16, y64, ("HQQ module", 300))
    # a bf16 layer: x is converted once, y is bf16
    d = _synth(8, "plain")
    d["scales"] = torch.from_numpy(d["scales"]).to(torch.bfloat16).to(torch.float16).numpy()   # (scales a bf16 checkpoint can hold)
    ref = Ref(d)
    layer = to_layer(d, DEV, dtype=torch.bfloat16)
    xb = _x(d["K"])[1][:300].to(torch.bfloat16)
    y = layer(xb)
    assert y.dtype == torch.bfloat16 and y.shape == (300, d["N"])
    err = O.rel_err(y.float().cpu().numpy().astype(np.float64), ref.y64(xb.float().cpu().numpy().astype(np.float16)))
    print(f"bf16 module: rel_err vs float64 {err:.2e}")
    assert err <= TOL


def test_act_order_siblings_gather_once_and_run_the_sorted_copy(monkeypatch, routed):
    from qllm_amd import ops
    from qllm_amd.modeling.q_layers import quant_linear_gptq as Q
    d = _synth(8, "plain", act_order=True)
    ref = Ref(d)
    a, b = to_layer(d, DEV), to_layer(d, DEV)   # two siblings: the same g_idx, hence ONE interned permutation
    x = randx(300, d["K"], seed=308)
    xt = _dev(x)
    gathers = []
    real = ops.gather_columns
    monkeypatch.setattr(ops, "gather_columns", lambda *args, **kw: (gathers.append(1), real(*args, **kw))[1])
    _no_dequant(monkeypatch)
    ya = a(xt)
    assert a._resolve_act_order() and a._ao is not None and a._ao_gemm_refused is None
    _check(ya, ref.y16(x), ref.y64(x), ("act-order module", 300))
    gathered = Q._LAST_GATHER[xt.device][3]
    yb = b(xt)
    assert Q._LAST_GATHER[xt.device][3] is gathered and len(gathers) == 1 and a._ao[2] is b._ao[2]   # the siblings share the gather
    assert torch.equal(ya, yb)
    ao_w, _k, perm = a._ao
    assert torch.equal(ya, ops.linear_forward_bitgemm(ao_w, real(xt, perm)))


def test_a_layer_the_kernel_refuses_falls_back(monkeypatch, routed):
    """K % 64 == 32: the entry refuses, the module dequantises and calls the dense GEMM as before -- and still matches the oracle."""
    from qllm_amd import ops
    d = _synth(8, "k1056")
    ref = Ref(d)
    layer = to_layer(d, DEV)
    x = randx(300, d["K"], seed=1056)
    xt = _dev(x)
    with pytest.raises(ops.QllmUnsupported, match="multiple of 64"):
        ops.linear_forward_bitgemm(layer._descriptor(None, 0), xt)
    _check(layer(xt), ref.y16(x), ref.y64(x), ("K = 1056 module", 300))
    with monkeypatch.context() as mp:
        _no_dequant(mp)
        with pytest.raises(AssertionError, match="ops.dequant was called"):
            layer(xt)
