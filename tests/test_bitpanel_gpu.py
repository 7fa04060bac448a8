"""-m gpu: the fused mid-batch kernel (csrc/bitpanel.hip, qllm_linear_forward_bitpanel) -- 17..512 rows on the GPTQ / HQQ row-stream
layouts in place, 2..8 bits -- against the oracle within the project's contract (tests/test_numerics_contract_gpu.py: 1e-2 of the
reference's fp16 CPU path, 2e-3 of float64 on the reference's own W), bit for bit against itself (determinism, a dirty workspace, a
graph), under guard bands, and through the modules (plain and act-order layers) that used to dequantise and call a dense GEMM here."""
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
ROWS = (17, 32, 33, 64, 65, 128, 129, 200, 512)   # every row-tile count, a ragged last row tile, two and four row blocks, a ragged last one
# name -> (layout, group, K, N, zero kind, bias).  N = 992: N * bits % 32 == 0 for every width, N % 64 == 32; N = 1000: no multiple of 16;
# N = 128: two panels -> split-K
CASES = {"g32_bias": ("GPTQ", 32, 512, 992, "asym", True), "hqq_ragged": ("HQQ", 64, 1024, 1000, "f16", False),
         "sym_split": ("GPTQ", 128, 4096, 128, "sym", False), "plain": ("GPTQ", 128, 1024, 1024, "asym", False)}
# K tails: K / 32 odd (35, 33, 17: the last k-pair of x is half dead), even but no multiple of the 8-unit tile (34), and splits whose
# unit count is no multiple of 8 (35 -> 18 + 17, 100 -> five splits of 20): zero-filled x against live weight units inside a tile
TAILS = {"k1120_split": ("GPTQ", 32, 1120, 128, "asym", False), "k1056": ("GPTQ", 32, 1056, 192, "asym", True),
         "k544": ("GPTQ", 32, 544, 128, "asym", False), "k1088_hqq_split": ("HQQ", 64, 1088, 128, "f16", False),
         "k3200_split": ("GPTQ", 128, 3200, 128, "sym", False)}
CASES.update(TAILS)
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


@functools.lru_cache(maxsize=None)
def _case(bits, name):
    """(descriptor, keepalive, oracle y in fp16 and float64 for the 512 shared rows, Ref) of one synthetic layer; computed once"""
    from qllm_amd import ops
    d = _synth(bits, name)
    layout, g, K, N, zk, _bias = CASES[name]
    ref = Ref(d)
    qz = None if zk == "sym" else _dev(d["qzeros"])   # symmetric: NULL qzeros (the packed zeros synth made are all 2^(bits-1))
    w, keep = ops.make_weight(layout, _dev(d["qweight"]), _dev(d["scales"]), qz, None, None if d["bias"] is None else _dev(d["bias"]),
                              K, N, g, bits, 0)
    x = _x(K)[0]
    return w, keep, ref.y16(x), ref.y64(x), ref


def _check(y, y16, y64, tag):
    y = y.float().cpu().numpy()
    m = y.shape[0]
    e16, e64 = O.rel_err(y, y16[:m]), O.rel_err(y.astype(np.float64), y64[:m])
    print(f"{tag}: rel_err vs fp16 oracle {e16:.2e}, vs float64 {e64:.2e}")
    assert np.isfinite(y).all() and e16 <= TOL and e64 <= TOL64, tag


def _raw(w, xt, ws=None, nbytes=0, out=None):
    """The C entry with the caller's workspace (None: NULL -> no K split)"""
    from qllm_amd import _lib, ops
    y = torch.empty((xt.shape[0], w.N), dtype=xt.dtype, device=xt.device) if out is None else out
    dt = _lib.DT_BF16 if xt.dtype == torch.bfloat16 else _lib.DT_F16
    rc = _lib.load().qllm_linear_forward_bitpanel(C.byref(w), xt.data_ptr(), y.data_ptr(), xt.shape[0], dt,
                                                  None if ws is None else ws.data_ptr(), nbytes, ops._stream_ptr())
    _lib.check(rc)
    return y


def _split(w, m, have_workspace=True):
    from qllm_amd import ops
    return int(ops.bitpanel_describe(w, m, have_workspace).rsplit("split_k=", 1)[1])


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 7, 8])
def test_matches_the_oracle_at_every_row_count(bits, name):
    from qllm_amd import ops
    w, _keep, y16, y64, ref = _case(bits, name)
    xt = _x(w.K)[1]
    if name.endswith("_split"):
        assert _split(w, 64) > 1 and _split(w, 512) > 1 and _split(w, 64, have_workspace=False) == 1
    if name == "k3200_split":
        assert _split(w, 64) == 5   # 100 units: five splits of 20, two and a half tiles each
    for m in ROWS:
        y = ops.linear_forward_bitpanel(w, xt[:m])
        assert y.shape == (m, w.N) and y.dtype == torch.float16
        _check(y, y16, y64, (bits, name, m))
    # the same call without a workspace: no split, the same bounds
    for m in (33, 200):
        _check(_raw(w, xt[:m]), y16, y64, (bits, name, m, "no workspace"))
    # bf16 activations: converted to fp16 while x is staged, bf16 result (the oracle sees the bf16 values as fp16)
    xb = xt[:40].to(torch.bfloat16)
    yb = ops.linear_forward_bitpanel(w, xb)
    assert yb.dtype == torch.bfloat16
    err = O.rel_err(yb.float().cpu().numpy().astype(np.float64), ref.y64(xb.float().cpu().numpy().astype(np.float16)))
    print(f"{(bits, name)} bf16: rel_err vs float64 {err:.2e}")
    assert err <= TOL


# ---- the other ingest ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g32_bias", "hqq_ragged", "sym_split", "k1120_split", "k3200_split"])
@pytest.mark.parametrize("bits", [2, 3, 4, 5, 6, 7, 8])
def test_lds_staged_words_give_the_same_bits(bits, name):
    """QLLM_BITPANEL_LDS = 1: the packed words go through LDS instead of straight into registers.  The fragments, hence every sum, are
    the same: bit-equal to the default ingest, ragged panels, K tails, splits and bf16 included."""
    from qllm_amd import ops
    w, _keep, y16, y64, _ref = _case(bits, name)
    xt = _x(w.K)[1]
    xb = xt[:40].to(torch.bfloat16)
    want = {m: ops.linear_forward_bitpanel(w, xt[:m]) for m in (17, 64, 129, 512)}
    want_b, want_raw = ops.linear_forward_bitpanel(w, xb), _raw(w, xt[:200])
    ops.set_knob("QLLM_BITPANEL_LDS", 1)
    try:
        for m, y in want.items():
            got = ops.linear_forward_bitpanel(w, xt[:m])
            _check(got, y16, y64, (bits, name, m, "LDS ingest"))
            assert torch.equal(got, y), (bits, name, m)
        assert torch.equal(ops.linear_forward_bitpanel(w, xb), want_b) and torch.equal(_raw(w, xt[:200]), want_raw)
    finally:
        ops.reset_knobs()


# ---- determinism, clean workspace ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits,name,m", [(8, "sym_split", 64), (7, "hqq_ragged", 129), (5, "g32_bias", 33)])
def test_repeated_calls_are_bit_equal_and_leave_the_counters_zero(bits, name, m):
    from qllm_amd import ops
    w, _keep, _y16, _y64, _ref = _case(bits, name)
    xt = _x(w.K)[1]
    ws = ops.workspace(torch.device(DEV), 0)
    small = ops.linear_forward(w, xt[:4])   # the bit-stream matvec through the same workspace, before ...
    assert ops.plan_describe([w], 4).startswith("bitgemv ")
    y = ops.linear_forward_bitpanel(w, xt[:m])
    assert torch.equal(y, ops.linear_forward_bitpanel(w, xt[:m]))
    torch.cuda.synchronize()
    assert bool((ws[:COUNTERS] == 0).all())
    assert torch.equal(small, ops.linear_forward(w, xt[:4]))   # ... and right after
    assert torch.equal(y, ops.linear_forward_bitpanel(w, xt[:m]))


# ---- hostile memory (workspace B of tests/test_route_memory_gpu.py) ----------------------------------------------------------------
@pytest.mark.parametrize("bits,name,m", [(5, "g32_bias", 33), (7, "hqq_ragged", 129), (8, "sym_split", 64)])
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
    if name == "sym_split":
        assert _split(gw, m) > 1
    need = lib.qllm_bitpanel_workspace_bytes(C.byref(gw), m)
    clean = torch.zeros(need, dtype=torch.uint8, device=DEV)
    want = _raw(gw, gx, clean, need)
    _check(want, y16, y64, (bits, name, m, "guarded"))
    past = 64 << 10
    dirty = torch.full((need + past,), 0xFF, dtype=torch.uint8, device=DEV)
    assert dirty.data_ptr() % 256 == 0
    assert lib.qllm_workspace_init(dirty.data_ptr(), need, ops._stream_ptr()) == 0
    band = 2048
    for call in ("first call", "second call"):
        ybuf = torch.full((band + m * w.N + band,), SENTINEL, dtype=torch.int16, device=DEV)
        yv = ybuf[band:band + m * w.N].view(torch.float16).view(m, w.N)
        _raw(gw, gx, dirty, need, out=yv)
        torch.cuda.synchronize()
        assert bool((ybuf[:band] == SENTINEL).all()) and bool((ybuf[band + m * w.N:] == SENTINEL).all()), (call, "a store outside y")
        assert not bool((ybuf[band:band + m * w.N] == SENTINEL).any()), (call, "y not fully written")
        assert torch.equal(yv, want), (call, "differs from the clean workspace")
        assert bool((dirty[:COUNTERS] == 0).all()), (call, "counter page left dirty")
        assert bool((dirty[need:] == 0xFF).all()), (call, "a store past the stated workspace size")
    assert bool((clean[:COUNTERS] == 0).all())


# ---- graph -----------------------------------------------------------------------------------------------------------------------
def test_two_calls_in_a_graph_replay_bit_equal():
    from qllm_amd import ops
    wa = _case(8, "sym_split")[0]
    wb = _case(5, "g32_bias")[0]
    xa, xb = _x(wa.K)[1][:64].contiguous(), _x(wb.K)[1][:33].contiguous()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ea, eb = ops.linear_forward_bitpanel(wa, xa).clone(), ops.linear_forward_bitpanel(wb, xb).clone()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ya, yb = ops.linear_forward_bitpanel(wa, xa), ops.linear_forward_bitpanel(wb, xb)
    for _ in range(3):
        ya.zero_()
        yb.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(ya, ea) and torch.equal(yb, eb)


# ---- the modules -----------------------------------------------------------------------------------------------------------------
def _no_dequant(monkeypatch):
    from qllm_amd import ops

    def boom(*a, **k):
        raise AssertionError("ops.dequant was called: a W was materialised")
    monkeypatch.setattr(ops, "dequant", boom)


@pytest.fixture
def routed():
    """The modules send 17..128 rows to the kernel, whatever the library's default cutoff is (QLLM_BITPANEL_MAX_M: a measured line that
    moves with the kernel; 0 = the modules do not use the entry); `routed()` puts that state back after a test has moved a knob."""
    from qllm_amd import ops

    def route():
        ops.reset_knobs()
        ops.set_knob("QLLM_BITPANEL_MAX_M", 128)
    route()
    yield route
    ops.reset_knobs()


@pytest.mark.parametrize("bits", [8, 5])
def test_module_runs_mid_batch_without_a_w(bits, monkeypatch, routed):
    """The test that fails without the feature: 64 rows of a 5- / 8-bit layer used to call ops.dequant."""
    from qllm_amd import ops
    d = _synth(bits, "plain")
    _w, _keep, y16, y64, _ref = _case(bits, "plain")
    layer = to_layer(d, DEV)
    xt = _x(d["K"])[1]
    eager = layer(xt[:64])   # (unpatched)
    with monkeypatch.context() as mp:
        _no_dequant(mp)
        y = layer(xt[:64])
        _check(y, y16, y64, (bits, "module", 64))
        assert torch.equal(y, eager)
        out = torch.empty_like(y)
        assert torch.equal(layer.forward_into(xt[:64], out), y)   # forward_into gets the kernel through forward
        # 16 rows: the matvec, as before
        assert ops.plan_describe([layer._descriptor(None, 0)], 16).startswith("bitgemv ")
        _check(layer(xt[:16]), y16, y64, (bits, "module", 16))
        # switched off: the old path runs -- and asks for W
        ops.set_knob("QLLM_BITPANEL", 0)
        try:
            with pytest.raises(AssertionError, match="ops.dequant was called"):
                layer(xt[:64])
        finally:
            routed()
        # above the module's cutoff: the old path as well
        ops.set_knob("QLLM_BITPANEL_MAX_M", 64)
        try:
            _check(layer(xt[:64]), y16, y64, (bits, "module, cutoff 64", 64))
            with pytest.raises(AssertionError, match="ops.dequant was called"):
                layer(xt[:65])
        finally:
            routed()
    # unpatched and switched off: dequant + GEMM agrees with the fused call
    ops.set_knob("QLLM_BITPANEL", 0)
    try:
        old = layer(xt[:64])
    finally:
        routed()
    assert O.rel_err(eager.float().cpu().numpy(), old.float().cpu().numpy()) <= TOL64


@pytest.mark.parametrize("bits", [8, 5])
def test_act_order_module_gathers_and_runs_the_sorted_copy(bits, monkeypatch, routed):
    from qllm_amd import ops
    from qllm_amd.modeling.q_layers import quant_linear_gptq as Q
    d = _synth(bits, "plain", act_order=True)
    ref = Ref(d)
    a, b = to_layer(d, DEV), to_layer(d, DEV)   # two siblings: the same g_idx, hence ONE interned permutation
    x = randx(40, d["K"], seed=40 + bits)
    xt = _dev(x)
    gathers = []
    real = ops.gather_columns
    monkeypatch.setattr(ops, "gather_columns", lambda *args, **kw: (gathers.append(1), real(*args, **kw))[1])
    _no_dequant(monkeypatch)
    ya = a(xt)
    assert a._resolve_act_order() and a._ao is not None
    _check(ya, ref.y16(x), ref.y64(x), (bits, "act-order module", 40))
    gathered = Q._LAST_GATHER[xt.device][3]
    yb = b(xt)
    assert Q._LAST_GATHER[xt.device][3] is gathered and len(gathers) == 1 and a._ao[2] is b._ao[2]   # the siblings share the gather
    assert torch.equal(ya, yb)
    ao_w, _k, perm = a._ao
    assert torch.equal(ya, ops.linear_forward_bitpanel(ao_w, real(xt, perm)))


# ---- continuity --------------------------------------------------------------------------------------------------------------------
def test_row_17_continues_row_16():
    """The rows a 16-row call (the bit-stream matvec) and a 17-row call (this kernel) share differ by the contract's roundings only:
    the 4e-3 x scale rule of tests/test_numerics_contract_gpu.py."""
    from qllm_amd import ops
    w, _keep, _y16, y64, _ref = _case(6, "plain")
    xt = _x(w.K)[1]
    assert ops.plan_describe([w], 16).startswith("bitgemv ")
    lo = ops.linear_forward(w, xt[:16]).double().cpu().numpy()
    hi = ops.linear_forward_bitpanel(w, xt[:17]).double().cpu().numpy()
    scale = float(np.abs(y64[:1]).max())
    diff = np.abs(lo - hi[:16]).max()
    print(f"rows 0..15 at M = 16 and M = 17: max difference {diff:.3e} (scale {scale:.3f})")
    assert diff <= 4e-3 * max(scale, float(np.abs(hi).max()))
