"""-m gpu: act-order GPTQ layers at 2 / 5 / 6 / 7 / 8 bits decode without a W -- the gathering form of the bit-stream matvec
(csrc/bitgemv_ao.hip, qllm_linear_forward_permuted) on the row-sorted copy of the layer -- against the oracle (the reference's CPU path
with g_idx: DequantizeLinearBlockWise + matmul) within the decode contract of tests/test_bitgemv_gpu.py (1e-2 against the oracle's fp16
path, 2e-3 against float64 of the reference's own W), and bit for bit against the plain kernel on a gathered copy of x."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from conftest import load_golden
from gpu_util import Ref, guarded, randx, synth, to_layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL, TOL64 = 1e-2, 2e-3
AO_FIXTURES = ["gptq_w2_g64_actorder", "gptq_w5_g64_actorder_bias", "gptq_w6_g128_actorder", "gptq_w7_g64_actorder",
               "gptq_w8_g128_actorder_sym"]
SHAPES = {"g128": (128, 1024, 256), "ragged": (32, 1024, 1000)}   # (group, K, N)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _sorted(d, n=None):
    """The row-sorted copy of the act-order layer `d` as the library sees it: (plain descriptor, keepalive, perm); n: keep the first
    n columns only (symmetric layers: no packed zero points to cut)."""
    from qllm_amd import ops
    perm = np.argsort(d["g_idx"], kind="stable")
    q = O.gptq_int_weight(d["qweight"], d["bits"], d["K"])[perm]
    n = d["N"] if n is None else n
    qz = None if d["qzeros"] is None else _dev(d["qzeros"])
    bias = None if d["bias"] is None else _dev(d["bias"][:n])
    w, keep = ops.make_weight("GPTQ", _dev(O.pack_along_rows(q[:, :n], d["bits"])), _dev(d["scales"][:, :n]), qz, None, bias, d["K"], n,
                              d["groupsize"], d["bits"], 0)
    return w, keep, _dev(perm.astype(np.int32))


@functools.lru_cache(maxsize=None)
def _case(bits, shape):
    """(descriptor, keepalive, perm, Ref) of one synthetic act-order layer; computed once and shared."""
    g, K, N = SHAPES[shape]
    packed = (N * bits) % 32 == 0   # packed zero points need whole words per group row; else symmetric with qzeros = None
    n_syn = N if packed else (N + 31) // 32 * 32
    d = synth("GPTQ", bits, g, K, n_syn, "asym" if packed else "sym", True, shape == "g128", seed=K + N + bits)
    ref = Ref(d)
    if not packed:   # synthesised 24 columns wider (the packer wants whole words), served and checked on the first N
        d = dict(d, qzeros=None)
        ref.w, ref.w16, ref.w64, ref.w32 = ref.w[:, :N], ref.w16[:, :N].contiguous(), ref.w64[:, :N].contiguous(), ref.w32[:, :N].contiguous()
    return _sorted(d, N) + (ref,)


def _check(y, ref, x, tag):
    y = y.float().cpu().numpy()
    e16, e64 = O.rel_err(y, ref.y16(x)), O.rel_err(y, ref.y64(x))
    print(f"{tag}: rel_err vs fp16 oracle {e16:.2e}, vs float64 {e64:.2e}")
    assert e16 <= TOL and e64 <= TOL64, tag


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("bits", [2, 5, 6, 7, 8])
def test_permuted_matvec_matches_oracle_and_the_plain_kernel(bits, shape):
    from qllm_amd import ops
    w, _keep, perm, ref = _case(bits, shape)
    K = w.K
    assert ops.plan_describe([w], 1).startswith(f"bitgemv bits={bits} ")
    for m in (1, 2, 3, 8, 16):   # the five row tiles
        x = randx(m, K, seed=m)
        xt = _dev(x)
        y = ops.linear_forward_permuted(w, perm, xt)
        assert y.shape == (m, w.N)
        _check(y, ref, x, (bits, shape, m))
        # no tolerance: the same arithmetic in the same order as the plain kernel on a gathered x; and a repeated call is bit-equal
        assert torch.equal(y, ops.linear_forward(w, ops.gather_columns(xt, perm))), (bits, shape, m)
        assert torch.equal(y, ops.linear_forward_permuted(w, perm, xt)), (bits, shape, m)
    # bf16 activations: converted while they are staged; bf16 result
    xb = _dev(randx(4, K, seed=9)).to(torch.bfloat16)
    yb = ops.linear_forward_permuted(w, perm, xb)
    assert yb.dtype == torch.bfloat16
    assert O.rel_err(yb.float().cpu().numpy(), ref.y64(xb.float().cpu().numpy().astype(np.float16))) <= TOL
    assert torch.equal(yb, ops.linear_forward(w, ops.gather_columns(xb, perm)))


def _raw(w, perm, xt, ws):
    """The C entry points with the caller's workspace (None: NULL -> no K split); perm None: the plain entry."""
    from qllm_amd import _lib
    lib = _lib.load()
    y = torch.empty((xt.shape[0], w.N), dtype=xt.dtype, device=xt.device)
    wp, wn = (ws.data_ptr(), ws.numel()) if ws is not None else (None, 0)
    stream = torch.cuda.current_stream().cuda_stream
    if perm is None:
        rc = lib.qllm_linear_forward(C.byref(w), xt.data_ptr(), y.data_ptr(), xt.shape[0], _lib.DT_F16, wp, wn, stream)
    else:
        rc = lib.qllm_linear_forward_permuted(C.byref(w), perm.data_ptr(), xt.data_ptr(), y.data_ptr(), xt.shape[0], _lib.DT_F16, wp, wn, stream)
    _lib.check(rc)
    return y


@pytest.mark.parametrize("bits", [8, 5])
def test_two_chunks_of_staged_activations_and_the_k_split(bits):
    """K = 4096 at 16 rows: without a workspace one K block of 128 units against an LDS budget of 105 -- the chunk loop runs twice; with
    one, the K range is split over blocks (fp32 slabs + ticket)."""
    from qllm_amd import ops
    d = synth("GPTQ", bits, 64, 4096, 64, "asym", True, False, seed=40 + bits)
    ref = Ref(d)
    w, _keep, perm = _sorted(d)
    x = randx(16, 4096, seed=16)
    xt = _dev(x)
    xg = ops.gather_columns(xt, perm)
    assert "split_k=1" in ops.plan_describe([w], 16, have_workspace=False)
    y0 = _raw(w, perm, xt, None)
    _check(y0, ref, x, (bits, "two chunks"))
    assert torch.equal(y0, _raw(w, None, xg, None)) and torch.equal(y0, _raw(w, perm, xt, None))
    split = int(ops.plan_describe([w], 16).rsplit("split_k=", 1)[1])
    assert 1 < split <= 8, split
    y1 = ops.linear_forward_permuted(w, perm, xt)
    _check(y1, ref, x, (bits, "split-K"))
    assert torch.equal(y1, ops.linear_forward(w, xg)) and torch.equal(y1, ops.linear_forward_permuted(w, perm, xt))


def test_hqq_zero_points_with_a_random_permutation():
    from qllm_amd import ops
    d = synth("HQQ", 8, 64, 1024, 256, "f16", False, False, seed=77)
    ref = Ref(d)
    w, _keep = ops.make_weight("HQQ", _dev(d["qweight"]), _dev(d["scales"]), _dev(d["qzeros"]), None, None, 1024, 256, 64, 8, 0)
    perm = np.random.default_rng(5).permutation(1024).astype(np.int32)
    pt = _dev(perm)
    for m in (1, 16):
        x = randx(m, 1024, seed=30 + m)
        xt = _dev(x)
        y = ops.linear_forward_permuted(w, pt, xt)
        _check(y, ref, np.ascontiguousarray(x[:, perm]), ("HQQ", m))
        assert torch.equal(y, ops.linear_forward(w, ops.gather_columns(xt, pt)))
        assert torch.equal(y, ops.linear_forward_permuted(w, pt, xt))


@pytest.mark.parametrize("m", [1, 16])
def test_guard_bands_on_the_ragged_layer(m):
    """x and y sit between NaN bands: a read outside x poisons the result, a write outside y disturbs a band."""
    from qllm_amd import ops
    w, _keep, perm, ref = _case(8, "ragged")
    x = randx(m, w.K, seed=50 + m)
    _xbuf, xv = guarded(_dev(x))
    ybuf, yv = guarded(torch.zeros((m, w.N), dtype=torch.float16, device=DEV))
    ops.linear_forward_permuted(w, perm, xv, out=yv)
    assert not torch.isnan(yv).any()
    lead = (ybuf.numel() - yv.numel()) // 2
    assert torch.isnan(ybuf[:lead]).all() and torch.isnan(ybuf[lead + yv.numel():]).all()
    _check(yv, ref, x, ("guarded", m))


# ---- the module ---------------------------------------------------------------------------------------------------------------
def _no_dequant(monkeypatch):
    from qllm_amd import ops

    def boom(*a, **k):
        raise AssertionError("ops.dequant was called: a W was materialised")
    monkeypatch.setattr(ops, "dequant", boom)


@pytest.mark.parametrize("name", AO_FIXTURES)
def test_reference_fixture_decodes_on_the_fused_route(name, monkeypatch):
    from qllm_amd import ops
    g = load_golden("actorder_bits/" + name)
    layer = to_layer(g, DEV)
    w64 = torch.from_numpy(g["W_fwd"]).double()
    b64 = torch.from_numpy(g["bias"]).double() if g["bias"] is not None else 0
    real_dequant = ops.dequant
    with monkeypatch.context() as mp:
        _no_dequant(mp)
        for rows, want in ((1, g["y1"]), (16, g["y"][:16])):
            y = layer(_dev(g["x"][:rows])).cpu().numpy()
            e16 = O.rel_err(y, want)
            e64 = O.rel_err(y, (torch.from_numpy(g["x"][:rows]).double() @ w64 + b64).numpy())
            print(f"{name} M={rows}: rel_err vs reference forward {e16:.2e}, vs float64 of its W {e64:.2e}")
            assert e16 <= TOL and e64 <= TOL64
    assert layer._ao is not None and layer._perm is None
    # above 16 rows: the fallback of before, unchanged
    assert O.rel_err(layer(_dev(g["x"])).cpu().numpy(), g["y"]) <= TOL
    # the sorted copy holds the layer's own numbers: row j of its W is row perm[j] of the original's, bit for bit
    ao_w, _k, perm = layer._ao
    w_orig = real_dequant(layer._descriptor(layer.g_idx, 0), torch.device(DEV))
    assert torch.equal(real_dequant(ao_w, torch.device(DEV)), w_orig.index_select(0, perm.long()))
    assert np.array_equal(w_orig.cpu().numpy().view(np.uint16), g["W_fwd"].view(np.uint16))


def test_module_cache_follows_the_buffers_and_stays_out_of_copies(monkeypatch):
    g = load_golden("actorder_bits/gptq_w8_g128_actorder_sym")
    layer = to_layer(g, DEV)
    keys = sorted(layer.state_dict())
    x = _dev(g["x"][:1])
    _no_dequant(monkeypatch)
    y = layer(x)
    first = layer._ao
    assert first is not None and torch.equal(layer(x), y) and layer._ao is first   # built once
    # copies and the state dict see the layer's own buffers only
    dup = copy.deepcopy(layer)
    assert "_ao" not in dup.__dict__ and "_ao_key" not in dup.__dict__
    sd = layer.state_dict()
    assert sorted(sd) == keys
    for k in ("qweight", "qzeros", "scales", "g_idx"):
        assert np.array_equal(sd[k].cpu().numpy(), g[k]) and torch.equal(getattr(dup, k), getattr(layer, k)), k
    assert torch.equal(dup(x), y) and dup._ao is not None and dup._ao is not first
    # an in-place change of qweight: the copy is rebuilt from the new integers
    qw2 = np.ascontiguousarray(np.roll(g["qweight"], 1, axis=1))
    layer.qweight.copy_(_dev(qw2))
    y2 = layer(x).cpu().numpy()
    assert layer._ao is not first
    want = O.forward("GPTQ", g["x"][:1], qw2, g["scales"], g["qzeros"], g["g_idx"], g["bias"], 8, g["groupsize"], g["K"], 0).numpy()
    assert O.rel_err(y2, want) <= TOL


def test_module_takes_the_measured_form_per_row_count(monkeypatch):
    """1-2 rows: the gathering matvec (one launch); 3-16 rows: gather_columns + the plain matvec on the same copy -- the faster form by
    profiles/bitgemv_actorder.md.  Same bits either way, and no W is written."""
    from qllm_amd import ops
    g = load_golden("actorder_bits/gptq_w8_g128_actorder_sym")
    layer = to_layer(g, DEV)
    calls = []
    for fn in ("linear_forward_permuted", "gather_columns", "linear_forward"):
        real = getattr(ops, fn)
        monkeypatch.setattr(ops, fn, lambda *a, _real=real, _fn=fn, **k: (calls.append(_fn), _real(*a, **k))[1])
    _no_dequant(monkeypatch)
    for rows, want in ((1, ["linear_forward_permuted"]), (2, ["linear_forward_permuted"]), (3, ["gather_columns", "linear_forward"]),
                       (16, ["gather_columns", "linear_forward"])):
        x = _dev(g["x"][:rows])
        del calls[:]
        y = layer(x)
        assert calls == want, (rows, calls)
        ao_w, _k, perm = layer._ao
        assert torch.equal(y, ops.linear_forward_permuted(ao_w, perm, x)), rows
    # 2 bits with N > K at one row: the one shape where one launch lost
    wide = type(layer)(2, 64, 64, 128, False, dtype=torch.float16)
    assert not wide._ao_one_launch(1) and wide._ao_one_launch(2) and not wide._ao_one_launch(3)


def test_matvec_switched_off_builds_no_copy():
    """QLLM_BITGEMV = 0: the layer asks before it builds the row-sorted copy, and runs the path of before."""
    from qllm_amd import ops
    g = load_golden("actorder_bits/gptq_w5_g64_actorder_bias")
    layer = to_layer(g, DEV)
    x = _dev(g["x"][:1])
    ops.set_knob("QLLM_BITGEMV", 0)
    try:
        y = layer(x).cpu().numpy()
        assert layer._ao is None and layer._ao_key is None
    finally:
        ops.reset_knobs()
    assert O.rel_err(y, g["y1"]) <= TOL
    assert O.rel_err(layer(x).cpu().numpy(), g["y1"]) <= TOL and layer._ao is not None


def test_four_bit_act_order_keeps_its_native_path():
    g = load_golden("gptq_w4_g128_actorder")
    layer = to_layer(g, DEV)
    y = layer(_dev(g["x"][:1])).cpu().numpy()
    assert O.rel_err(y, g["y1"]) <= TOL
    assert layer._perm is not None and layer._ao is None


def test_sibling_group_over_such_layers_falls_through(monkeypatch):
    from qllm_amd.modeling.q_layers.fused import SiblingGroup
    g = load_golden("actorder_bits/gptq_w8_g128_actorder_sym")
    a, b = to_layer(g, DEV), to_layer(g, DEV)
    x = _dev(g["x"][:1])
    alone = a(x)
    group = SiblingGroup([a, b])
    a._siblings = b._siblings = group
    _no_dequant(monkeypatch)
    assert torch.equal(a(x), alone) and torch.equal(b(x), alone)
    assert group.forward_for(a, x) is None and group.grouped_launches == 0


def test_permuted_forward_in_a_graph():
    """One permuted forward captured on one stream (no parallel branches), replayed twice: bit-equal to eager."""
    from qllm_amd import ops
    w, _keep, perm, _ref = _case(8, "g128")
    xt = _dev(randx(2, w.K, seed=61))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = ops.linear_forward_permuted(w, perm, xt).clone()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.linear_forward_permuted(w, perm, xt)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


# ---- end to end: the quantizer's product ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [8, 2])
def test_quantize_linear_act_order_decodes_fused(bits, monkeypatch):
    from qllm_amd.quantization.gptq import quantize_linear
    gen = torch.Generator().manual_seed(bits)
    lin = torch.nn.Linear(512, 256, bias=False, dtype=torch.float16)
    lin.weight.data = (torch.randn((256, 512), generator=gen) * 0.05).to(torch.float16)
    lin = lin.to(DEV)
    a = torch.randn((512, 1024), generator=gen, dtype=torch.float64)
    a = a * (torch.rand((512, 1), generator=gen, dtype=torch.float64) * 3 + 0.2)             # uneven diagonal: a real permutation
    hessian = (a @ a.T / 1024).float().to(DEV)
    layer = quantize_linear(lin, hessian, bits=bits, group_size=128, act_order=True)
    wq = lin.weight.data                                                                      # [out, in]: the dequantized weights
    assert layer._resolve_act_order()
    x = _dev(randx(1, 512, seed=70 + bits))
    _no_dequant(monkeypatch)
    y = layer(x).cpu().numpy()
    assert layer._ao is not None
    want = (x.double().cpu() @ wq.double().cpu().T).numpy()
    err = O.rel_err(y, want)
    print(f"quantize_linear bits={bits}: rel_err vs x . wq in float64 {err:.2e}")
    assert err <= TOL64
