"""-m gpu: Falcon-shaped layers (N or K an odd multiple of 64, 64-wide groups) through the q_layer modules and their native copies --
gemm3's half-wide last column tile at prefill sizes, the batch-1 kernel at K % 128 == 64 -- against the oracle, fp16 and bf16, every
zero-point kind; the tail tile's column placement bit for bit; determinism and split vs unsplit; no read past the layer's tables; the
release policy; the fused all-reduce gate."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from gpu_util import Ref, guarded, oracle_w, randx, synth, to_layer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-2


def _rows(M):
    """row subset the CPU oracles are evaluated on: the first / a middle / the last rows (every row when M is small)"""
    if M <= 16:
        return np.arange(M)
    mid = M // 2
    return np.unique(np.r_[0:8, mid - 4:mid + 4, M - 8:M])


def _route(layer, M):
    from qllm_amd import ops
    return ops.plan_describe([layer.decode_descriptor()], M)


def _expect_route(plan, K, N, M):
    if M == 1:
        assert plan.startswith("strip1 ") and " g64 " in plan, plan
    elif M >= 300 or (M > 64 and K * N > 1 << 25):
        assert plan.startswith("gemm3 "), plan
        assert ("n_tail=64" in plan) == (N % 128 == 64), plan
    else:
        assert plan.startswith("panel "), plan


CASES = [  # layout, K, N, zero kind, bias, M values
    ("GPTQ", 4544, 4672, "asym", True, (1, 100, 300, 2048)),     # Falcon-7B's fused query_key_value
    ("HQQ", 4544, 4544, "f16", False, (1, 100, 300, 2048)),      # dense (o_proj)
    ("GEMM", 4544, 18176, "asym", False, (1,)),                  # dense_h_to_4h at batch 1 (N % 128 == 0: gemm3 as before above)
    ("GPTQ", 18176, 4544, "sym", True, (1, 100, 300, 2048)),     # dense_4h_to_h
    ("GEMM", 1088, 320, "asym", True, (1, 100, 300, 2048)),
    ("HQQ", 1088, 320, "f16", True, (1, 300)),
    ("GPTQ", 1088, 320, "asym", False, (1, 300)),
    ("HQQ", 1088, 64, "f16", True, (1, 300, 2048)),                # one half-wide tile is the whole layer (multi-query k / v)
]


@pytest.mark.parametrize("layout,K,N,zk,bias,ms", CASES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}" for c in CASES])
def test_falcon_shapes_match_the_oracle(layout, K, N, zk, bias, ms):
    d = synth(layout, 4, 64, K, N, zk, False, bias, seed=K + N)
    layer = to_layer(d, DEV)
    ref = Ref(d)
    for M in ms:
        x = randx(M, K, seed=M)
        xt = torch.from_numpy(x).to(DEV)
        y = layer(xt)
        _expect_route(_route(layer, M), K, N, M)
        rows = _rows(M)
        yr = y[torch.from_numpy(rows).to(DEV)].cpu().numpy()
        want = ref.y16(x[rows])
        assert y.shape == (M, N) and np.isfinite(yr).all()
        assert O.rel_err(yr, want) <= TOL, (M, O.rel_err(yr, want))
        assert O.rel_err(yr, ref.y64(x[rows])) <= 2e-3, M
        yb = layer(xt.to(torch.bfloat16))                # bf16 activations: the native bf16 forms
        assert yb.dtype == torch.bfloat16
        ybr = yb[torch.from_numpy(rows).to(DEV)].float().cpu().numpy()
        assert O.rel_err(ybr, want) <= TOL, (M, "bf16", O.rel_err(ybr, want))
    assert layer.decode_descriptor().layout in (_layouts()), "the module served its native copy"


def _layouts():
    from qllm_amd import _lib
    return (_lib.LAYOUT_NATIVE, _lib.LAYOUT_NATIVE_F16Z)


@pytest.mark.parametrize("layout,zk", [("GPTQ", "asym"), ("HQQ", "f16")])
def test_half_wide_tail_tile_dequantises_bit_exactly(layout, zk):
    """x = the identity: y IS the kernel's W -- every column of the half-wide last tile (4480..4543) must be the oracle's column, bit
    for bit (pins where the tail tile's 64 live columns land and that its dead half never reaches y)."""
    K, N = 1088, 4544
    d = synth(layout, 4, 64, K, N, zk, False, False, seed=7)
    layer = to_layer(d, DEV)
    eye = torch.eye(K, dtype=torch.float16, device=DEV)
    got = layer(eye)
    plan = _route(layer, K)
    assert plan.startswith("gemm3 ") and "n_tail=64" in plan, plan
    want = oracle_w(d)
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want.view(np.uint16))


@pytest.mark.parametrize("K,M,split", [(4544, 2048, "tail_split=4"), (4544, 300, "split_k=2"), (18176, 100, "split_k=4")])
def test_splits_are_deterministic_and_match_the_unsplit_launch(K, M, split):
    from qllm_amd import ops
    N = 4544
    d = synth("GPTQ", 4, 64, K, N, "asym", False, True, seed=K + M)
    layer = to_layer(d, DEV)
    xt = torch.from_numpy(randx(M, K, seed=3)).to(DEV)
    y = layer(xt)
    assert split in _route(layer, M) and "n_tail=64" in _route(layer, M)
    assert torch.equal(y, layer(xt.clone()))                  # fixed-order sum of the partial tiles
    knob = "QLLM_GEMM3_TAIL" if split.startswith("tail") else "QLLM_GEMM2_SPLITK"
    try:
        ops.set_knob(knob, 0)
        plan = _route(layer, M)
        assert "split" not in plan and "n_tail=64" in plan, plan
        y1 = layer(xt)
    finally:
        ops.reset_knobs()
    assert O.rel_err(y.cpu().numpy(), y1.cpu().numpy()) <= 1e-3
    assert torch.isfinite(y).all()
    # the workspace is left clean (counters re-armed): a split call of another shape right after is still right
    x2 = randx(300, K, seed=4)
    y2 = layer(torch.from_numpy(x2).to(DEV))
    ref = Ref(d)
    rows = _rows(300)
    assert O.rel_err(y2[torch.from_numpy(rows).to(DEV)].cpu().numpy(), ref.y16(x2[rows])) <= TOL


@pytest.mark.parametrize("layout,zk,K,N", [("HQQ", "f16", 4544, 4544), ("GPTQ", "asym", 4544, 4672), ("HQQ", "f16", 1088, 320)])
def test_no_read_past_the_native_tables(layout, zk, K, N):
    """The native copy's scales / zero points / bias between bands of NaN in memory: a read past column N (gemm3's dead half tile) or past
    k-step T (the batch-1 kernel's last window) would put a NaN into y."""
    from qllm_amd import ops
    d = synth(layout, 4, 64, K, N, zk, False, True, seed=3 * K + N)
    layer = to_layer(d, DEV)
    w = layer.decode_descriptor()
    assert w.layout in _layouts()
    native_keep = layer._native[1]                           # (qweight, scales, qzeros, None, bias) of the native copy
    nq, ns, nz, _, nb = native_keep
    (_, gs), (_, gb) = guarded(ns, 8192), guarded(nb, 8192)
    gz = guarded(nz, 8192)[1] if nz is not None and nz.dtype == torch.float16 else nz
    gw = ops.QllmWeight(nq.data_ptr(), gs.data_ptr(), gz.data_ptr() if gz is not None else None, None, gb.data_ptr(),
                        w.K, w.N, w.group_size, w.bits, w.layout, w.add_zero_bias)
    ref = Ref(d)
    for M in (1, 300, 2048):
        x = randx(M, K, seed=M + 1)
        y = ops.linear_forward(gw, torch.from_numpy(x).to(DEV))
        assert torch.isfinite(y).all(), M
        rows = _rows(M)
        assert O.rel_err(y[torch.from_numpy(rows).to(DEV)].cpu().numpy(), ref.y16(x[rows])) <= TOL, M
    torch.cuda.synchronize()
    del gs, gb, gz


def test_falcon_layer_stays_released_after_a_prefill_call():
    """release_reference: the prefill call (M = 300) is now served by the native copy, so the layer keeps ONE copy of its integers --
    before, the unsupported route regenerated the reference buffers and set _needs_reference for good."""
    K, N = 4544, 4544
    d = synth("GPTQ", 4, 64, K, N, "asym", False, False, seed=9)
    layer = to_layer(d, DEV)
    layer.release_reference = True
    ref = Ref(d)
    x1 = randx(1, K, seed=1)
    y1 = layer(torch.from_numpy(x1).to(DEV))
    assert layer._released is not None and layer.qweight.numel() == 0
    x = randx(300, K, seed=2)
    y = layer(torch.from_numpy(x).to(DEV))
    assert layer._needs_reference is False
    assert layer._released is not None and layer.qweight.numel() == 0
    rows = _rows(300)
    assert O.rel_err(y[torch.from_numpy(rows).to(DEV)].cpu().numpy(), ref.y16(x[rows])) <= TOL
    assert O.rel_err(y1.cpu().numpy(), ref.y16(x1)) <= TOL


def test_fused_allreduce_refuses_the_layer_and_the_two_step_path_serves_it():
    """qllm_linear_forward_allreduce gates on 128-wide groups: a K = 4544 g64 layer -- which the batch-1 kernel now takes -- is refused
    (UNSUPPORTED), the module's forward_allreduce_into says False, and forward_into (RowParallelQuantLinear's two-step path) is right."""
    from qllm_amd import _lib
    K, N = 4544, 4544
    d = synth("HQQ", 4, 64, K, N, "f16", False, False, seed=11)
    layer = to_layer(d, DEV)
    x = torch.from_numpy(randx(1, K, seed=5)).to(DEV)
    table = torch.zeros(8, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = torch.empty(1, N, dtype=torch.float16, device=DEV)
    lib = _lib.load()

    class OneRankReducer:     # calls the fused entry as a world-of-one reducer would
        def linear_all_reduce(self, w, x2d, o):
            rc = lib.qllm_linear_forward_allreduce(C.byref(w), x2d.data_ptr(), o.data_ptr(), 1, _lib.DT_F16, table.data_ptr(), 0, 1,
                                                   1 << 20, status.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == _lib.QLLM_ERR_UNSUPPORTED, (rc, _lib.last_error())
            return False

    assert _route(layer, 1).startswith("strip1 ")
    assert layer.forward_allreduce_into(x, out, OneRankReducer()) is False
    layer.forward_into(x, out)
    assert O.rel_err(out.cpu().numpy(), Ref(d).y16(x.cpu().numpy())) <= TOL
