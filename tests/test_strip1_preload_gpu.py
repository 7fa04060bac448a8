"""-m gpu: the preloading twins of the batch-1 kernel (csrc/strip1_pre.hip, QLLM_STRIP1_PRELOAD = 1) against the untouched kernels
(QLLM_STRIP1_PRELOAD = 0) in the same process: torch.equal on the raw bits, tolerance zero.  Every built twin at the smallest shape that
reaches it (K from the shape table: the exact round and a shifted last window per (waves, round) pair; N = 64 columns, or 257 strips
where the table asks for more blocks than compute units), the three zero-point kinds, fp16 and bf16, bias and add_zero_bias, grouped
launches of unequal widths (surplus blocks; siblings beyond the preloaded problem 0), views at a storage offset, a captured graph.
The two diagnostics twins run under qllm_debug_timeline; the slot they fill also says which kernel filled it (word 6: 1 = a twin), which
is the suite's proof that the knob's default dispatches the twins and 0 the kernels of before."""
import contextlib
import ctypes

import pytest
import torch

from gpu_util import randx, synth, to_layer
from qllm_amd import _lib, ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KNOB = "QLLM_STRIP1_PRELOAD"

# (K, N, extra knob, plan line after "strip1 "): every (waves, round) pair, exact and shifted
FORMS = [(512, 64, None, "nw=4 round=8 grid"), (1024, 64, None, "nw=4 round=8 exact grid"),
         (1152, 64, None, "nw=4 round=16 grid"), (2048, 64, None, "nw=4 round=16 exact grid"),
         (2176, 64, None, "nw=4 round=32 grid"), (4096, 64, None, "nw=4 round=32 exact grid"),
         (2176, 4112, None, "nw=8 round=16 grid"), (4096, 4112, None, "nw=8 round=16 exact grid"),
         (3200, 4112, None, "nw=7 round=16 grid"), (3584, 4112, None, "nw=7 round=16 exact grid"),
         (4224, 64, None, "nw=8 round=24 grid"), (6144, 64, None, "nw=8 round=24 exact grid"),
         (6272, 64, None, "nw=8 round=32 grid"), (8192, 64, None, "nw=8 round=32 exact grid"),
         (6272, 64, "QLLM_S1_T256_NW16", "nw=16 round=16 grid"), (8192, 64, "QLLM_S1_T256_NW16", "nw=16 round=16 exact grid"),
         (8320, 64, None, "nw=16 round=24 grid"), (12288, 64, None, "nw=16 round=24 exact grid"),
         (11008, 64, None, "nw=15 round=24 grid"), (11520, 64, None, "nw=15 round=24 exact grid"),
         (12416, 64, None, "nw=16 round=32 grid"), (16384, 64, None, "nw=16 round=32 exact grid"),
         (16512, 64, None, "nw=16 round=40 grid"), (20480, 64, None, "nw=16 round=40 exact grid"),
         (20608, 64, None, "nw=16 round=48 grid"), (24576, 64, None, "nw=16 round=48 exact grid"),
         (24704, 64, None, "nw=16 round=56 grid"), (28672, 64, None, "nw=16 round=56 exact grid"),
         (28800, 64, None, "nw=16 round=64 grid"), (32768, 64, None, "nw=16 round=64 exact grid")]
ZKS = {"packed": ("GPTQ", "asym"), "f16": ("HQQ", "asym"), "sym": ("GPTQ", "sym")}


@contextlib.contextmanager
def knobs(**kv):
    try:
        for k, v in kv.items():
            ops.set_knob(k, v)
        yield
    finally:
        ops.reset_knobs()


def descriptors(K, widths, zk="packed", bias=False, compat=0, seed=3):
    """(descriptors, what keeps their tensors alive)"""
    layout, zkind = ZKS[zk]
    ws, keep = [], []
    for i, n in enumerate(widths):
        d = synth(layout, 4, 128, K, n, zkind, False, bias, seed=seed + 7 * i)
        layer = to_layer(d, DEV)
        if zk == "sym":
            layer._descriptor(None, 0)
            src = ops.make_weight("GPTQ", layer.qweight, layer.scales, None, None, layer.bias, K, n, 128, 4, compat)
            w, k = ops.repack_native(*src)[0:2]
            keep.append((src, k, layer))
        else:
            w = layer.native_descriptor(compat)
            keep.append(layer)
        ws.append(w)
    return ws, keep


def forward(ws, x, outs=None):
    if len(ws) > 1:
        return ops.linear_forward_grouped(ws, x, outs)
    return [ops.linear_forward(ws[0], x, None if outs is None else outs[0])]


def both(ws, x, plan, extra=None, make_outs=None):
    """The launch with the twins and with the untouched kernels; asserts the plan lines (the form, and which kernel takes it)."""
    extra = {extra: 1} if extra else {}
    with knobs(**extra):
        line = ops.plan_describe(ws, 1)
        assert line.startswith("strip1 " + plan) and "args=" not in line, line   # the default: the twins
        assert ops.get_knob(KNOB) in (None, 1)
        got = forward(ws, x, make_outs() if make_outs else None)
    with knobs(**{KNOB: 0}, **extra):
        line = ops.plan_describe(ws, 1)
        assert " args=kernarg " in line and line.replace(" args=kernarg", "").startswith("strip1 " + plan), line
        want = forward(ws, x, make_outs() if make_outs else None)
    torch.cuda.synchronize()
    return got, want


def same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert torch.equal(g.view(torch.int16), w.view(torch.int16))
        assert g.float().abs().max() > 0   # (not two untouched buffers)


@pytest.mark.parametrize("K,N,extra,plan", FORMS, ids=[p.replace(" grid", "").replace(" ", "_") for _, _, _, p in FORMS])
def test_every_twin(K, N, extra, plan):
    ws, keep = descriptors(K, (N,))
    x = torch.from_numpy(randx(1, K, seed=K)).to(DEV)
    same_bits(*both(ws, x, plan, extra))


@pytest.mark.parametrize("zk,compat", [("packed", 0), ("packed", 1), ("f16", 0), ("sym", 0)])
@pytest.mark.parametrize("act", ["f16", "bf16"])
@pytest.mark.parametrize("bias", [False, True])
def test_zero_kinds_activations_bias(zk, compat, act, bias):
    K = 1152                                    # nw=4 round=16, the last wave's window shifted back
    ws, keep = descriptors(K, (64,), zk, bias, compat)
    x = torch.from_numpy(randx(1, K, seed=11)).to(DEV)
    same_bits(*both(ws, x if act == "f16" else x.to(torch.bfloat16), "nw=4 round=16 grid"))


@pytest.mark.parametrize("zk", ["packed", "f16"])
@pytest.mark.parametrize("widths", [(16, 48, 32), (48, 16, 80), (32, 64)])
def test_grouped_siblings(widths, zk):
    """Unequal widths: the grid is the widest sibling's, surplus blocks leave; siblings 1 and 2 are beyond the preloaded problem 0."""
    K = 1024
    ws, keep = descriptors(K, widths, zk, True, 0)
    x = torch.from_numpy(randx(1, K, seed=5)).to(DEV).to(torch.bfloat16)
    got, want = both(ws, x, "nw=4 round=8 exact grid=strips x %d" % len(widths))
    assert [t.shape[-1] for t in got] == list(widths)
    same_bits(got, want)


def test_views_at_a_storage_offset():
    K, N = 2176, 64
    ws, keep = descriptors(K, (N,))
    base = torch.zeros(K + 24, dtype=torch.float16, device=DEV)
    x = base[24:].view(1, K)
    x.copy_(torch.from_numpy(randx(1, K, seed=2)).to(DEV))
    assert x.storage_offset() == 24
    pool = []

    def make_outs():
        buf = torch.full((N + 40,), 7.0, dtype=torch.float16, device=DEV)
        pool.append(buf)
        return [buf[8:8 + N].view(1, N)]
    got, want = both(ws, x, "nw=4 round=32 grid", make_outs=make_outs)
    assert got[0].storage_offset() == 8
    same_bits(got, want)
    for buf in pool:   # nothing outside the view
        assert torch.all(buf[:8] == 7.0) and torch.all(buf[8 + N:] == 7.0)


def test_captured_graph_replays():
    K, widths = 1024, (16, 48, 32)
    ws, keep = descriptors(K, widths, "packed", True, 1)
    x = torch.from_numpy(randx(1, K, seed=9)).to(DEV)
    with knobs(**{KNOB: 0}):
        want = [t.clone() for t in forward(ws, x)]
    eager = [t.clone() for t in forward(ws, x)]
    torch.cuda.synchronize()
    same_bits(eager, want)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        forward(ws, x)            # (warm-up on the capture's stream)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = forward(ws, x)
    for _ in range(2):
        for o in outs:
            o.zero_()
        graph.replay()
        torch.cuda.synchronize()
        same_bits(outs, want)


@pytest.mark.parametrize("K,N,plan", [(4096, 4112, "nw=8 round=16 exact grid"), (11008, 64, "nw=15 round=24 grid")])
def test_diagnostics_twins_under_the_timeline(K, N, plan):
    """strip1_kernel_pre<8, 16, true, true> and <15, 24, false, true> against the diagnostics forms of strip1_kernel (whose entry stamp
    moved in front of their scalar loads): same bits, and every stamped block's slot is written in order by the kernel the knob names."""
    lib = _lib.load()
    ws, keep = descriptors(K, (N,), "packed", True, 0)
    x = torch.from_numpy(randx(1, K, seed=4)).to(DEV)
    outs, slots = {}, {}
    for pre in (1, 0):
        buf = torch.zeros(24, dtype=torch.int64, device=DEV)
        with knobs(**({} if pre else {KNOB: 0})):
            line = ops.plan_describe(ws, 1)
            assert line.replace(" args=kernarg", "").startswith("strip1 " + plan) and (" args=kernarg " in line) == (not pre), line
            assert lib.qllm_debug_timeline(ctypes.c_void_p(buf.data_ptr()), 1) == 0
            try:
                outs[pre] = forward(ws, x)
                torch.cuda.synchronize()
            finally:
                assert lib.qllm_debug_timeline(None, 0) == 0
        slots[pre] = buf.cpu().view(3, 8)
    same_bits(outs[1], outs[0])
    n_strips = N // 16
    for pre in (1, 0):
        t = slots[pre]
        stamped = {0, n_strips // 2, n_strips - 1}     # the first, the middle and the last block of problem 0 (they may coincide)
        rows = [r for r in range(3) if int(t[r, 0]) != 0]
        assert 0 in rows and len(rows) >= 1 and (len(stamped) < 3 or rows == [0, 1, 2]), (pre, t)
        for r in rows:
            entry, issued, staged, mfma, summed, end = (int(v) for v in t[r, :6])
            assert 0 < entry <= issued <= staged <= mfma <= summed <= end, (pre, r, t[r])
            assert int(t[r, 6]) == pre and int(t[r, 7]) == 0, (pre, r, t[r])   # word 6: the twin says 1, strip1_kernel 0
