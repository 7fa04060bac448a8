"""-m gpu: the grouped bit-stream matvec (qllm_linear_forward_bitgroup, csrc/bitgemv_group.hip) -- 2 / 5 / 6 / 7 / 8-bit layers that share
x, at decode sizes, in one launch.  The contract is bit-identity with the members' own launches (every member keeps its split, its
chunking and its slab / counter range); on top of it the constants of tests/test_bitgemv_gpu.py against the oracle.

Shapes are tiny on purpose: A has ragged last column blocks and members of 3 / 2 / 2 column blocks without a split (K / 32 = 16 units
are one per lane slot); B splits every member 8 ways (K / 512 bounds it) with 4 / 2 / 1 column blocks; C is symmetric, two equal members."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_util import Ref, randx, synth, to_layer
from oracle import ref_cpu as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITS = (2, 5, 6, 7, 8)
TOL16, TOL64 = 1e-2, 2e-3      # tests/test_bitgemv_gpu.py: against Ref.y16 / Ref.y64
# bf16 results: the same file's bound for them.  y is rounded to 8 significant bits -- 2 ** -9 of the largest element alone is 2e-3 (measured
# here: 1.9e-3 .. 2.6e-3 against Ref.y64 in every bf16 case, 3e-4 .. 9e-4 in the fp16 ones)
TOL_BF16 = 1e-2
COUNTERS = 16384
SENTINEL = 0x7E5A              # an fp16 NaN nobody computes
GUARD = 64 << 10

#        layout  zero kind  g    K     widths          member with a bias
CASES = {"A": ("HQQ", "f16", 64, 512, (96, 40, 34), 1),
         "B": ("GPTQ", "asym", 128, 4096, (128, 64, 32), 0),
         "C": ("GPTQ", "sym", 32, 1024, (64, 64), None)}
_built = {}


def _case(name, bits):
    """(descriptors, keepalive, [Ref]) of a case, built and evaluated once"""
    from qllm_amd import ops
    if (name, bits) not in _built:
        layout, zk, g, K, widths, biased = CASES[name]
        descs, keep, refs = [], [], []
        for i, n in enumerate(widths):
            d = synth(layout, bits, g, K, n, zk, False, i == biased, seed=1000 * bits + 10 * i + ord(name))
            refs.append(Ref(d))
            if zk == "sym":
                qw, sc = torch.from_numpy(d["qweight"]).to(DEV), torch.from_numpy(d["scales"]).to(DEV)
                w, k = ops.make_weight("GPTQ", qw, sc, None, None, None, K, n, g, bits, 0)
                keep.append(k)
            else:
                layer = to_layer(d, DEV)
                w = layer.decode_descriptor()
                keep.append(layer)
            descs.append(w)
        _built[(name, bits)] = (descs, keep, refs)
    return _built[(name, bits)]


def _x(m, K, bf16, seed):
    """(the oracle's input, the device tensor)"""
    x = randx(m, K, seed=seed)
    xt = torch.from_numpy(x).to(DEV)
    if bf16:
        xt = xt.to(torch.bfloat16)
        x = xt.float().cpu().numpy().astype(np.float16)
    return x, xt


def _splits(text):
    assert text.startswith("bitgroup "), text
    return [int(v) for v in text.rsplit("split_k=", 1)[1].split(",")]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_group_equals_the_member_launches_and_the_oracle(name, bits):
    from qllm_amd import ops
    descs, _keep, refs = _case(name, bits)
    K = descs[0].K
    splits = _splits(ops.bitgroup_describe(descs, 1))
    if name == "B":
        assert all(1 < s <= K // 512 for s in splits), splits     # every member of B splits
    if name == "A":
        assert splits == [1, 1, 1], splits
    for m, bf16 in ((1, False), (3, False), (16, False), (2, True), (8, True)):
        assert _splits(ops.bitgroup_describe(descs, m)) == [int(ops.plan_describe([w], m).rsplit("split_k=", 1)[1]) for w in descs]
        x, xt = _x(m, K, bf16, seed=m + bits)
        outs = ops.linear_forward_bitgroup(descs, xt)
        for i, (w, y, ref) in enumerate(zip(descs, outs, refs)):
            assert y.shape == (m, w.N) and y.dtype == xt.dtype
            assert torch.equal(y, ops.linear_forward(w, xt)), (name, bits, m, i)
            got = y.float().cpu().numpy()
            e16, e64 = O.rel_err(got, ref.y16(x)), O.rel_err(got.astype(np.float64), ref.y64(x))
            print(f"case {name} bits={bits} m={m} bf16={bf16} member {i}: rel_err y16 {e16:.2e} y64 {e64:.2e}")
            if bf16:
                assert e64 <= TOL_BF16 and e16 <= TOL_BF16, (name, bits, m, i, e16, e64)
            else:
                assert e16 <= TOL16 and e64 <= TOL64, (name, bits, m, i, e16, e64)


class Outputs:
    """All of a call's y in ONE buffer of sentinel halves: a band, y[0], a 16-byte gap, y[1], ..., a band (tests/test_route_memory_gpu.py)"""

    def __init__(self, M, widths, dtype=torch.float16):
        band, gap = 2048, 8
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
        assert bool((self.buf[mask] == SENTINEL).all()), (what, "a store outside y")
        for i, (a, c, _) in enumerate(self.spans):
            assert not bool((self.buf[a:a + c] == SENTINEL).any()), (what, f"y[{i}] not fully written")


def _raw(descs, xt, outs, ws_ptr, ws_bytes):
    from qllm_amd import _lib as L
    from qllm_amd import ops
    arr = (L.QllmWeight * len(descs))(*descs)
    ys = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
    dt = L.DT_BF16 if xt.dtype == torch.bfloat16 else L.DT_F16
    rc = L.load().qllm_linear_forward_bitgroup(arr, ys, len(descs), xt.data_ptr(), xt.shape[0], dt, ws_ptr, ws_bytes, ops._stream_ptr())
    assert rc == 0, (rc, L.last_error())


def _need(descs, m):
    from qllm_amd import _lib as L
    return L.load().qllm_bitgroup_workspace_bytes((L.QllmWeight * len(descs))(*descs), len(descs), m)


@pytest.mark.parametrize("bits", BITS)
def test_raw_call_stays_inside_its_outputs_and_its_declared_workspace(bits):
    """Case B (every member splits) through the C ABI: outputs between sentinel bands, a workspace of exactly the declared size whose slabs
    are poison, a guard region behind it."""
    from qllm_amd import _lib as L
    from qllm_amd import ops
    descs, _keep, _refs = _case("B", bits)
    m = 3
    widths = [w.N for w in descs]
    _x_np, xt = _x(m, descs[0].K, False, seed=33)
    need = _need(descs, m)
    splits = _splits(ops.bitgroup_describe(descs, m))
    assert all(s > 1 for s in splits) and need == COUNTERS + sum(s * m * n * 4 for s, n in zip(splits, widths))
    want = [ops.linear_forward(w, xt) for w in descs]
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    assert L.load().qllm_workspace_init(ws.data_ptr(), need, ops._stream_ptr()) == 0, L.last_error()
    for call in ("first call", "second call"):
        out = Outputs(m, widths)
        _raw(descs, xt, out.ys, ws.data_ptr(), need)
        torch.cuda.synchronize()
        out.check(call)
        assert bool((ws[:COUNTERS] == 0).all()), (call, "counter page left dirty")
        assert bool((ws[need:] == 0xFF).all()), (call, "a store past the declared workspace")
        for i, (y, w_) in enumerate(zip(out.ys, want)):
            assert torch.equal(y, w_), (bits, call, i)


@pytest.mark.parametrize("bits", (2, 7, 8))
def test_without_a_usable_workspace_no_member_splits(bits):
    """Workspace NULL, and one byte short of the declared size: served; both equal qllm_linear_forward called with a NULL workspace."""
    from qllm_amd import _lib as L
    from qllm_amd import ops
    descs, _keep, refs = _case("B", bits)
    m = 2
    x, xt = _x(m, descs[0].K, False, seed=44)
    widths = [w.N for w in descs]
    plain = []
    for w in descs:
        y = torch.empty((m, w.N), dtype=torch.float16, device=DEV)
        rc = L.load().qllm_linear_forward(C.byref(w), xt.data_ptr(), y.data_ptr(), m, L.DT_F16, None, 0, ops._stream_ptr())
        assert rc == 0, L.last_error()
        plain.append(y)
    null = Outputs(m, widths)
    _raw(descs, xt, null.ys, None, 0)
    need = _need(descs, m)
    ws = torch.full((need + GUARD,), 0xFF, dtype=torch.uint8, device=DEV)
    ws[:COUNTERS].zero_()
    short = Outputs(m, widths)
    _raw(descs, xt, short.ys, ws.data_ptr(), need - 1)
    torch.cuda.synchronize()
    null.check("NULL workspace")
    short.check("short workspace")
    assert bool((ws[COUNTERS:] == 0xFF).all()) and bool((ws[:COUNTERS] == 0).all())   # nothing of it was used
    for i in range(len(descs)):
        assert torch.equal(null.ys[i], plain[i]) and torch.equal(short.ys[i], plain[i]), (bits, i)
        assert O.rel_err(plain[i].cpu().numpy(), refs[i].y16(x)) <= TOL16


@pytest.mark.parametrize("bits", (5, 8))
def test_a_group_of_one_is_a_plain_call(bits):
    from qllm_amd import ops
    descs, _keep, _refs = _case("B", bits)
    _x_np, xt = _x(4, descs[0].K, False, seed=55)
    for w in descs:
        assert torch.equal(ops.linear_forward_bitgroup([w], xt)[0], ops.linear_forward(w, xt))


def test_members_in_any_order_and_outs_given():
    """The launch sorts the members widest first; the outputs stay with the caller's order."""
    from qllm_amd import ops
    descs, _keep, _refs = _case("B", 6)
    _x_np, xt = _x(3, descs[0].K, False, seed=66)
    order = [2, 0, 1]
    outs = [torch.empty((3, descs[i].N), dtype=torch.float16, device=DEV) for i in order]
    got = ops.linear_forward_bitgroup([descs[i] for i in order], xt, outs)
    for o, g, i in zip(outs, got, order):
        assert g is o and torch.equal(o, ops.linear_forward(descs[i], xt)), i


def test_grouped_forward_in_a_graph():
    """One grouped call captured on one stream (no parallel branches), replayed twice: bit-equal to eager."""
    from qllm_amd import ops
    descs, _keep, _refs = _case("B", 8)
    _x_np, xt = _x(2, descs[0].K, False, seed=61)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = [y.clone() for y in ops.linear_forward_bitgroup(descs, xt)]
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ys = ops.linear_forward_bitgroup(descs, xt)
    for _ in range(2):
        for y in ys:
            y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for y, e in zip(ys, eager):
            assert torch.equal(y, e)


# ---- through the modules ---------------------------------------------------------------------------------------------------------------
def _siblings():
    gptq = [to_layer(synth("GPTQ", 8, 128, 512, n, "asym", False, i == 0, seed=300 + i), DEV) for i, n in enumerate((64, 32, 32))]
    hqq = [to_layer(synth("HQQ", 2, 64, 512, n, "f16", False, False, seed=310 + i), DEV) for i, n in enumerate((64, 32))]
    return gptq, hqq


def _alone(layers, x):
    groups = [l._siblings for l in layers]
    try:
        for l in layers:
            l._siblings = None
        return [l(x) for l in layers]
    finally:
        for l, g in zip(layers, groups):
            l._siblings = g


@pytest.mark.parametrize("which", ("gptq8", "hqq2"))
def test_sibling_groups_decode_with_one_launch(which):
    """On the parent of this entry the group switched itself off at one row (the planner has no grouped kernel for these widths)."""
    from qllm_amd.modeling.q_layers import fuse_siblings
    gptq, hqq = _siblings()
    layers = gptq if which == "gptq8" else hqq
    g = fuse_siblings(layers)
    x1 = torch.from_numpy(randx(1, 512, seed=1)).to(DEV)
    outs = [l(x1) for l in layers]
    assert g.grouped_launches == 1 and g.enabled
    for o, a in zip(outs, _alone(layers, x1)):
        assert torch.equal(o, a)
    # 17 rows: above the entry's rows -- the layers' own paths; the group stays on for decode
    x17 = torch.from_numpy(randx(17, 512, seed=2)).to(DEV)
    outs17 = [l(x17) for l in layers]
    assert g.grouped_launches == 1 and g.enabled
    for o, a in zip(outs17, _alone(layers, x17)):
        assert torch.equal(o, a)
    x1b = torch.from_numpy(randx(1, 512, seed=3)).to(DEV)
    outs = [l(x1b) for l in layers]
    assert g.grouped_launches == 2 and g.enabled
    for o, a in zip(outs, _alone(layers, x1b)):
        assert torch.equal(o, a)
    x4 = torch.from_numpy(randx(4, 512, seed=4)).to(DEV).reshape(2, 2, 512)   # a batch of two sequences
    outs = [l(x4) for l in layers]
    assert g.grouped_launches == 3 and outs[0].shape == (2, 2, layers[0].outfeatures)
    for o, a in zip(outs, _alone(layers, x4)):
        assert torch.equal(o, a)


@pytest.mark.parametrize("knob", ("QLLM_BITGROUP", "QLLM_BITGROUP_MAX_M"))
def test_knobs_switch_the_grouped_launch_off(knob):
    from qllm_amd import ops
    from qllm_amd.modeling.q_layers import fuse_siblings
    gptq, _hqq = _siblings()
    x1 = torch.from_numpy(randx(1, 512, seed=5)).to(DEV)
    want = [l(x1) for l in gptq]
    g = fuse_siblings(gptq)
    try:
        ops.set_knob(knob, 0)
        outs = [l(x1) for l in gptq]
    finally:
        ops.reset_knobs()
    assert g.grouped_launches == 0
    for o, w in zip(outs, want):
        assert torch.equal(o, w)
