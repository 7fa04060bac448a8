"""-m gpu: the tensor-parallel decode kernels at settings no multi-process test reaches, in ONE process (tests/allreduce_world.py): every
`AR` instantiation of the batch-1 kernel (qllm_linear_forward_allreduce, 11 (waves, round) pairs x exact / shifted last window), worlds of
1..16 ranks with the first, middle and last rank launched, launches of 512 blocks (more than there are CUs: the "last block sums" ticket
taken by blocks that were not co-resident), HQQ layers with fp16 zero points, the one-shot kernel alone, graph replay, guard bands.

The epoch, flags, ticket and slots are plain device memory: before rank rho is launched the test writes into rho's staging buffer what
the ranks that have not run yet will push (vector, then flag = epoch), launches that ONE rank and checks the result, the status word,
the epoch and ticket, and every byte of every rank's buffer (guards included) against a shadow copy that follows the protocol.  Ranks run
round-robin, so the slots of ranks below rho come from real launches.  Every wait of a kernel is satisfied before the kernel starts (the
harness reads the flags back on the host first): no second process, no second stream, nothing left for a running kernel to wait for.

Every comparison is bit for bit.  Expected sums are computed on the CPU (allreduce_world.expected_sum: fp32, rank order onto 0.0f, one
rounding); the fused launch's pushed vector is the plain launch's y on the same shard (include/qllm_mi355x.h: "bit-identical to
qllm_linear_forward + qllm_allreduce_oneshot").  Staging buffers are qllm_comm_alloc memory wrapped zero-copy as tensors through
__cuda_array_interface__.  Layers are random integers generated on the device in the GPTQ / HQQ layouts and re-laid-out by
qllm_repack_native, as the modules do."""
import numpy as np
import pytest
import torch

from allreduce_world import World, bits_of, cancelling_large, expected_sum, mixed_vectors
from gpu_util import guarded
from test_route_memory_gpu import Outputs, _guarded_descriptor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = {"f16": torch.float16, "bf16": torch.bfloat16}
VARIANTS = (("GPTQ", "asym", False), ("HQQ", "f16", True), ("GPTQ", "sym", True), ("HQQ", "f16", False), ("GPTQ", "asym", True), ("GPTQ", "sym", False))
G = 128


def _lib():
    from qllm_amd import _lib as L
    return L.load()


def _layer(layout, zk, bias, K, N, seed):
    """(native descriptor, keepalive): a random 4-bit g128 layer built on the device in its reference layout (any int32 is a valid word),
    scales as tests/test_strip1_gpu.py scales them so y stays finite, re-laid-out by the library's own repack."""
    from qllm_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(seed)
    qweight = torch.randint(-2 ** 31, 2 ** 31, (K // 8, N), dtype=torch.int64, device=DEV, generator=gen).to(torch.int32)
    scales = ((torch.rand((K // G, N), device=DEV, generator=gen) * 0.010 + 0.002) * ((4096 / K) ** 0.5 * 0.5)).half()
    if layout == "HQQ":
        qzeros = (torch.rand((K // G, N), device=DEV, generator=gen) * 15).half()
    elif zk == "sym":
        qzeros = None
    else:
        qzeros = torch.randint(-2 ** 31, 2 ** 31, (K // G, N // 8), dtype=torch.int64, device=DEV, generator=gen).to(torch.int32)
    b = (torch.randn(N, device=DEV, generator=gen) * 0.5).half() if bias else None
    w, keep = ops.repack_native(*ops.make_weight(layout, qweight, scales, qzeros, None, b, K, N, G, 4))
    L = ops._lib
    assert w.layout == (L.LAYOUT_NATIVE_F16Z if layout == "HQQ" else L.LAYOUT_NATIVE) and (w.qzeros is None) == (zk == "sym")
    return w, keep


def _x(K, dtype, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn((1, K), device=DEV, generator=gen).to(dtype)


def _plain(w, x):
    from qllm_amd import ops
    y = ops.linear_forward(w, x)
    assert bool(torch.isfinite(y).all())
    return y


def _plan(nw, rnd, exact):
    return f"strip1 nw={nw} round={rnd}{' exact' if exact else ''} grid=strips x 1 layout=strip-major"


def _dev_vec(bits, dtype):
    return torch.from_numpy(bits.view(np.int16)).to(DEV).view(dtype)


# ---- A. every AR form, a world of one, against the plain launch --------------------------------------------------------------------------
# (K not exact, K exact) of every (waves, round) pair of launch_strip1_allreduce; N = 256: 16 strips, N = 8192: 512 strips
FORMS_256 = [(4, 8, 256, 1024), (4, 16, 1152, 2048), (4, 32, 2176, 4096), (8, 24, 5120, 6144), (8, 32, 6656, 8192),
             (15, 24, 11008, 11520), (16, 24, 11776, 12288), (16, 32, 14336, 16384)]
FORMS_8192 = [(8, 16, 3840, 4096, None), (7, 16, 3200, 3584, None), (16, 16, 6656, 8192, "QLLM_S1_T256_NW16")]
FORMS = [(nw, rnd, k, 256, ex, None) for nw, rnd, k0, k1 in FORMS_256 for k, ex in ((k0, False), (k1, True))]
FORMS += [(nw, rnd, k, 8192, ex, knob) for nw, rnd, k0, k1, knob in FORMS_8192 for k, ex in ((k0, False), (k1, True))]
assert len(FORMS) == 22 and len({(f[0], f[1], f[4]) for f in FORMS}) == 22


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("nw,rnd,K,N,exact,knob", FORMS, ids=[f"{f[0]}x{f[1]}{'e' if f[4] else ''}-K{f[2]}-N{f[3]}" for f in FORMS])
def test_every_ar_form_in_a_world_of_one_is_the_plain_launch(nw, rnd, K, N, exact, knob, dt):
    """qllm_linear_forward_allreduce(world = 1) == qllm_linear_forward, bit for bit (one rank's fp32 round trip is the identity), three
    calls in a row (parities 1, 0, 1: the third finds the first's data in its slot); the plan string pins the instantiation."""
    from qllm_amd import ops
    dtype = DTYPES[dt]
    layout, zk, bias = VARIANTS[FORMS.index((nw, rnd, K, N, exact, knob)) % len(VARIANTS)]
    w, keep = _layer(layout, zk, bias, K, N, seed=K + N)
    slot = N * 2 if N == 8192 else 64 << 10
    try:
        if knob:
            ops.set_knob(knob, 1)
        with World(_lib(), 1, slot) as world:
            for call in range(3):
                assert ops.plan_describe([w], 1) == _plan(nw, rnd, exact), ops.plan_describe([w], 1)
                x = _x(K, dtype, seed=7 * K + call)
                want = _plain(w, x)
                if knob:   # the form only this knob reaches: its plain launch against the default form's (8 waves x 32) on the same layer,
                    ops.reset_knobs()   # within the bounds tests/test_strip1_gpu.py holds every form to against the oracle
                    base = _plain(w, x).float()
                    ops.set_knob(knob, 1)
                    assert float((want.float() - base).abs().max() / base.abs().max()) <= (2e-3 if dt == "f16" else 2e-2)
                y = torch.full((1, N), float("nan"), dtype=dtype, device=DEV)
                e, parity = world.begin(0, [want])
                assert parity == (call + 1) & 1
                world.fused(0, w, x, y)
                world.finish(0, e, parity, want)
                world.end_round()
                assert torch.equal(y.view(torch.int16), want.view(torch.int16)), (call, int((y.view(torch.int16) != want.view(torch.int16)).sum()))
    finally:
        ops.reset_knobs()


# ---- B. the fused entry in worlds of 2, 3, 8 and 16 ---------------------------------------------------------------------------------------
TP_LAYERS = [(1024, 8192, 4, 8, True), (3584, 8192, 7, 16, True), (5504, 4096, 8, 24, False)]   # K per rank, N, the form


def _round(world, vectors, dt, launch):
    """One round-robin round: every rank in turn, `launch(rho) -> result tensor`; returns the expected bits"""
    want = expected_sum([bits_of(v) for v in vectors], dt)
    for rho in range(world.W):
        e, parity = world.begin(rho, vectors, real=range(rho))
        got = launch(rho)
        world.finish(rho, e, parity, vectors[rho])
        assert np.array_equal(bits_of(got), want), (f"epoch {e} rank {rho} of {world.W}", int((bits_of(got) != want).sum()))
    world.end_round()
    return want


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("W", [2, 3, 8, 16])
@pytest.mark.parametrize("K,N,nw,rnd,exact", TP_LAYERS, ids=[f"K{c[0]}-N{c[1]}" for c in TP_LAYERS])
def test_fused_launch_in_worlds_of_2_to_16(K, N, nw, rnd, exact, W, dt):
    """W independent shards (bias on rank 0's only, as parallel.shard_rows gives it), every rank its own x.  Rank r pushes the bits of the
    plain launch on its shard; every rank's result is the CPU's rank-ordered fp32 sum of those.  Two fused rounds (both parities), then a
    round in which the odd ranks run the plain launch + qllm_allreduce_oneshot on the same buffers, then (worlds of three and more) a
    fused round built so that a sum in another order has other bits."""
    from qllm_amd import ops
    dtype = DTYPES[dt]
    layout, zk, _ = VARIANTS[TP_LAYERS.index((K, N, nw, rnd, exact))]
    shards = [_layer(layout, zk, r == 0, K, N, seed=1000 * K + r) for r in range(W)]
    for w, _ in shards:
        assert ops.plan_describe([w], 1) == _plan(nw, rnd, exact), ops.plan_describe([w], 1)
    with World(_lib(), W, N * 2 if N == 8192 else 64 << 10) as world:
        for rnd_no in range(4 if W >= 3 else 3):
            xs = [_x(K, dtype, seed=31 * K + 17 * rnd_no + r) for r in range(W)]
            descs = [w for w, _ in shards]
            mixed, pair = rnd_no == 2, rnd_no == 3
            if pair:
                # a round whose sum depends on the ORDER (real shard outputs are all of one magnitude: their fp32 sum rounds to the same
                # 16 bits in almost any order).  The last two ranks run the same shard on x and -x scaled up by a power of two -- outputs
                # +L and (but for an element here and there) exactly -L, |L| in the thousands (fp16) / about ten thousand (bf16) -- and all others on x scaled down: in rank
                # order the small ranks' sum is rounded to fp32's grid at L before L cancels; a sum that meets the pair first keeps it whole
                up = 2.0 ** (10 if dt == "f16" else 13)   # (x stays inside fp16's range: the kernel converts bf16 activations to fp16)
                xs = [x * 2.0 ** -6 for x in xs]
                xs[W - 2] = xs[W - 2] * 2.0 ** 6 * up
                xs[W - 1] = -xs[W - 2]
                descs[W - 1] = descs[W - 2]
            ys = [_plain(w, x) for w, x in zip(descs, xs)]
            if pair:
                host = [bits_of(y) for y in ys]
                differ = (expected_sum(host, dt) != expected_sum(host, dt, order=range(W - 1, -1, -1))).mean()
                assert differ >= 0.01, ("the round cannot tell the rank order", differ)

            def launch(rho):
                if mixed and rho % 2:
                    t = ys[rho].clone()
                    world.oneshot(rho, t)
                    return t
                y = torch.full((1, N), float("nan"), dtype=dtype, device=DEV)
                world.fused(rho, descs[rho], xs[rho], y)
                return y

            _round(world, ys, dt, launch)


# ---- C. the one-shot kernel alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("W", [1, 2, 5, 8, 16])
def test_oneshot_kernel_round_robin(W, dt):
    """n = 8200 is past one pass of the kernel's 1024 threads, n = slot_bytes / 2 fills the slot, n = 8 leaves the larger calls' data in the
    rest of it; three rounds each.  A world of one returns its input."""
    dtype = DTYPES[dt]
    slot = 32 << 10
    with World(_lib(), W, slot) as world:
        for n in (8200, slot // 2, 8):
            for rnd_no in range(3):
                host = mixed_vectors(W, n, dt, seed=100 * W + 10 * rnd_no + n % 7)
                vectors = [_dev_vec(v, dtype) for v in host]

                def launch(rho):
                    t = vectors[rho].clone()
                    world.oneshot(rho, t)
                    return t

                want = _round(world, vectors, dt, launch)
                assert W > 1 or np.array_equal(want, host[0])


# ---- D. graph replay -----------------------------------------------------------------------------------------------------------------------
def _capture(call):
    """warm up on a side stream, then capture, as tests/test_tp_collective_gpu.py does"""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        call()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("W,rho", [(1, 0), (3, 2)])
@pytest.mark.parametrize("form", ["fused", "oneshot"])
def test_graph_replay_advances_the_epoch(form, W, rho, dt):
    """One rank's launch captured into a graph and replayed three times.  No other rank runs: before every replay torch operations on the
    replay's stream write the other ranks' vectors and flags for the next epoch (the epoch is read and bumped by the kernel itself)."""
    dtype = DTYPES[dt]
    K, N = 3584, 8192
    w, keep = _layer("HQQ", "f16", True, K, N, seed=5)
    n = N if form == "fused" else 8200
    x = torch.empty((1, K), dtype=dtype, device=DEV)     # the graph's static tensors
    t = torch.empty(n, dtype=dtype, device=DEV)

    def feed(step):
        """this epoch's vectors: the launched rank's from its own input, the others chosen"""
        host = mixed_vectors(W, n, dt, seed=50 * W + step)
        vectors = [_dev_vec(v, dtype) for v in host]
        if form == "fused":
            x.copy_(_x(K, dtype, seed=200 + step))
            vectors[rho] = _plain(w, x).reshape(-1)
            t.fill_(float("nan"))
            if W == 3:   # ranks 0 and 1 hold +L and -L: in rank order they cancel before rank 2's y arrives, in any other order y is
                large = _dev_vec(cancelling_large(n, dt, seed=step), dtype)   # rounded to fp32's grid at L (about y's last bit) first
                vectors[0], vectors[1] = large, -large
        else:
            t.copy_(vectors[rho])
        return vectors

    with World(_lib(), W, 32 << 10) as world:
        call = (lambda: world.fused(rho, w, x, t)) if form == "fused" else (lambda: world.oneshot(rho, t))

        def step(no, run):
            vectors = feed(no)
            host = [bits_of(v) for v in vectors]
            want = expected_sum(host, dt)
            assert W < 3 or (want != expected_sum(host, dt, order=range(W - 1, -1, -1))).mean() >= 0.01
            e, parity = world.begin(rho, vectors)
            assert e == no + 1
            run()
            world.finish(rho, e, parity, vectors[rho])
            world.end_round()
            assert np.array_equal(bits_of(t), want), (form, W, f"epoch {e}", int((bits_of(t) != want).sum()))

        step(0, lambda: _capture(call))          # the warm-up launch is epoch 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for no in (1, 2, 3):
            step(no, g.replay)
        del g


# ---- E. memory ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("K,N,variant", [(1024, 8192, 1), (3584, 8192, 4), (11008, 256, 1)], ids=["K1024-N8192", "K3584-N8192", "K11008-N256"])
def test_fused_launch_between_guard_bands(K, N, variant, dt):
    """y in a buffer of sentinel halves with bands on both sides (tests/test_route_memory_gpu.py), x, scales, fp16 zero points and bias
    between NaN bands: a world of three, every rank launched, two rounds."""
    dtype = DTYPES[dt]
    W = 3
    layout, zk, _ = VARIANTS[variant]
    hold, shards = [], []
    for r in range(W):
        w, keep = _layer(layout, zk, r == 0, K, N, seed=77 * K + r)
        shards.append((w, _guarded_descriptor(w, keep, hold), keep))
    with World(_lib(), W, N * 2 if N == 8192 else 64 << 10) as world:
        for rnd_no in range(2):
            xs = [_x(K, dtype, seed=3 * K + 5 * rnd_no + r) for r in range(W)]
            gxs = [guarded(x, 4096)[1] for x in xs]
            ys = [_plain(w, x) for (w, _, _), x in zip(shards, xs)]
            outs = []

            def launch(rho):
                out = Outputs(1, [N], dtype)
                outs.append(out)
                world.fused(rho, shards[rho][1], gxs[rho], out.ys[0])
                return out.ys[0]

            _round(world, ys, dt, launch)
            for rho, out in enumerate(outs):
                out.check(f"rank {rho} round {rnd_no}")
