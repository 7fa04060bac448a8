"""BASELINE configs[4]: Llama-2-70B AWQ w4 g128, per-layer matmuls sharded column-parallel over 8 GPUs with one RCCL
all-reduce per Megatron pair.  Used by bench.py:

    python -m torch.distributed.run --nproc-per-node 8 ... bench.py --gpus 8 --tp 8     the real thing (one rank per GPU)
    python bench.py --tp 1                                                            the per-rank shard shapes, no collective
    bench.py --full                                                                   extra.tp_shard_* via shard_shapes_leg()

Per rank and layer at TP = P (hidden 8192, 64 heads / 8 KV heads, intermediate 28672, 80 layers):
    q/k/v   column-parallel, 8192 -> (8192 + 2 x 1024) / P, one grouped launch (sibling group), output stays sharded
    o       row-parallel,    8192 / P -> 8192, partial sums -> ONE all-reduce of [M, 8192]
    gate/up column-parallel, 8192 -> 2 x 28672 / P, one grouped launch, output stays sharded
    down    row-parallel,    28672 / P -> 8192, ONE all-reduce
so a layer costs four kernel launches and two all-reduces on the compute stream (qllm_amd/parallel.py wrappers; the
attention / activation glue between the linears is not part of the hot path and is stood in for by feeding the q and gate
shards forward, which have exactly the row-parallel layers' input widths).  The reference has no distributed code at all
(qllm/modeling/base.py:294-295 asserts the sharded branch away).
"""
import json
import os
import time

import torch

H70, KV70, I70, L70, G = 8192, 1024, 28672, 80, 128
M_MAX_ONESHOT = 4   # rows whose [M, 8192] sum still travels through the one-shot kernel (64 KB)
HBM_PEAK_GBPS = 8000.0
MFMA_PEAK_TFLOPS = 2500.0


def _alg_bytes(K, N, M, g=G):
    Gn = (K + g - 1) // g
    return K * N // 2 + Gn * N * 2 + Gn * N // 2 + 2 * M * K + 2 * M * N


def _layer(cls, K, N, dev, gen):
    layer = cls(4, G, K, N, False, dtype=torch.float16)
    layer.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, layer.qweight.shape, dtype=torch.int32, device=dev, generator=gen)
    layer.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, layer.qzeros.shape, dtype=torch.int32, device=dev, generator=gen)
    layer.scales = ((torch.rand(layer.scales.shape, device=dev, generator=gen) * 0.4 + 0.8) / (K ** 0.5 * 6.5)).to(torch.float16)
    return layer.to(dev)


class ShardBlock(torch.nn.Module):
    """One decoder layer's shards on this rank, as the Megatron pairing leaves them (built directly at shard shapes: the
    synthetic integers of a shard are as good as a slice of synthetic full-size integers; tests/ cover slicing)."""

    def __init__(self, cls, P, dev, gen, group=None, reducer=None):
        super().__init__()
        from qllm_amd import parallel as TP
        self.q_proj = _layer(cls, H70, H70 // P, dev, gen)
        self.k_proj = _layer(cls, H70, KV70 // P, dev, gen)
        self.v_proj = _layer(cls, H70, KV70 // P, dev, gen)
        self.o_proj = TP.RowParallelQuantLinear(_layer(cls, H70 // P, H70, dev, gen), group, reducer=reducer)
        self.gate_proj = _layer(cls, H70, I70 // P, dev, gen)
        self.up_proj = _layer(cls, H70, I70 // P, dev, gen)
        self.down_proj = TP.RowParallelQuantLinear(_layer(cls, I70 // P, H70, dev, gen), group, reducer=reducer)

    def forward(self, h):
        q = self.q_proj(h)
        self.k_proj(h)
        self.v_proj(h)
        o = self.o_proj(q)          # row-parallel: all-reduce inside (world > 1)
        gate = self.gate_proj(o)
        self.up_proj(o)
        return self.down_proj(gate)  # all-reduce inside


def shard_bytes_per_token(P, n_layers, M=1):
    per = (_alg_bytes(H70, H70 // P, M) + 2 * _alg_bytes(H70, KV70 // P, M) + _alg_bytes(H70 // P, H70, M) +
           2 * _alg_bytes(H70, I70 // P, M) + _alg_bytes(I70 // P, H70, M))
    return n_layers * per


def shard_flops(P, n_layers, M):
    return n_layers * 2.0 * M * (2 * H70 * H70 // P + 2 * H70 * KV70 // P + 3 * H70 * I70 // P)


def _capture(fn, warm=2):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(warm):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = fn()
    g.replay()   # (capturing executes nothing: make `out` the step's real output before a caller checks it -- bench.capture)
    torch.cuda.synchronize()
    return g, out


def _time(fn, iters, warm=10):
    for _ in range(warm):   # (untimed: the clock ramp after the stack was built -- bench.time_events)
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def build_stack(P, n_layers, dev, seed, group=None, reducer=None):
    from qllm_amd.modeling.q_layers import WQLinear_GEMM, install_sibling_groups
    gen = torch.Generator(device=dev).manual_seed(seed)
    blocks = torch.nn.ModuleList([ShardBlock(WQLinear_GEMM, P, dev, gen, group, reducer) for _ in range(n_layers)])
    install_sibling_groups(blocks, [WQLinear_GEMM])
    return blocks


def shard_shapes_leg(dev, n_layers=80):
    """1 GPU: what one rank of an 8-way tensor-parallel Llama-2-70B executes (no collective), decode M=1 and prefill M=2048.
    80 layers = the model's depth: one hipGraph per token, as a serving loop would replay it (rounds 3-4 timed a 16-layer graph and
    charged the per-replay boundary, ~8 us, to 16 layers instead of 80)."""
    from qllm_amd import ops
    P = 8
    blocks = build_stack(P, n_layers, dev, seed=77)

    def fwd(h):
        for b in blocks:
            h = b(h)
        return h

    out = {}
    h1 = torch.randn(1, H70, device=dev, dtype=torch.float16)
    g, y = _capture(lambda: fwd(h1))
    ms = _time(g.replay, 20)
    del g
    nbytes = shard_bytes_per_token(P, n_layers, 1)
    b0 = blocks[0]
    out["tp_shard_decode_m1"] = {
        "what": f"per-rank shards of Llama-2-70B at TP=8 ({n_layers} layers, 4 launches per layer, no collective)",
        "us_per_layer": round(ms * 1e3 / n_layers, 2), "GBps": round(nbytes / ms / 1e6, 1),
        "frac_of_hbm_peak": round(nbytes / ms / 1e6 / HBM_PEAK_GBPS, 4),
        "plans": {"qkv 8192->1024+128+128": b0.q_proj._siblings.describe(1),
                  "o 1024->8192": ops.plan_describe([b0.o_proj.shard.decode_descriptor()], 1),
                  "gate/up 8192->2x3584": b0.gate_proj._siblings.describe(1),
                  "down 3584->8192": ops.plan_describe([b0.down_proj.shard.decode_descriptor()], 1)}}
    xp = torch.randn(2048, H70, device=dev, dtype=torch.float16)
    few = torch.nn.ModuleList(list(blocks)[:4])

    def fwd_p():
        h = xp
        for b in few:
            h = b(h)
        return h
    g, _ = _capture(fwd_p)
    ms = _time(g.replay, 10)
    del g
    tf = shard_flops(P, 4, 2048) / ms / 1e9
    out["tp_shard_prefill_m2048"] = {"ms_per_4_layers": round(ms, 3), "TFLOPs": round(tf, 1),
                                     "frac_of_mfma_peak": round(tf / MFMA_PEAK_TFLOPS, 4)}
    return out


def verify_sharding(world, rank, dev, group=None):
    """Before anything is timed: ONE decoder layer's linears at the full Llama-2-70B shapes, identical on every rank (same seed),
    sharded with qllm_amd.parallel (shard_columns / shard_rows slices of those very integers) -- the tensor-parallel result must
    equal the unsharded HIP result computed on the same rank: bit-exact for the gathered column-parallel layer (columns are
    independent), within 2e-3 for the Megatron pairs (the all-reduce changes the summation order).  Raises on mismatch."""
    from qllm_amd import parallel as TP
    from qllm_amd.modeling.q_layers import WQLinear_GEMM
    gen = torch.Generator(device=dev).manual_seed(20240607)   # NOT rank-dependent
    q, o = _layer(WQLinear_GEMM, H70, H70, dev, gen), _layer(WQLinear_GEMM, H70, H70, dev, gen)
    gate, down = _layer(WQLinear_GEMM, H70, I70, dev, gen), _layer(WQLinear_GEMM, I70, H70, dev, gen)
    report = {}
    for M in (1, 16):
        x = torch.randn(M, H70, device=dev, dtype=torch.float16, generator=gen)
        y_gate = gate(x)
        y_cp = TP.ColumnParallelQuantLinear.from_full(gate, group, gather_output=True)(x)
        if not torch.equal(y_cp, y_gate):
            raise AssertionError(f"column-parallel gate_proj (gathered) differs from the unsharded layer at M={M}")
        for name, a, b in (("q->o", q, o), ("gate->down", gate, down)):
            y_full = b(a(x))
            col = TP.ColumnParallelQuantLinear.from_full(a, group, gather_output=False)
            row = TP.RowParallelQuantLinear.from_full(b, group, input_is_parallel=True)
            y_tp = row(col(x))
            err = float((y_tp.float() - y_full.float()).abs().max() / y_full.float().abs().max())
            if not err <= 2e-3:
                raise AssertionError(f"Megatron pair {name} at M={M}: sharded vs unsharded relative error {err}")
            report[f"{name} M={M}"] = round(err, 6)
    torch.cuda.synchronize()
    if rank == 0:
        print(f"[tp_bench] sharded == unsharded on {world} rank(s): column-parallel bit-exact, Megatron pairs rel err {report}", flush=True)
    del q, o, gate, down
    torch.cuda.empty_cache()
    return report


def measure(args, world, rank, dev, info):
    """The tensor-parallel leg on `world` ranks (or 1 rank running the TP=8 shard shapes without a collective): returns the record
    on rank 0, None on the others.  EVERY rank must call it (collectives inside).  `args.tp_layers` (default: all 80) shortens the
    stack for smoke runs (tests/test_tp_collective_gpu.py drives this function with two gloo ranks on one GPU, so that the first
    8-GPU lease is not its first execution).  Callers: run() (`bench.py --tp N`) and bench.py's `--gpus N --full` run, which puts the
    record on its JSON line as extra.tp70b (round-5 verdict: the driver only ever passes --gpus N)."""
    import torch.distributed as dist
    P = world if world > 1 else 8
    if world > 1 and getattr(args, "tp", 0) not in (0, world):   # (0: bench.py --gpus N without --tp: the degree is the world size)
        raise SystemExit(f"--tp {args.tp} needs --gpus {args.tp} (one rank per GPU)")
    n_layers = int(getattr(args, "tp_layers", 0) or L70)
    backend = dist.get_backend() if world > 1 else None
    if rank == 0:
        print(f"[tp_bench] world_size={dist.get_world_size() if world > 1 else 1} backend={backend} tp_degree={P} layers={n_layers}", flush=True)
    parity = None
    if world > 1:
        parity = verify_sharding(world, rank, dev)
    # the timed stack is built at shard shapes from per-rank seeds (as good as slices of synthetic full-size integers and 8 x
    # less to generate; the slicing itself was just verified on one full-size layer)
    # decode-sized all-reduces ([1, 8192] fp16 = 16 KB): the one-shot peer-write kernel (qllm_amd/comm.py) unless QLLM_TP_ONESHOT=0
    reducer, reducer_mode = None, "dist.all_reduce"
    if world > 1 and os.environ.get("QLLM_TP_ONESHOT", "1") != "0":
        try:
            from qllm_amd.comm import OneShotAllReduce
            reducer = OneShotAllReduce(max_bytes=M_MAX_ONESHOT * H70 * 2)
            reducer_mode = "one-shot peer-write kernel (HIP IPC staging buffers)"
            if reducer.disabled_reason is not None:   # (its collective self-test failed: every rank falls back together)
                reducer_mode = f"dist.all_reduce (one-shot self-test failed: {reducer.disabled_reason})"
        except Exception as e:  # noqa: BLE001  (e.g. IPC not permitted in this container): RCCL serves the sums
            reducer_mode = f"dist.all_reduce (one-shot unavailable: {type(e).__name__}: {e})"
    if rank == 0:
        print(f"[tp_bench] row-parallel sums: {reducer_mode}", flush=True)
    blocks = build_stack(P, n_layers, dev, seed=4321 + rank, reducer=reducer)
    M = 1
    h0 = torch.randn(M, H70, device=dev, dtype=torch.float16)
    if world > 1:
        dist.broadcast(h0, 0)

    def step():
        h = h0
        for b in blocks:
            h = b(h)
        return h

    # Graph path: one rank (no collective) or RCCL ("nccl": its collectives are stream operations and capture with the kernels).
    # Any other backend (gloo: host-side collectives) runs eagerly BY DESIGN; a failed RCCL capture is reported, not hidden.
    # (round 5: with the one-shot reducer every sum of the step is one of the library's own kernels -- fused into the row-parallel
    #  launch at batch 1 -- so the step captures whatever the backend)
    #  -- a reducer whose self-test failed serves nothing: its sums are dist.all_reduce calls again, host-side under gloo)
    oneshot_live = reducer is not None and reducer.disabled_reason is None
    want_graph = world == 1 or ((backend == "nccl" or oneshot_live) and os.environ.get("QLLM_TP_GRAPH", "1") != "0")
    graph_mode = "eager (backend %s: collectives are not stream operations)" % backend if not want_graph else None
    run_step = step
    out = None
    if want_graph:
        try:
            graph, out = _capture(step)
            run_step = graph.replay
            graph_mode = "hipGraph replay"
        except Exception as e:  # noqa: BLE001
            torch.cuda.synchronize()
            graph_mode = f"eager (capture FAILED: {type(e).__name__}: {e})"
    if out is None:
        out = step()
    if rank == 0:
        print(f"[tp_bench] step runs as: {graph_mode}", flush=True)
    assert torch.isfinite(out.float()).all()

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        run_step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run_step()
    barrier()
    wall = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([wall], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t[0])
    ms_per_step = wall * 1e3 / args.steps
    # the same step with the row-parallel launches and their all-reduces as TWO launches each (fuse_reduce off): what the fusion buys
    ms_unfused = None
    fused = bool(reducer is not None and world > 1 and getattr(blocks[0].o_proj, "fuse_reduce", False))
    if fused:
        for b in blocks:
            b.o_proj.fuse_reduce = b.down_proj.fuse_reduce = False
        run2 = step
        if want_graph and graph_mode == "hipGraph replay":
            try:
                graph2, _ = _capture(step)
                run2 = graph2.replay
            except Exception:  # noqa: BLE001
                torch.cuda.synchronize()
        for _ in range(args.warmup):
            run2()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            run2()
        barrier()
        w2 = time.perf_counter() - t0
        t = torch.tensor([w2], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        ms_unfused = float(t[0]) * 1e3 / args.steps
        for b in blocks:
            b.o_proj.fuse_reduce = b.down_proj.fuse_reduce = True
        ms_fused = ms_per_step
        # the step that is REPORTED is the faster of the two on this topology (identical on every rank: both times are maxima over
        # ranks).  Two ranks sharing one GPU (the only multi-rank run this repository has had) favour two launches: the fused
        # launch's last block spins for the peer's flags while the peer's own launch waits for the device.
        keep_fused = ms_fused <= ms_unfused
        if not keep_fused:
            ms_per_step, wall = ms_unfused, ms_unfused * args.steps / 1e3
            for b in blocks:
                b.o_proj.fuse_reduce = b.down_proj.fuse_reduce = False
        if rank == 0:
            print(f"[tp_bench] row-parallel GEMV + all-reduce: fused (one launch) {ms_fused:.4f} ms per step, unfused (two launches) {ms_unfused:.4f}"
                  f" -> reporting the {'fused' if keep_fused else 'unfused'} step", flush=True)
        fused = keep_fused
    ar_us = ar1_us = None
    if world > 1:  # the decode-sized all-reduce on its own ([1, 8192] fp16 = 16 KB: latency-bound over xGMI)
        buf = torch.zeros(M, H70, device=dev, dtype=torch.float16)
        for _ in range(10):
            dist.all_reduce(buf)
        torch.cuda.synchronize()
        ar_us = _time(lambda: dist.all_reduce(buf), 200) * 1e3
        if reducer is not None:
            for _ in range(10):
                reducer.all_reduce(buf)
            torch.cuda.synchronize()
            ar1_us = _time(lambda: reducer.all_reduce(buf), 200) * 1e3
            reducer.check()
    nbytes = shard_bytes_per_token(P, n_layers, M)
    rec = None
    if rank == 0:
        rec = {
            "metric": "decode_tokens_per_s_llama2_70b_w4a16_g128_linear_stack_tp", "value": round(M * args.steps / wall, 2),
            "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
            "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "f16", "data": "synthetic",
            "config": {"workload": "llama2-70b-awq-w4-g128-decode-b1-tp", "tp_degree": P, "ranks": world, "backend": backend,
                       "layers": n_layers, "launches_per_layer": 4, "all_reduces_per_layer": 2 if world > 1 else 0,
                       "row_parallel_all_reduce_fused_into_gemv": fused, "ranks_seen": dist.get_world_size() if world > 1 else 1,
                       "graph": graph_mode, "parallelism": f"tp{P}" + ("" if world > 1 else " (1 rank, no collective)"),
                       "device": info["arch"]},
            "roofline": {"bound": "hbm", "kernel": "qllm::strip1_kernel", "achieved": round(nbytes / ms_per_step / 1e6, 1),
                         "peak": HBM_PEAK_GBPS, "unit": "GB/s (per rank)", "frac": round(nbytes / ms_per_step / 1e6 / HBM_PEAK_GBPS, 4),
                         "traffic": None},
            "all_reduce_us_16KB": None if ar_us is None else round(ar_us, 2),
            "oneshot_all_reduce_us_16KB": None if ar1_us is None else round(ar1_us, 2), "row_parallel_sums": reducer_mode,
            "ms_per_step_unfused_all_reduce": None if ms_unfused is None else round(ms_unfused, 4),
            "ms_per_step_fused_all_reduce": None if ms_unfused is None else round(ms_fused, 4),
            "sharded_vs_unsharded": None if parity is None else {"column_parallel": "bit-exact", "megatron_pairs_rel_err": parity},
            "cpu_baseline": None}
    if reducer is not None:
        reducer.close()
    del blocks
    torch.cuda.empty_cache()
    return rec


def stub_measure(args, world, rank):
    """QLLM_BENCH_STUB=1 (tests/test_bench_contract_cpu.py, no GPU): the collective pattern of measure() -- broadcast of the input,
    barriers, max-over-ranks of the wall time -- on gloo with a trivial CPU step, so that `bench.py --gpus N` carries an
    extra.tp70b object whose keys are the real leg's.  Marked as a stub; carries no measurement."""
    import torch.distributed as dist
    h0 = torch.ones(1, 8)
    if os.environ.get("QLLM_BENCH_STUB_HANG") == str(rank):   # (the watchdog's test: this rank never reaches the collective)
        time.sleep(3600)
    if world > 1:
        dist.broadcast(h0, 0)
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        h0 = h0 * 1.0
    if world > 1:
        dist.barrier()
    t = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    if world > 1:
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank != 0:
        return None
    return summary({"value": None, "ms_per_step": round(float(t[0]) * 1e3 / max(args.steps, 1), 4), "n_gpus": world,
                    "config": {"workload": "stub", "tp_degree": world, "ranks_seen": dist.get_world_size() if world > 1 else 1,
                               "backend": dist.get_backend() if world > 1 else None, "graph": None, "layers": 0,
                               "row_parallel_all_reduce_fused_into_gemv": None},
                    "roofline": None, "all_reduce_us_16KB": None, "oneshot_all_reduce_us_16KB": None,
                    "row_parallel_sums": "STUB", "ms_per_step_unfused_all_reduce": None, "ms_per_step_fused_all_reduce": None,
                    "sharded_vs_unsharded": None}, stub=True)


def summary(rec, stub=False):
    """extra.tp70b of bench.py's `--gpus N` line: the tensor-parallel record, flattened to the keys the round-5 verdict names."""
    c = rec["config"]
    out = {"what": "Llama-2-70B AWQ w4 g128 decode, batch 1, column/row-parallel over the run's ranks, one all-reduce per Megatron pair "
                   "(BASELINE configs[4]; tools/tp_bench.py)",
           "tokens_per_s": rec["value"], "ms_per_step": rec["ms_per_step"], "tp_degree": c["tp_degree"], "layers": c["layers"],
           "ranks_seen": c["ranks_seen"], "backend": c["backend"], "graph": c["graph"],
           "all_reduce_us_16KB": rec["all_reduce_us_16KB"], "oneshot_all_reduce_us_16KB": rec["oneshot_all_reduce_us_16KB"],
           "row_parallel_sums": rec["row_parallel_sums"],
           "ms_per_step_fused_all_reduce": rec["ms_per_step_fused_all_reduce"],
           "ms_per_step_unfused_all_reduce": rec["ms_per_step_unfused_all_reduce"],
           "reported_step_fuses_all_reduce": c["row_parallel_all_reduce_fused_into_gemv"],
           "sharded_vs_unsharded": rec["sharded_vs_unsharded"],
           "per_rank_roofline": rec["roofline"]}
    if stub:
        out["stub"] = "QLLM_BENCH_STUB=1: launch-path test on CPU, not a measurement"
    return out


def run(args, world, rank, dev, info):
    """bench.py --tp N: the tensor-parallel leg as the run's ONE JSON line."""
    import torch.distributed as dist
    rec = measure(args, world, rank, dev, info)
    if rank == 0:
        print(json.dumps(rec), flush=True)
    if world > 1 and not getattr(args, "keep_process_group", False):
        dist.destroy_process_group()
