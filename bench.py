#!/usr/bin/env python3
"""Headline benchmark (BASELINE.json): W4A16 g128 dequant-GEMM on Llama-2-7B shapes.

    python bench.py --gpus N --steps K --warmup W          (N > 1 without WORLD_SIZE in the environment: re-launches itself as
                                                            `python -m torch.distributed.run --nnodes=1 --nproc-per-node N
                                                            --master-addr 127.0.0.1 ... bench.py <same flags>`; under a launcher
                                                            it reads RANK / LOCAL_RANK / WORLD_SIZE / MASTER_*)
    python bench.py ... --full                             also every side measurement below (sustained phase, PMC traffic,
                                                            extra legs, cpu_baseline; with N > 1 the tensor-parallel leg)
    python bench.py ... --dump-outputs DIR                 after the timed steps, rank 0 writes what its last step returned:
                                                            DIR/decode_out.npy, float32 [1, 4096] (inputs are seeded: two builds
                                                            run with the same flags can be compared output for output)

A plain run (no --full) sets up, warms up, times exactly K steps (HIP events and a host clock around them, ending in a
device synchronise), writes the outputs if asked, and prints the line: metric, value, unit, higher_is_better, dtype,
ms_per_step (= wall time of the K steps / K), config and roofline (from the timed steps' events; traffic null).

Workload (config.workload = "llama2-7b-awq-w4-g128-decode-b1"): BASELINE.json configs[1] -- the 32 x 7 quantized
linears of Llama-2-7B in the AWQ "GEMM" pack mode, w4 g128 asymmetric zeros, batch 1.  ONE STEP = one decode token
through the whole linear stack, driven through the q_layer MODULES exactly as a loaded model drives them
(`q_proj(h)`, `k_proj(h)`, `v_proj(h)`, `o_proj(q)`, `gate_proj(o)`, `up_proj(o)`, `down_proj(gate)` per layer; every
launch is fed by the previous one like in the model), replayed from a hipGraph on one stream.  The modules carry the sibling
groups the loader installs (q/k/v and gate/up -> one grouped launch each: 4 launches per layer; `--fused 0` gives the 7-launch
form) and decode from the library's native strip-major copy of their integers, built once on the device at first use
(qllm_repack_native).  Weights are synthetic (no network: random packed int4 words, random fp16 scales
sized to keep activations O(1)) and RESIDENT IN HBM before the timed region; 3.5 GB of weights per pass means nothing is
served from the 256 MB Infinity Cache.

value = decode tokens/s over all ranks (rank r runs an independent replica: batch elements are independent units,
no data-path collective -> "scaling": "weak").  `--tp N` instead runs the Llama-2-70B column/row-parallel layer stack
(BASELINE configs[4]) with one RCCL all-reduce per Megatron pair; see tp_leg().

Extra objects on the JSON line (a plain run carries `roofline` alone, with `traffic` null; the rest needs --full):
  roofline     dominant kernel = the decode matvec (one kernel function serves every launch of the step).
               achieved = algorithmic bytes per launch (packed weights + scales + zeros + x + y,
               3,369,484,288 B per token / launches) / average launch duration, the latter measured here with HIP events
               on the launch stream over the K timed steps (= event time / launches: inter-kernel gaps included).
               traffic = HBM bytes per launch from two rocprofv3 PMC passes (FETCH_SIZE, WRITE_SIZE; separate passes,
               FETCH doubled per MI355X_MICROARCH.md) that THIS run spawns on itself (`--pmc-child`, 8 layers, the same
               kernels); null if rocprofv3 is absent or without --full.
  sustained    the same graph replayed on after the K steps until the GPU has been busy --min-timed-s in all.
  cpu_baseline the reference's CPU torch formulation (oracle/ref_torch.py: shift/mask dequant + fp16 torch.matmul,
               bit-identical to the oracle) timed on this host's cores over one decoder layer (3 warm + 5 timed calls per
               shape, thread count picked by a short sweep and stated), extrapolated x32.
  extra        per-shape decode GB/s (+ the same layers and the whole stack at batch 64: the mid-batch panel kernel), the other
               launch forms, M=2048 prefill TFLOP/s (AWQ; act-order GPTQ = configs[2]), HQQ g64 M=16 (configs[3]) and the
               Llama-2-70B per-rank shard shapes of configs[4].
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HIDDEN, INTER, LAYERS, GROUP = 4096, 11008, 32, 128
HBM_PEAK_GBPS = 8000.0      # MI355X HBM3E spec (MI355X_MICROARCH.md)
HBM_COPY_GBPS = 6300.0      # ... and the measured float4-copy ceiling of the same guide (roofline.frac_of_achievable)
MFMA_PEAK_TFLOPS = 2500.0   # dense f16/bf16 MFMA peak (no sparsity)


def alg_bytes(K, N, M, g=GROUP, zeros="packed", act_order=False):
    G = (K + g - 1) // g
    z = G * N * 2 if zeros == "f16" else G * N // 2
    return K * N // 2 + G * N * 2 + z + (4 * K if act_order else 0) + 2 * M * K + 2 * M * N


def make_layer(cls, K, N, dev, gen, act_order=False, bits=4, group=GROUP, g_idx=None):
    layer = cls(bits, group, K, N, False, dtype=torch.float16)
    shape_w, shape_z, shape_s = layer.qweight.shape, layer.qzeros.shape, layer.scales.shape
    layer.qweight = torch.randint(-2 ** 31, 2 ** 31 - 1, shape_w, dtype=torch.int32, device=dev, generator=gen)
    if layer.qzeros.dtype.is_floating_point:  # HQQ: fp16 zero points
        layer.qzeros = (torch.rand(shape_z, device=dev, generator=gen) * (2 ** bits - 1)).to(torch.float16)
    else:
        layer.qzeros = torch.randint(-2 ** 31, 2 ** 31 - 1, shape_z, dtype=torch.int32, device=dev, generator=gen)
    # std(q - z) ~ 6.5 for independent uniform nibbles: scale so each linear roughly preserves magnitude
    base = 1.0 / (K ** 0.5 * 6.5 * (2 ** bits) / 16)
    layer.scales = ((torch.rand(shape_s, device=dev, generator=gen) * 0.4 + 0.8) * base).to(torch.float16)
    if act_order:  # (g_idx: the order shared with the layers fed by the same input, see Block)
        layer.g_idx = (layer.g_idx[torch.randperm(K)] if g_idx is None else g_idx).contiguous()
    return layer.to(dev)


class Block(torch.nn.Module):
    """One decoder layer's quantized linears under their Llama names (what swap_quantized_linears leaves in a model)."""

    def __init__(self, cls, dev, gen, act_order=False, hidden=HIDDEN, inter=INTER, kv=None, bits=4, group=GROUP):
        super().__init__()
        kv = hidden if kv is None else kv
        # act-order: GPTQ's permutation is argsort(diag(H)) of the layer INPUT's Hessian (qllm/quantization/gptq/gptq.py:168), so
        # q/k/v share one g_idx and gate/up another, as in a real checkpoint; o_proj and down_proj have their own
        def order(K):
            return (torch.arange(K, dtype=torch.int32) // group)[torch.randperm(K)] if act_order else None
        # bits: one width for the layer, or {module name: width} (mixed precision: quant_config_by_layer.json gives every linear its own)
        wb = (lambda name: bits[name]) if isinstance(bits, dict) else (lambda name: bits)
        mk = lambda name, K, N, gi=None: make_layer(cls, K, N, dev, gen, act_order, wb(name), group, gi)  # noqa: E731
        g_attn, g_mlp = order(hidden), order(hidden)
        self.q_proj = mk("q_proj", hidden, hidden, g_attn)
        self.k_proj = mk("k_proj", hidden, kv, g_attn)
        self.v_proj = mk("v_proj", hidden, kv, g_attn)
        self.o_proj = mk("o_proj", hidden, hidden, order(hidden))
        self.gate_proj = mk("gate_proj", hidden, inter, g_mlp)
        self.up_proj = mk("up_proj", hidden, inter, g_mlp)
        self.down_proj = mk("down_proj", inter, hidden, order(inter))

    def forward(self, h):
        q = self.q_proj(h)
        k = self.k_proj(h)  # noqa: F841  (k, v feed attention in the real model)
        v = self.v_proj(h)  # noqa: F841
        o = self.o_proj(q)
        gate = self.gate_proj(o)
        up = self.up_proj(o)  # noqa: F841
        return self.down_proj(gate)


class Stack(torch.nn.Module):
    """The quantized linears of the decoder stack, driven in model order through the module API."""

    def __init__(self, cls, n_layers, dev, seed, act_order=False, fused=True, bits=4, group=GROUP):
        super().__init__()
        from qllm_amd.modeling.q_layers import install_sibling_groups
        gen = torch.Generator(device=dev).manual_seed(seed)
        # bits: one width, or a function of the decoder layer's index returning a width or a {module name: width} dict
        per_layer = bits if callable(bits) else (lambda i: bits)
        self.blocks = torch.nn.ModuleList([Block(cls, dev, gen, act_order, bits=per_layer(i), group=group) for i in range(n_layers)])
        self.groups = install_sibling_groups(self, [cls]) if fused else 0
        # the loader's memory policy (modeling/base.load_quantized): one copy of every layer on the device, in the native layout
        from qllm_amd.modeling.base import release_reference_layouts
        release_reference_layouts(self)

    def set_fused(self, on: bool):
        for m in self.modules():
            g = getattr(m, "_siblings", None)
            if g is not None:
                g.enabled = on

    def forward(self, h):
        for b in self.blocks:
            h = b(h)
        return h


def bytes_per_token(n_layers=LAYERS, M=1):
    return n_layers * (4 * alg_bytes(HIDDEN, HIDDEN, M) + 2 * alg_bytes(HIDDEN, INTER, M) + alg_bytes(INTER, HIDDEN, M))


def flops_per_pass(n_layers, M):
    return n_layers * 2.0 * M * (4 * HIDDEN * HIDDEN + 3 * HIDDEN * INTER)


def capture(fn, warm=2):
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
    # (capturing executes nothing: `out` is graph-pool memory nobody has written yet -- one replay makes it the step's real output
    #  before any caller looks at it; round 5: a run after 11 minutes of other GPU work found non-finite garbage there)
    g.replay()
    torch.cuda.synchronize()
    return g, out


def time_events(fn, iters, warm=10):
    """ms per call over `iters` calls (HIP events on the current stream), after `warm` untimed calls: a leg that starts right after
    its stack was built sees the clock ramp for its first milliseconds (round 5, tools/rounds5/g22_warm.py: the first 20 replays of
    the configs[3] stack ran 1.5-3 % slower than the next 120) -- the headline leg has always had its --warmup steps."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters  # ms


def decode_step_fn(stack, h0):
    """One decode token through the stack's modules."""
    return lambda: stack(h0)


def cpu_baseline_leg(dev):
    """The reference's CPU torch formulation (oracle/ref_torch.py) on this host's cores, bounded sample: one decoder layer.
    AWQ has no CPU forward in the reference at all (WQLinear_GEMM.forward needs its CUDA engine), so the layer
    is timed in the GPTQ layout its integers repack to: same int4 count, same scales/zeros, same ops."""
    import numpy as np
    from oracle import ref_torch as T

    cores = os.cpu_count() or 1
    rng = np.random.default_rng(0)
    shapes = [(HIDDEN, HIDDEN)] * 4 + [(HIDDEN, INTER)] * 2 + [(INTER, HIDDEN)]
    layers = []
    for (K, N) in shapes:
        qw = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, size=(K // 8, N), dtype=np.int64).astype(np.int32))
        qz = torch.from_numpy(rng.integers(-2 ** 31, 2 ** 31 - 1, size=(K // GROUP, N // 8), dtype=np.int64).astype(np.int32))
        sc = torch.from_numpy(((rng.random((K // GROUP, N)) * 0.4 + 0.8) / (K ** 0.5 * 6.5)).astype(np.float16))
        layers.append((K, N, qw, qz, sc))
    xs = {K: torch.from_numpy(rng.standard_normal((1, K)).astype(np.float16)) for K in (HIDDEN, INTER)}

    def call(i):
        K, N, qw, qz, sc = layers[i]
        return T.forward_gptq_torch(xs[K], qw, sc, qz, GROUP, 4)

    # thread count: short sweep on the 4096x4096 shape (more threads than ~32 usually lose on these bandwidth-light ops)
    sweep = {}
    for t in sorted({1, 8, 16, 32, 64, cores} & set(range(1, cores + 1))):
        torch.set_num_threads(t)
        call(0)
        t0 = time.perf_counter()
        call(0)
        call(0)
        sweep[t] = (time.perf_counter() - t0) / 2
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    per_shape = []
    for i in (0, 4, 6):  # one of each shape: 3 warm + 5 timed, median
        for _ in range(3):
            call(i)
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            y = call(i)
            ts.append(time.perf_counter() - t0)
        per_shape.append(sorted(ts)[2])
    per_layer = 4 * per_shape[0] + 2 * per_shape[1] + per_shape[2]
    # parity of the GPU path against this very formulation, same tensors (north_star: <= 1e-2 relative)
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    K, N, qw, qz, sc = layers[6]
    gl = QuantLinearGPTQ(4, GROUP, K, N, False, dtype=torch.float16)
    gl.qweight, gl.qzeros, gl.scales = qw, qz, sc
    y_gpu = gl.to(dev)(xs[K].to(dev)).float().cpu()
    rel = float((y_gpu - y.float()).abs().max() / y.float().abs().max())
    return dict(value=round(1.0 / (per_layer * LAYERS), 4), unit="tokens/s", cores=best, kind="port",
                sample=f"1 of {LAYERS} decoder layers (7 w4 g128 linears, M=1; torch shift/mask dequant + fp16 torch.matmul, "
                       f"oracle/ref_torch.py), 3 warm + 5 timed calls per shape (median), extrapolated x{LAYERS}; "
                       f"torch threads={best} of {cores} host cores, chosen by a sweep "
                       f"{ {k: round(v * 1e3, 1) for k, v in sweep.items()} } ms per 4096x4096 call",
                ms_per_shape={"4096x4096": round(per_shape[0] * 1e3, 2), "4096x11008": round(per_shape[1] * 1e3, 2),
                              "11008x4096": round(per_shape[2] * 1e3, 2)},
                gpu_vs_cpu_rel_err_11008x4096=round(rel, 6))


LINEARS = (("q_proj", HIDDEN, HIDDEN), ("k_proj", HIDDEN, HIDDEN), ("v_proj", HIDDEN, HIDDEN), ("o_proj", HIDDEN, HIDDEN),
           ("gate_proj", HIDDEN, INTER), ("up_proj", HIDDEN, INTER), ("down_proj", INTER, HIDDEN))
# the two ways a mixed-precision recipe assigns widths (BASELINE configs[3] "mixed 3/4-bit layers"): by decoder layer, or by module kind
MIX_BY_LAYER = lambda i: 4 if i % 2 == 0 else 3  # noqa: E731
MIX_BY_MODULE = lambda i: {"q_proj": 3, "k_proj": 3, "v_proj": 4, "o_proj": 4, "gate_proj": 3, "up_proj": 3, "down_proj": 4}  # noqa: E731


def hqq_leg(dev, n_layers=LAYERS):
    """BASELINE configs[3]: HQQ g64 fp16 zeros, batch 16, 4-bit and 3-bit decoder layers (the reference mixes them per layer).
    A stack of the model's depth for each width (32 layers: one hipGraph per batch step, like the headline leg -- a four-layer
    graph, rounds 3-4, charged the replay boundary of a step to four layers instead of 32: ~1.5 us per layer), through the modules
    with the loader's sibling groups; the 7-launch form beside it.  Round 6: the same stack as ONE mixed model -- widths alternating
    by decoder layer (`hqq_mixed34_by_layer`), and by module kind (`hqq_mixed34_by_module`: q / k / gate / up at 3 bits, v / o / down
    at 4 -- q/k share a grouped launch, v runs alone: 5 launches per layer)."""
    extra = {}
    from qllm_amd.modeling.q_layers import QuantLinearHQQ
    x16 = torch.randn(16, HIDDEN, device=dev, dtype=torch.float16)
    for bits_sel, tag in ((4, "hqq_w4_g64_m16"), (3, "hqq_w3_g64_m16"), (MIX_BY_LAYER, "hqq_mixed34_by_layer_g64_m16"),
                          (MIX_BY_MODULE, "hqq_mixed34_by_module_g64_m16")):
        hs = Stack(QuantLinearHQQ, n_layers, dev, seed=7 + (bits_sel if isinstance(bits_sel, int) else 5), bits=bits_sel, group=64)
        # (only the packed words scale with the bit width: scales, fp16 zero points, x and y do not)
        nbytes = 0
        for i in range(n_layers):
            wb = bits_sel(i) if callable(bits_sel) else bits_sel
            for (name, K, N) in LINEARS:
                b = wb[name] if isinstance(wb, dict) else wb
                nbytes += alg_bytes(K, N, 16, 64, "f16") - K * N // 2 + K * N * b // 8
        nbytes /= n_layers   # per layer
        res = {}
        for fz in (True, False):
            hs.set_fused(fz)
            gh, _ = capture(lambda: hs(x16))
            ms = time_events(gh.replay, 20) / n_layers
            del gh
            res["grouped" if fz else "ungrouped"] = ms
        # (round 6) the same stack at batch 1: 64-wide groups ride the batch-1 kernel since round 6 (4 bits; 3-bit layers: the general strips)
        hs.set_fused(True)
        x1 = torch.randn(1, HIDDEN, device=dev, dtype=torch.float16)
        g1, _ = capture(lambda: hs(x1))
        res["batch1"] = time_events(g1.replay, 20) / n_layers
        del g1
        extra[tag] = {"ms_per_layer": round(res["grouped"], 4), "GBps": round(nbytes / res["grouped"] / 1e6, 1),
                      "ms_per_layer_batch1": round(res["batch1"], 4),
                      "frac_of_hbm_peak": round(nbytes / res["grouped"] / 1e6 / HBM_PEAK_GBPS, 4), "layers": n_layers,
                      "sibling_groups": hs.groups, "ms_per_layer_7_launches": round(res["ungrouped"], 4)}
        del hs
        torch.cuda.empty_cache()
    return extra


def pmc_traffic(args):
    """HBM bytes per launch of the decode kernel: two rocprofv3 PMC passes over a child run of this file."""
    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rocprof is None:
        return None, "rocprofv3 not found"
    per = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        d = tempfile.mkdtemp(prefix="qllm_pmc_", dir="/tmp")
        env = dict(os.environ, TMPDIR="/tmp")
        cmd = [rocprof, "--kernel-trace", "--pmc", ctr, "-d", d, "-o", "p", "--output-format", "csv", "--",
               sys.executable, os.path.abspath(__file__), "--pmc-child", "--steps", "2", "--warmup", "1", "--no-extra",
               "--fused", str(args.fused)]
        try:
            subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240, check=True)
            f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
            tot, n = 0.0, 0
            for r in csv.DictReader(open(f[0])):
                if r["Counter_Name"] != ctr:
                    continue
                if re.search(r"qllm::strip\d?_kernel", r["Kernel_Name"]):  # (strip1_kernel: the batch-1 kernel, round 5)
                    tot += float(r["Counter_Value"])
                    n += 1
            per[ctr] = tot / max(n, 1)
        except Exception as e:  # noqa: BLE001
            shutil.rmtree(d, ignore_errors=True)
            return None, f"rocprofv3 --pmc {ctr} pass failed: {type(e).__name__}"
        shutil.rmtree(d, ignore_errors=True)
    # FETCH_SIZE / WRITE_SIZE are in KB; FETCH counts 64 B per 128-B request on gfx950 for wide coalesced reads (x2)
    return int((2.0 * per["FETCH_SIZE"] + per["WRITE_SIZE"]) * 1024), (
        "this run: rocprofv3 --kernel-trace --pmc FETCH_SIZE / --pmc WRITE_SIZE (separate passes) over `bench.py --pmc-child` "
        "(8 layers, same kernels); bytes = (2 x FETCH_SIZE + WRITE_SIZE) x 1024, averaged over "
        "the decode-kernel dispatches")


def pmc_prefill_mfma_busy():
    """Matrix-pipe occupancy of the prefill kernel: one rocprofv3 PMC pass (SQ_VALU_MFMA_BUSY_CYCLES, GRBM_GUI_ACTIVE) over a child run
    of this file that launches the 256x128 prefill kernel on the three Llama-2-7B shapes at M = 2048.  busy = MFMA-busy cycles per
    SIMD / active cycles per XCD (SQ counters sum over the 1024 SIMDs, GRBM_GUI_ACTIVE over the 8 XCDs)."""
    rocprof = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if rocprof is None:
        return None, "rocprofv3 not found"
    d = tempfile.mkdtemp(prefix="qllm_pmc_", dir="/tmp")
    env = dict(os.environ, TMPDIR="/tmp")
    cmd = [rocprof, "--kernel-trace", "--pmc", "SQ_VALU_MFMA_BUSY_CYCLES", "GRBM_GUI_ACTIVE", "-d", d, "-o", "p", "--output-format", "csv", "--",
           sys.executable, os.path.abspath(__file__), "--pmc-child-prefill"]
    try:
        subprocess.run(cmd, cwd="/tmp", env=env, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=240, check=True)
        f = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
        busy, active, n = 0.0, 0.0, 0
        rows = {}
        for r in csv.DictReader(open(f[0])):
            if "qllm::gemm3_kernel" not in r["Kernel_Name"]:
                continue
            rows.setdefault(r["Dispatch_Id"], {})[r["Counter_Name"]] = float(r["Counter_Value"])
        for v in rows.values():
            if "SQ_VALU_MFMA_BUSY_CYCLES" in v and "GRBM_GUI_ACTIVE" in v and v["GRBM_GUI_ACTIVE"] > 0:
                busy += v["SQ_VALU_MFMA_BUSY_CYCLES"] / 1024.0
                active += v["GRBM_GUI_ACTIVE"] / 8.0
                n += 1
        shutil.rmtree(d, ignore_errors=True)
        if not n:
            return None, "no gemm3 dispatch in the counter pass"
        return round(busy / active, 4), ("this run: rocprofv3 --kernel-trace --pmc SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE over `bench.py "
                                         "--pmc-child-prefill` (%d dispatches of qllm::gemm3_kernel at M = 2048); busy cycles per SIMD / active cycles per XCD" % n)
    except Exception as e:  # noqa: BLE001
        shutil.rmtree(d, ignore_errors=True)
        return None, f"rocprofv3 MFMA-busy pass failed: {type(e).__name__}"


def pmc_child_prefill():
    """Target of pmc_prefill_mfma_busy: two prefill passes of one decoder layer's linears at M = 2048 (AWQ w4 g128 through the modules)."""
    dev = torch.device("cuda", 0)
    from qllm_amd.modeling.q_layers import WQLinear_GEMM
    ps = Stack(WQLinear_GEMM, 1, dev, seed=99)
    xp = torch.randn(2048, HIDDEN, device=dev, dtype=torch.float16)
    for _ in range(2):
        ps(xp)
    torch.cuda.synchronize()


def self_launch(n: int) -> int:
    """`bench.py --gpus N` started without a launcher: run the same command line under torch.distributed.run, one rank per GPU on
    this node (rendezvous on 127.0.0.1, a free port).  Rank 0 of the child job prints the ONE JSON line; its exit code is ours."""
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def stub_main(args, world, rank):
    """QLLM_BENCH_STUB=1 (tests/test_bench_contract_cpu.py): the launch / rendezvous / reduction / printing path of a multi-rank run
    on a GPU-less host -- gloo, a trivial CPU step -- so that the first multi-GPU lease is not the first execution of this code.
    The line it prints is marked as a stub and carries no measurement."""
    import torch.distributed as dist
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    if world > 1:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    x = torch.ones(64, 64)
    for _ in range(args.warmup):
        x = x @ x * 1e-2
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        x = x @ x * 1e-2
    if world > 1:
        dist.barrier()
    wall = time.perf_counter() - t0
    if world > 1:
        t = torch.tensor([wall], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall = float(t[0])
    result = {"metric": "decode_tokens_per_s_llama2_7b_w4a16_g128_linear_stack", "value": None, "unit": "tokens/s",
              "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(wall * 1e3 / args.steps, 4),
              "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f16",
              "data": "STUB (QLLM_BENCH_STUB=1: launch-path test on CPU, not a measurement)",
              "config": {"workload": "stub", "parallelism": f"replicas x{world}", "backend": "gloo" if world > 1 else None},
              "roofline": None, "cpu_baseline": None}
    if world > 1 and args.full:   # the same second leg as the real run: every rank enters it, rank 0 gets the record (watchdog included)
        from tools import tp_bench
        tp_leg_guarded(result, rank, lambda: tp_bench.stub_measure(args, world, rank), args.tp_timeout_s)
    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


def tp_leg_guarded(result, rank, leg, timeout_s):
    """`--gpus N` (N > 1), after the replica measurement: the tensor-parallel leg of BASELINE configs[4] (Llama-2-70B sharded over the
    run's N ranks, tools/tp_bench.py) -> result["extra"]["tp70b"].  The replica line must survive whatever that leg does on hardware
    it has never run on (round-5 verdict: "the first 8-GPU lease must not come back empty"): an exception is recorded in the object;
    a leg still running after `timeout_s` (a rank stuck in a collective) makes rank 0 print the line WITH the replica numbers and an
    error entry and every rank leave with os._exit(0) -- the stuck collective cannot be joined."""
    import threading
    done = threading.Event()

    def watchdog():
        if done.wait(timeout_s):
            return
        if rank == 0:
            result.setdefault("extra", {})["tp70b"] = {"error": f"timeout: the tensor-parallel leg was still running after {timeout_s} s; "
                                                                "the replica measurement above is unaffected"}
            print(json.dumps(result), flush=True)
        else:
            time.sleep(5.0)   # (rank 0 prints first: a launcher may tear the job down when the first rank leaves)
        os._exit(0)

    threading.Thread(target=watchdog, daemon=True).start()
    try:
        rec = leg()
        if rank == 0:
            result.setdefault("extra", {})["tp70b"] = rec
    except BaseException as e:  # noqa: BLE001  (SystemExit included: the line is printed by the caller either way)
        if rank == 0:
            result.setdefault("extra", {})["tp70b"] = {"error": f"{type(e).__name__}: {e}"}
    finally:
        done.set()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--fused", type=int, default=int(os.environ.get("QLLM_BENCH_FUSED", "1")),
                    help="1: sibling groups (q/k/v and gate/up as one grouped launch each: 4 launches per layer instead of 7)")
    ap.add_argument("--tp", type=int, default=0, help="Llama-2-70B tensor-parallel leg (BASELINE configs[4]); 1 = shard shapes on one GPU")
    ap.add_argument("--tp-layers", type=int, default=0, help="--tp: decoder layers of the stack (default: all 80)")
    ap.add_argument("--tp-timeout-s", type=float, default=420.0,
                    help="--full, --gpus N > 1: seconds the tensor-parallel leg behind extra.tp70b may take before the line is printed without it")
    ap.add_argument("--full", action="store_true",
                    help="after the headline measurement run every side measurement too: the sustained phase, the PMC passes, the "
                         "extra legs, cpu_baseline and (--gpus N > 1) the tensor-parallel leg; a plain run does none of them")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the last timed step's output (rank 0) to DIR/decode_out.npy as float32")
    ap.add_argument("--no-tp-leg", action="store_true", help="--full, --gpus N > 1: replicas only, no extra.tp70b")
    ap.add_argument("--no-extra", action="store_true", help="--full: skip the per-shape / prefill / CPU legs")
    ap.add_argument("--no-pmc", action="store_true", help="--full: skip the rocprofv3 PMC passes behind roofline.traffic")
    ap.add_argument("--pmc-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--pmc-child-prefill", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--min-timed-s", type=float, default=8.0,
                    help="--full: after the K timed steps keep replaying until the GPU has been busy this long (reported as "
                         "`sustained`; the headline numbers are those of exactly K steps)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.dump_outputs and args.tp:
        ap.error("--dump-outputs writes the decode step of the headline run; --tp runs another workload")
    if args.pmc_child_prefill:
        return pmc_child_prefill()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        sys.exit(self_launch(args.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch one rank per GPU (or run without a launcher: bench.py starts the ranks itself)")
    if os.environ.get("QLLM_BENCH_STUB") == "1":
        return stub_main(args, world, rank)
    # QLLM_BENCH_SHARE_GPU0=1 (tests/test_tp_collective_gpu.py on the 1-GPU box): every rank on cuda:0 and gloo over device tensors --
    # RCCL refuses two ranks on one device.  The line says so (config.backend "gloo"); never set by the driver.
    share_gpu0 = os.environ.get("QLLM_BENCH_SHARE_GPU0") == "1"
    if share_gpu0:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if share_gpu0:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from qllm_amd import _lib
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ, WQLinear_GEMM

    info = _lib.device_info(local_rank)  # raises unless gfx950 + library present: no fallback is ever benchmarked

    if args.tp:
        from tools import tp_bench
        return tp_bench.run(args, world, rank, dev, info)

    n_layers = 8 if args.pmc_child else LAYERS
    fused = bool(args.fused)
    stack = Stack(WQLinear_GEMM, n_layers, dev, seed=1234 + rank, fused=fused)
    h0 = torch.randn(1, HIDDEN, device=dev, dtype=torch.float16, generator=torch.Generator(device=dev).manual_seed(4321 + rank))
    graph, out = capture(decode_step_fn(stack, h0))
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all(), "synthetic stack diverged"
    launches = n_layers * (4 if fused else 7)
    if fused:
        assert stack.groups == 2 * n_layers

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        graph.replay()
    barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(args.steps):
        graph.replay()
    e1.record()
    barrier()
    wall = time.perf_counter() - t0
    ev_ms = e0.elapsed_time(e1)
    if world > 1:
        t = torch.tensor([wall, ev_ms], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        wall, ev_ms = float(t[0]), float(t[1])
    if args.pmc_child:
        return
    if args.dump_outputs and rank == 0:
        # `out` is the graph's output buffer: after the barrier it holds what the last timed replay computed
        import numpy as np
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "decode_out.npy"), out.float().cpu().numpy())
    # sustained phase: the K timed steps are tens of milliseconds; keep the same graph replaying until the GPU has been busy for
    # --min-timed-s in all, so that an outside observer (a utilisation sampler around this process) sees the work.  Reported
    # beside the headline numbers, which stay those of exactly K steps.
    sustained = None
    if args.full and args.min_timed_s > 0:
        n_more = max(0, int((args.min_timed_s - wall) / max(wall / args.steps, 1e-6)))
        if n_more:
            t1 = time.perf_counter()
            for _ in range(n_more):
                graph.replay()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t1
            sustained = {"steps": n_more, "seconds": round(dt, 3), "ms_per_step": round(dt * 1e3 / n_more, 4),
                         "tokens_per_s_per_rank": round(n_more / dt, 2)}

    ms_per_step = wall * 1e3 / args.steps
    tokens_per_s = world * args.steps / wall
    bpt = bytes_per_token()
    avg_launch_us = ev_ms * 1e3 / (args.steps * launches)
    achieved = (bpt / launches) / (avg_launch_us * 1e-6) / 1e9

    traffic, traffic_source = None, "skipped (no --full / --no-pmc / --no-extra / multi-GPU run: rank 0 of a 1-GPU --full run collects it)"
    if args.full and rank == 0 and world == 1 and not args.no_pmc and not args.no_extra:
        del graph
        traffic, traffic_source = pmc_traffic(args)

    result = {
        "metric": "decode_tokens_per_s_llama2_7b_w4a16_g128_linear_stack", "value": round(tokens_per_s, 2),
        "unit": "tokens/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f16", "data": "synthetic", "sustained": sustained,
        "config": {"workload": "llama2-7b-awq-w4-g128-decode-b1", "pack_mode": "GEMM", "bits": 4, "group_size": GROUP,
                   "layers": LAYERS, "linears_per_layer": 7, "batch": 1, "launches_per_step": launches,
                   "driven_through": "q_layer modules (sibling groups installed by the loader)", "grouped_qkv_gateup": fused,
                   "weight_layout": "native strip-major copy built on device at first use (qllm_repack_native)" if os.environ.get("QLLM_NATIVE_LAYOUT", "1") != "0" else "reference buffers in place",
                   "graph": True, "parallelism": f"replicas x{world}", "ranks_seen": world,
                   "backend": (dist.get_backend() if world > 1 else None),
                   "device": info["arch"], "compute_units": info["compute_units"]},
        "roofline": {"bound": "hbm", "kernel": "qllm::strip1_kernel (batch-1 decode matvec, csrc/strip1_kernel.hpp; serves every launch of the step)",
                     "achieved": round(achieved, 1), "peak": HBM_PEAK_GBPS, "unit": "GB/s",
                     "frac": round(achieved / HBM_PEAK_GBPS, 4), "achievable": HBM_COPY_GBPS,
                     "frac_of_achievable": round(achieved / HBM_COPY_GBPS, 4), "traffic": traffic, "traffic_source": traffic_source,
                     "bytes_per_launch": bpt // launches, "avg_launch_us": round(avg_launch_us, 3)},
    }

    if args.full and rank == 0 and world == 1 and not args.no_extra:
        extra = {}
        # per-shape decode bandwidth (32 distinct weight sets per shape => HBM resident, not cache resident), ordinary launches
        stack.set_fused(False)
        for name, key, (K, N) in (("attn_4096x4096", "q_proj", (HIDDEN, HIDDEN)), ("mlp_4096x11008", "gate_proj", (HIDDEN, INTER)),
                                  ("mlp_11008x4096", "down_proj", (INTER, HIDDEN))):
            x = torch.randn(1, K, device=dev, dtype=torch.float16)
            ls = [getattr(b, key) for b in stack.blocks]
            g, _ = capture(lambda: [l(x) for l in ls])
            ms = time_events(g.replay, 20) / len(ls)
            extra[f"decode_{name}"] = {"us": round(ms * 1e3, 2), "GBps": round(alg_bytes(K, N, 1) / ms / 1e6, 1)}
            # the same layers at batch 64 (between the BASELINE configs: continuous-batching decode; csrc/panel.hip since round 4)
            x64 = torch.randn(64, K, device=dev, dtype=torch.float16)
            g, _ = capture(lambda: [l(x64) for l in ls])
            ms = time_events(g.replay, 20) / len(ls)
            extra[f"batch64_{name}"] = {"us": round(ms * 1e3, 2), "GBps": round(alg_bytes(K, N, 64) / ms / 1e6, 1),
                                        "TFLOPs": round(2.0 * 64 * K * N / ms / 1e9, 1)}
        # the whole stack at batch 64 through the modules (sibling groups: q/k/v and gate/up one grouped panel launch each, round 4)
        try:
            stack.set_fused(fused)
            h64 = torch.randn(64, HIDDEN, device=dev, dtype=torch.float16) * 0.1
            gg, o64 = capture(decode_step_fn(stack, h64))
            ms = time_events(gg.replay, 10)
            del gg
            extra["batch64_stack"] = {"ms_per_step": round(ms, 4), "tokens_per_s": round(64e3 / ms, 1), "us_per_layer": round(ms * 1e3 / n_layers, 2),
                                      "TFLOPs": round(2.0 * 64 * (4 * HIDDEN * HIDDEN + 3 * HIDDEN * INTER) * n_layers / ms / 1e9, 1),
                                      "finite": bool(torch.isfinite(o64.float()).all())}
        except Exception as e:  # noqa: BLE001  (a side leg must not take the headline down with it)
            extra["batch64_stack"] = {"error": f"{type(e).__name__}: {e}"}
            torch.cuda.synchronize()
        # batches 2 and 4 (round 6: the batch-1 kernel's four-row forms -- the group's four A rows carry four batch rows)
        for mb in (2, 4):
            try:
                hb = torch.randn(mb, HIDDEN, device=dev, dtype=torch.float16) * 0.1
                gg, _ = capture(decode_step_fn(stack, hb))
                ms = time_events(gg.replay, 20)
                del gg
                extra[f"decode_stack_batch{mb}"] = {"ms_per_step": round(ms, 4), "tokens_per_s": round(mb * 1e3 / ms, 1), "us_per_layer": round(ms * 1e3 / n_layers, 2),
                                                    "GBps": round(bytes_per_token(n_layers, mb) / ms / 1e6, 1),
                                                    "frac_of_hbm_peak": round(bytes_per_token(n_layers, mb) / ms / 1e6 / HBM_PEAK_GBPS, 4)}
            except Exception as e:  # noqa: BLE001
                extra[f"decode_stack_batch{mb}"] = {"error": f"{type(e).__name__}: {e}"}
                torch.cuda.synchronize()
        # the other launch forms of the same step (all through the modules): 7 launches per layer; the reference buffers in place
        for tag, fz, native in (("ungrouped", False, True), ("fused_reference_layout_in_place", True, False)):
            stack.set_fused(fz)
            old = os.environ.get("QLLM_NATIVE_LAYOUT")
            if not native:
                os.environ["QLLM_NATIVE_LAYOUT"] = "0"
            try:
                gg, _ = capture(decode_step_fn(stack, h0))
                ms = time_events(gg.replay, 20)
                del gg
                extra["decode_stack_" + tag] = {"ms_per_token": round(ms, 4), "tokens_per_s": round(1e3 / ms, 1),
                                                "GBps": round(bpt / ms / 1e6, 1), "frac_of_hbm_peak": round(bpt / ms / 1e6 / HBM_PEAK_GBPS, 4)}
            except Exception as e:  # noqa: BLE001  (a side leg must not take the headline down with it)
                extra["decode_stack_" + tag] = {"error": f"{type(e).__name__}: {e}"}
                torch.cuda.synchronize()
            finally:
                if not native:
                    if old is None:
                        del os.environ["QLLM_NATIVE_LAYOUT"]
                    else:
                        os.environ["QLLM_NATIVE_LAYOUT"] = old
        stack.set_fused(fused)
        del stack
        torch.cuda.empty_cache()
        # prefill M=2048 (BASELINE configs[2]: GPTQ act-order) and AWQ, one layer's 7 linears x 4 layers
        # (awq_bf16: bf16 activations on the same kernel -- x converted to fp16 by a pre-pass, the result rounded to bf16, the
        #  arithmetic of the reference's shim, quant_linear_awq.py:29-36)
        # (round 6: awq_bf16 = NATIVE bf16 -- bf16 W, v_mfma_f32_32x32x16_bf16, no conversion pre-pass; awq_bf16_shim = the path until
        #  round 5, kept behind qllm_set_knob("QLLM_GEMM3_BF16", 0): x -> fp16 pre-pass, fp16 kernel, result rounded to bf16)
        from qllm_amd import ops as _ops
        for tag, cls, act, xdt in (("awq", WQLinear_GEMM, False, torch.float16), ("gptq_actorder", QuantLinearGPTQ, True, torch.float16),
                                   ("awq_bf16", WQLinear_GEMM, False, torch.bfloat16), ("awq_bf16_shim", WQLinear_GEMM, False, torch.bfloat16)):
            ps = Stack(cls, 4, dev, seed=99, act_order=act)
            xp = torch.randn(2048, HIDDEN, device=dev, dtype=xdt)
            if tag.endswith("_shim"):
                _ops.set_knob("QLLM_GEMM3_BF16", 0)
            try:
                gp, _ = capture(lambda: ps(xp))  # graph replay, like the headline leg: kernel time, not Python / allocator time
                ms = time_events(gp.replay, 10)
            finally:
                _ops.reset_knobs()
            del gp
            tf = flops_per_pass(4, 2048) / ms / 1e9
            extra[f"prefill_m2048_{tag}"] = {"ms_per_4_layers": round(ms, 3), "TFLOPs": round(tf, 1),
                                             "frac_of_mfma_peak": round(tf / MFMA_PEAK_TFLOPS, 4)}
            del ps
        # the other half of BASELINE's metric at top level: the prefill kernel against the dense MFMA peak (fp16 AWQ leg through the
        # modules = 4 launches of qllm::gemm3_kernel per layer since round 6: q/k/v and gate/up are one grouped grid each), with the matrix
        # pipe's occupancy from a live counter pass
        busy, busy_src = (None, "skipped (--no-pmc)") if args.no_pmc else pmc_prefill_mfma_busy()
        pf = extra["prefill_m2048_awq"]
        result["roofline_prefill"] = {
            "bound": "mfma", "kernel": "qllm::gemm3_kernel (256x128x64 tiles, 8 matrix + 4 dequant waves; csrc/gemm3.hip)",
            "workload": "llama2-7b-awq-w4-g128-prefill-m2048 (7 linears x 4 layers through the q_layer modules: 4 launches per layer, q/k/v and gate/up grouped; hipGraph replay)",
            "achieved": pf["TFLOPs"], "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": pf["frac_of_mfma_peak"],
            "gptq_actorder_frac": extra["prefill_m2048_gptq_actorder"]["frac_of_mfma_peak"],
            "awq_bf16_frac": extra["prefill_m2048_awq_bf16"]["frac_of_mfma_peak"],
            "awq_bf16_shim_frac": extra["prefill_m2048_awq_bf16_shim"]["frac_of_mfma_peak"],
            "mfma_busy_frac": busy, "mfma_busy_source": busy_src, "traffic": None}
        extra.update(hqq_leg(dev))
        try:  # BASELINE configs[4] on one GPU: the per-rank shard shapes of Llama-2-70B at TP = 8
            from tools import tp_bench
            extra.update(tp_bench.shard_shapes_leg(dev))
        except Exception as e:  # noqa: BLE001
            extra["tp_shard_error"] = f"{type(e).__name__}: {e}"
        result["extra"] = extra
        result["cpu_baseline"] = cpu_baseline_leg(dev)
    elif rank == 0:
        result["cpu_baseline"] = None

    if world > 1 and args.full and not args.no_tp_leg:
        # BASELINE configs[4] on the ranks of THIS run: Llama-2-70B column / row-parallel over `world` GPUs, one all-reduce per
        # Megatron pair (tools/tp_bench.measure) -- with --full the leg rides on the `--gpus N` line
        from tools import tp_bench
        try:
            del graph
        except NameError:
            pass
        del stack
        torch.cuda.empty_cache()
        tp_leg_guarded(result, rank, lambda: tp_bench.summary(tp_bench.measure(args, world, rank, dev, info)) if rank == 0
                       else tp_bench.measure(args, world, rank, dev, info), args.tp_timeout_s)

    if rank == 0:
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
