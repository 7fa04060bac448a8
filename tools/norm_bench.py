#!/usr/bin/env python3
"""A/B of RMSNorm in front of the q/k/v and gate/up launches at Llama-2-7B shapes (hidden 4096, intermediate 11008), in ONE process on
one box, the versions alternating A, B, C, A, B, C:

  seg    one norm -> sibling group segment at one row, us per segment, three ways --
           eager:   transformers' LlamaRMSNorm expression (about eight kernels), then ops.linear_forward_grouped   (today's sequence)
           kernel:  ops.rmsnorm (qllm_rmsnorm, csrc/rmsnorm.hip), then ops.linear_forward_grouped
           fused:   ops.linear_forward_rmsnorm (csrc/strip1_norm.hip): one launch
  group  the grouped launch alone, us per launch --
           plain:   ops.linear_forward_grouped on a precomputed xn
           fused:   ops.linear_forward_rmsnorm on x                                   (the prologue's cost, apart from the saved launches)
  norm   the norm alone at 1, 16 and 2048 rows, us per norm -- eager against ops.rmsnorm

Each version is a hipGraph of --links segments with weights of their own (nothing stays in L2 from one to the next), warmed up on its
own and replayed for at least --seconds per timing; --repeats timings per version.  Prints a table and one JSON line per row.

  python tools/norm_bench.py [--links 32] [--seconds 0.3] [--repeats 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import QuantLinearHQQ, WQLinear_GEMM  # noqa: E402

EPS = 1e-5


def eager_norm(x, w, eps=EPS):
    """LlamaRMSNorm.forward of transformers, expression for expression."""
    dt = x.dtype
    h = x.to(torch.float32)
    var = h.pow(2).mean(-1, keepdim=True)
    h = h * torch.rsqrt(var + eps)
    return w * h.to(dt)


def timed(graph, units, seconds):
    ms = bench.time_events(graph.replay, 20, warm=10)
    iters = max(20, int(seconds * 1e3 / ms) + 1)
    return bench.time_events(graph.replay, iters, warm=5) * 1e3 / units


def rounds(graphs, units, seconds, repeats):
    """us per unit of every graph, `repeats` times, the graphs alternating."""
    out = [[] for _ in graphs]
    for _ in range(repeats):
        for t, g in zip(out, graphs):
            t.append(timed(g, units, seconds))
    return out


def row(config, what, labels, times):
    means = [sum(t) / len(t) for t in times]
    spread = max(max(t) - min(t) for t in times)
    rec = dict(config=config, what=what, spread_us=round(spread, 3))
    for lab, t, m in zip(labels, times, means):
        rec[lab + "_us"] = [round(v, 3) for v in t]
        rec[lab + "_mean_us"] = round(m, 3)
    rec["last_beats_previous_beyond_spread"] = bool(means[-2] - means[-1] > spread)
    cells = "   ".join(f"{lab} {m:8.2f} us" for lab, m in zip(labels, means))
    print(f"{config:22s} {what:6s} {cells}   spread {spread:5.2f} us   {labels[-1]} - {labels[-2]}: {means[-1] - means[-2]:+6.2f} us", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  "
          f"torch {torch.__version__}  links per graph: {args.links}", flush=True)
    H, I = bench.HIDDEN, bench.INTER
    x = torch.randn(1, H, device=dev, dtype=torch.float16)
    configs = (("awq w4 g128", WQLinear_GEMM, 4, 128), ("hqq w4 g64", QuantLinearHQQ, 4, 64), ("hqq w3 g64", QuantLinearHQQ, 3, 64))
    for name, cls, bits, group in configs:
        for seg, widths in (("qkv", (H, H, H)), ("gate/up", (I, I))):
            gen = torch.Generator(device=dev).manual_seed(7)
            layers = [[bench.make_layer(cls, H, n, dev, gen, bits=bits, group=group) for n in widths] for _ in range(args.links)]
            descs = [[l.native_descriptor(0) for l in link] for link in layers]
            assert all(d is not None for link in descs for d in link)
            ws = [(torch.randn(H, device=dev) * 0.1 + 1).half() for _ in range(args.links)]
            tag = f"{name} {seg}"
            print(f"{tag}: {ops.rmsnorm_describe(descs[0], 1)}", flush=True)
            g_e, y_e = bench.capture(lambda: [ops.linear_forward_grouped(d, eager_norm(x, w)) for d, w in zip(descs, ws)][-1])
            g_k, y_k = bench.capture(lambda: [ops.linear_forward_grouped(d, ops.rmsnorm(x, w, EPS)) for d, w in zip(descs, ws)][-1])
            g_f, y_f = bench.capture(lambda: [ops.linear_forward_rmsnorm(d, x, w, EPS) for d, w in zip(descs, ws)][-1])
            print(f"{tag}: share of outputs that differ from eager's bits: kernel {float((y_k[0] != y_e[0]).float().mean()):.5f}  "
                  f"fused {float((y_f[0] != y_e[0]).float().mean()):.5f}", flush=True)
            row(tag, "seg", ("eager", "kernel", "fused"), rounds((g_e, g_k, g_f), args.links, args.seconds, args.repeats))
            xns = [ops.rmsnorm(x, w, EPS) for w in ws]
            g_p, _ = bench.capture(lambda: [ops.linear_forward_grouped(d, xn) for d, xn in zip(descs, xns)][-1])
            row(tag, "group", ("plain", "fused"), rounds((g_p, g_f), args.links, args.seconds, args.repeats))
            del g_e, g_k, g_f, g_p, layers, descs
            torch.cuda.empty_cache()
    ws = [(torch.randn(H, device=dev) * 0.1 + 1).half() for _ in range(args.links)]
    for m in (1, 16, 2048):
        xs = [torch.randn(m, H, device=dev, dtype=torch.float16) for _ in range(args.links)]
        g_e, _ = bench.capture(lambda: [eager_norm(xx, w) for xx, w in zip(xs, ws)][-1])
        g_k, _ = bench.capture(lambda: [ops.rmsnorm(xx, w, EPS) for xx, w in zip(xs, ws)][-1])
        row(f"K={H} M={m}", "norm", ("eager", "kernel"), rounds((g_e, g_k), args.links, args.seconds, args.repeats))


if __name__ == "__main__":
    main()
