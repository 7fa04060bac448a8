#!/usr/bin/env python3
"""The routed experts of one sparse MoE block above four tokens, fp16, two ways in ONE process, alternating A, B, A, B: us per block.

  loop    QuantExperts.forward_loop's steps on the experts' slices of the same stacks: one_hot, nonzero (the host synchronisation the
          loop has in every layer), per hit expert ops.linear_forward x 3, silu * up, the weight, index_add_.  It cannot be captured.
  fused   ops.moe_route + ops.moe_prefill_gate_up + ops.moe_prefill_down (csrc/moe_prefill.hip), also under graph replay

Both are timed as plain launches with a device synchronise per block inside the timed window (the loop has no other form); the fused
route's graph replay is reported next to it.  Ratios are loop / fused of the plain times; the spread is max - min over the repeats.

  points  Mixtral-8x7B (E, top_k, H, I) = (8, 2, 4096, 14336) and Qwen3-30B-A3B (128, 8, 2048, 768), T = 8 16 64 512 2048, uniform random
          routing; Mixtral also with every token on experts 0 and 1.  The fused time also as a share of the 6.3 TB/s copy ceiling over
          the packed bytes of the hit experts read ONCE (the algorithmic bytes; a row tile re-reads its expert's panel through L2).

  python tools/moe_prefill_bench.py [--seconds 0.5] [--repeats 3] [--tokens 8 16 64 512 2048]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qllm_amd import ops  # noqa: E402
from moe_decode_bench import COPY_CEILING, DEV, POINTS, descriptors, stack  # noqa: E402


def timed_sync(fn, seconds):
    """us per call, each call followed by a device synchronise, over at least `seconds`."""
    fn(), torch.cuda.synchronize()
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds or n < 3:
        fn()
        torch.cuda.synchronize()
        n += 1
    return (time.perf_counter() - t0) / n * 1e6


def point(args, gen, name, e, top_k, h, i, t, routing, st):
    gate, up, down, dg, du, dd = st
    x = torch.randn(t, h, device=DEV, dtype=torch.float16, generator=gen)
    if routing == "two":
        ids = torch.arange(top_k, device=DEV).repeat(t, 1).contiguous()
    else:
        ids = torch.stack([torch.randperm(e, device=DEV, generator=gen)[:top_k] for _ in range(t)])
    wts = torch.softmax(torch.randn(t, top_k, device=DEV, generator=gen), -1)
    ws = torch.empty(ops.moe_prefill_workspace_bytes(t, top_k, e, h, i), dtype=torch.uint8, device=DEV)

    def loop():
        y = torch.zeros_like(x)
        mask = torch.nn.functional.one_hot(ids, num_classes=e + 1).permute(2, 1, 0)
        for idx in torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero():
            ex = int(idx[0])
            pos, tok = torch.where(mask[ex])
            cur = x[tok]
            cur = ops.linear_forward(dd[ex], torch.nn.functional.silu(ops.linear_forward(dg[ex], cur)) * ops.linear_forward(du[ex], cur))
            y.index_add_(0, tok, (cur * wts[tok, pos, None]).to(y.dtype))
        return y

    def fused():
        route = ops.moe_route(ids, e, workspace=ws)
        return ops.moe_prefill_down(ops.moe_prefill_gate_up(x, ids, route, gate, up), ids, wts, route, down)

    with torch.no_grad():
        y_loop, y_fused = loop(), fused()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            fused()
        us = dict(loop=[], fused=[], fused_graph=[])
        for _ in range(args.repeats):
            us["loop"].append(timed_sync(loop, args.seconds))
            us["fused"].append(timed_sync(fused, args.seconds))
            us["fused_graph"].append(timed_sync(graph.replay, args.seconds))
    diff = (y_loop.float() - y_fused.float()).abs().max().item()
    mean = {w: sum(v) / len(v) for w, v in us.items()}
    spread = {w: max(v) - min(v) for w, v in us.items()}
    per_w = lambda k, nn: k * nn // 2 + (k // 128) * nn * 2 + (k // 128) * nn // 2   # noqa: E731  words, scales, zero points of one layer
    hit = len(set(ids.flatten().tolist()))
    nbytes = hit * 3 * per_w(h, i)
    tie = abs(mean["loop"] - mean["fused"]) <= max(spread["loop"], spread["fused"])
    rec = dict(model=name, routing=routing, E=e, top_k=top_k, H=h, I=i, T=t, describe=ops.moe_prefill_describe(t, top_k, e, h, i),
               mean_us={w: round(v, 2) for w, v in mean.items()}, spread_us={w: round(v, 2) for w, v in spread.items()}, hit_experts=hit, weight_bytes=nbytes,
               share_of_copy_ceiling=round(nbytes / COPY_CEILING / (mean["fused_graph"] * 1e-6), 3), ratio=round(mean["loop"] / mean["fused"], 3),
               verdict="tie" if tie else ("win" if mean["loop"] > mean["fused"] else "LOSS"), max_abs_diff_to_loop=diff)
    print(f"{name:14s} {routing:7s} T={t:5d}  loop {mean['loop']:10.1f} ({spread['loop']:7.1f})  fused {mean['fused']:9.1f} ({spread['fused']:6.1f})  graph "
          f"{mean['fused_graph']:9.1f} us   x{rec['ratio']:6.2f} {rec['verdict']:4s}  ceiling {rec['share_of_copy_ceiling']:.3f}  diff {diff:.2e}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, nargs="+", default=[8, 16, 64, 512, 2048])
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  torch {torch.__version__}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name, e, top_k, h, i in POINTS:
        gate, up, down = stack(e, h, i, gen), stack(e, h, i, gen), stack(e, i, h, gen)
        st = (gate, up, down, descriptors(gate, h, i), descriptors(up, h, i), descriptors(down, i, h))
        for routing in ("uniform", "two") if e == 8 else ("uniform",):
            for t in args.tokens:
                point(args, gen, name, e, top_k, h, i, t, routing, st)
        del st, gate, up, down
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
