#!/usr/bin/env python3
"""The routed experts of one sparse MoE block at decode, fp16, two ways in ONE process, alternating A, B, A, B: us per block under graph
replay (a hipGraph of --links blocks, each link with routing of its own so that consecutive links read different experts).

  loop    the modules' loop route with the routing ALREADY ON THE HOST (generous to the loop: the real one synchronises per layer and cannot
          be captured): per hit expert ops.linear_forward x 3 on the expert's slice of the stacks, silu * up, the weight, index_add_
  fused   ops.moe_gate_up + ops.moe_down (csrc/moe_decode.hip), each launch also on its own

  points  Mixtral-8x7B (E, top_k, H, I) = (8, 2, 4096, 14336) and Qwen3-30B-A3B (128, 8, 2048, 768), T = 1 and 4; the fused times also as a
          share of the 6.3 TB/s copy ceiling over the algorithmic bytes: the packed words, scales and zero points of the T * top_k slots

  python tools/moe_decode_bench.py [--links 4] [--seconds 0.3] [--repeats 3] [--tokens 1 4]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qllm_amd import ops  # noqa: E402
from attn_decode_bench import capture  # noqa: E402
from swiglu_bench import timed  # noqa: E402

DEV = "cuda:0"
POINTS = (("mixtral-8x7b", 8, 2, 4096, 14336), ("qwen3-30b-a3b", 128, 8, 2048, 768))
COPY_CEILING = 6.3e12   # bytes / s


def stack(e, k, n, gen):
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (e, n // 16, k // 8, 16), device=DEV, dtype=torch.int32, generator=gen)
    sc = (torch.rand(e, n // 16, k // 128, 16, device=DEV, generator=gen) * 0.01 + 0.002).half()
    qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (e, n // 16, k // 128, 2), device=DEV, dtype=torch.int32, generator=gen)
    return qw, sc, qz


def descriptors(st, k, n):
    return [ops.QllmWeight(st[0][e].data_ptr(), st[1][e].data_ptr(), st[2][e].data_ptr(), None, None, k, n, 128, 4, ops.LAYOUTS["NATIVE"], 0) for e in range(st[0].shape[0])]


def point(args, gen, name, e, top_k, h, i, t):
    gate, up, down = stack(e, h, i, gen), stack(e, h, i, gen), stack(e, i, h, gen)
    dg, du, dd = descriptors(gate, h, i), descriptors(up, h, i), descriptors(down, i, h)
    n = args.links
    xs = [torch.randn(t, h, device=DEV, dtype=torch.float16, generator=gen) for _ in range(n)]
    ids = [torch.stack([torch.randperm(e, device=DEV, generator=gen)[:top_k] for _ in range(t)]) for _ in range(n)]
    wts = [torch.softmax(torch.randn(t, top_k, device=DEV, generator=gen), -1) for _ in range(n)]
    host = [[(ex, *torch.where(idl.cpu() == ex)) for ex in sorted(set(idl.flatten().tolist()))] for idl in ids]   # (expert, tokens, slots)
    host = [[(ex, tok.to(DEV), pos.to(DEV)) for ex, tok, pos in link] for link in host]
    hs = [ops.moe_gate_up(x, idl, gate, up) for x, idl in zip(xs, ids)]

    def loop():
        outs = []
        for x, w, link in zip(xs, wts, host):
            y = torch.zeros_like(x)
            for ex, tok, pos in link:
                cur = x[tok]
                cur = ops.linear_forward(dd[ex], torch.nn.functional.silu(ops.linear_forward(dg[ex], cur)) * ops.linear_forward(du[ex], cur))
                y.index_add_(0, tok, (cur * w[tok, pos, None]).to(y.dtype))
            outs.append(y)
        return outs

    def gate_up():
        return [ops.moe_gate_up(x, idl, gate, up) for x, idl in zip(xs, ids)]

    def down_only():
        return [ops.moe_down(hh, idl, w, down) for hh, idl, w in zip(hs, ids, wts)]

    def fused():
        return [ops.moe_down(ops.moe_gate_up(x, idl, gate, up), idl, w, down) for x, idl, w in zip(xs, ids, wts)]

    names = ("loop", "gate_up", "down", "fused")
    with torch.no_grad():
        graphs, outs = zip(*(capture(f) for f in (loop, gate_up, down_only, fused)))
    diff = max((a.float() - b.float()).abs().max().item() for a, b in zip(outs[0], outs[3]))
    us = {w: [] for w in names}
    for _ in range(args.repeats):
        for w, g in zip(names, graphs):
            us[w].append(timed(g, n, args.seconds))
    mean = {w: sum(v) / len(v) for w, v in us.items()}
    spread = {w: max(v) - min(v) for w, v in us.items()}
    per_w = lambda k, nn: k * nn // 2 + (k // 128) * nn * 2 + (k // 128) * nn // 2   # noqa: E731  words, scales, zero points of one layer
    nbytes = dict(gate_up=t * top_k * 2 * per_w(h, i), down=t * top_k * per_w(i, h))
    nbytes["fused"] = nbytes["gate_up"] + nbytes["down"]
    share = {w: round(nbytes[w] / COPY_CEILING / (mean[w] * 1e-6), 3) for w in nbytes}
    rec = dict(model=name, E=e, top_k=top_k, H=h, I=i, T=t, describe=ops.moe_describe(t, top_k, e, h, i), mean_us={w: round(v, 2) for w, v in mean.items()},
               spread_us={w: round(v, 2) for w, v in spread.items()}, bytes=nbytes, share_of_copy_ceiling=share,
               fused_wins=bool(mean["loop"] - mean["fused"] > max(spread["loop"], spread["fused"])), max_abs_diff_to_loop=diff)
    print(f"{name:14s} T={t}  loop {mean['loop']:8.2f} ({spread['loop']:5.2f})  gate_up {mean['gate_up']:7.2f}  down {mean['down']:7.2f}  fused {mean['fused']:7.2f} "
          f"({spread['fused']:5.2f}) us   x{mean['loop'] / mean['fused']:5.2f}   ceiling: gate_up {share['gate_up']:.2f} down {share['down']:.2f} pair {share['fused']:.2f}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--tokens", type=int, nargs="+", default=[1, 4])
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  torch {torch.__version__}  "
          f"links per graph: {args.links}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for name, e, top_k, h, i in POINTS:
        for t in args.tokens:
            point(args, gen, name, e, top_k, h, i, t)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
