#!/usr/bin/env python3
"""A/B of the fused SwiGLU down-projection (qllm_linear_forward_swiglu, csrc/strip1_swiglu.hip) at Llama-2-7B's MLP shapes
(4096 / 11008), in ONE process on one box, the two versions alternating A, B, A, B:

  mlp    one decoder MLP through the modules, us per MLP --
           unfused: grouped gate/up launch, F.silu(g) * u, down_proj      (today's sequence: uninstall_fused_mlp)
           fused:   grouped gate/up launch, down_proj.forward_swiglu(g, u) (install_fused_mlp)
  down   the down_proj launch alone on fixed inputs, us per launch --
           plain:   down_proj(x) on a precomputed x = silu(g) * u
           swiglu:  ops.linear_forward_swiglu(w, g, u)                     (the prologue's cost, apart from the saved launch)

Each version is a hipGraph of --mlps MLPs with weights of their own (nothing stays in L2 from one to the next), warmed up on its own
and replayed for at least --seconds per timing; --repeats timings per version.  Prints a table and one JSON line per row.

  python tools/swiglu_bench.py [--mlps 32] [--seconds 0.5] [--repeats 3]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import (QuantLinearHQQ, WQLinear_GEMM, install_fused_mlp, install_sibling_groups,  # noqa: E402
                                        uninstall_fused_mlp)


class LlamaMLP(torch.nn.Module):
    """gate / up / down under their Llama names with transformers' forward (the class name is what install_fused_mlp looks for)."""

    def __init__(self, cls, dev, gen, bits, group):
        super().__init__()
        self.gate_proj = bench.make_layer(cls, bench.HIDDEN, bench.INTER, dev, gen, bits=bits, group=group)
        self.up_proj = bench.make_layer(cls, bench.HIDDEN, bench.INTER, dev, gen, bits=bits, group=group)
        self.down_proj = bench.make_layer(cls, bench.INTER, bench.HIDDEN, dev, gen, bits=bits, group=group)
        self.act_fn = torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class Chain(torch.nn.Module):
    def __init__(self, cls, n, dev, bits, group):
        super().__init__()
        gen = torch.Generator(device=dev).manual_seed(7)
        self.mlps = torch.nn.ModuleList([LlamaMLP(cls, dev, gen, bits, group) for _ in range(n)])
        self.groups = install_sibling_groups(self, [cls])
        from qllm_amd.modeling.base import release_reference_layouts
        release_reference_layouts(self)

    def forward(self, h):
        for m in self.mlps:
            h = m(h)
        return h


def timed(graph, per_replay_units, seconds):
    """us per unit over enough replays to last `seconds`."""
    ms = bench.time_events(graph.replay, 20, warm=10)
    iters = max(20, int(seconds * 1e3 / ms) + 1)
    return bench.time_events(graph.replay, iters, warm=5) * 1e3 / per_replay_units


def ab(graph_a, graph_b, units, seconds, repeats):
    a, b = [], []
    for _ in range(repeats):   # A, B, A, B
        a.append(timed(graph_a, units, seconds))
        b.append(timed(graph_b, units, seconds))
    return a, b


def row(name, what, la, lb, a, b):
    ma, mb = sum(a) / len(a), sum(b) / len(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    rec = dict(config=name, what=what, a=la, b=lb, a_us=[round(v, 3) for v in a], b_us=[round(v, 3) for v in b], a_mean_us=round(ma, 3),
               b_mean_us=round(mb, 3), saved_us=round(ma - mb, 3), spread_us=round(spread, 3), faster_beyond_spread=bool(ma - mb > spread))
    print(f"{name:14s} {what:5s} {la:8s} {ma:8.2f} us   {lb:7s} {mb:8.2f} us   saved {ma - mb:+6.2f} us   spread {spread:5.2f} us   "
          f"{'fused faster' if rec['faster_beyond_spread'] else 'within spread / slower'}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mlps", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  "
          f"torch {torch.__version__}  mlps per graph: {args.mlps}", flush=True)
    configs = (("awq w4 g128", WQLinear_GEMM, 4, 128, (1, 4)), ("hqq w4 g64", QuantLinearHQQ, 4, 64, (1,)), ("hqq w3 g64", QuantLinearHQQ, 3, 64, (1,)))
    for name, cls, bits, group, rows in configs:
        chain = Chain(cls, args.mlps, dev, bits, group)
        for m in rows:
            tag = f"{name} M={m}"
            h = torch.randn(m, bench.HIDDEN, device=dev, dtype=torch.float16)
            uninstall_fused_mlp(chain)
            g_unfused, y_unfused = bench.capture(lambda: chain(h))
            assert install_fused_mlp(chain, [cls]) == args.mlps
            for mlp in chain.mlps:   # (the modules' cutoff is the result of this measurement: every served row count is timed)
                mlp.down_proj.swiglu_max_m = 4
            g_fused, y_fused = bench.capture(lambda: chain(h))
            d0 = chain.mlps[0].down_proj
            print(f"{tag}: gate/up {chain.mlps[0].gate_proj._siblings.describe(m)}; down {ops.swiglu_describe(d0.native_descriptor(0), m)}; "
                  f"max |fused - unfused| after {args.mlps} MLPs: {float((y_fused.float() - y_unfused.float()).abs().max()):.3g} "
                  f"(max |y| {float(y_unfused.float().abs().max()):.3g})", flush=True)
            a, b = ab(g_unfused, g_fused, args.mlps, args.seconds, args.repeats)
            row(tag, "mlp", "unfused", "fused", a, b)
            # the down_proj launch alone, on fixed inputs
            gt = torch.randn(m, bench.INTER, device=dev, dtype=torch.float16)
            ut = torch.randn(m, bench.INTER, device=dev, dtype=torch.float16)
            xt = F.silu(gt) * ut
            downs = [mlp.down_proj for mlp in chain.mlps]
            descs = [d.native_descriptor(0) for d in downs]
            g_plain, _ = bench.capture(lambda: [ops.linear_forward(w, xt) for w in descs][-1])
            g_swi, _ = bench.capture(lambda: [ops.linear_forward_swiglu(w, gt, ut) for w in descs][-1])
            a, b = ab(g_plain, g_swi, args.mlps, args.seconds, args.repeats)
            row(tag, "down", "plain", "swiglu", a, b)
            del g_unfused, g_fused, g_plain, g_swi
        del chain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
