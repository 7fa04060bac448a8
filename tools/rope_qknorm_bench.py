#!/usr/bin/env python3
"""Qwen3's segment between the q/k/v launch and the attention core -- q_norm, k_norm, apply_rotary_pos_emb -- three ways, fp16, batch 1, in
ONE process on one box, the versions alternating A, B, C, A, B, C (the method of tools/attn_prefill_quant_bench.py): us per call under
graph replay (a hipGraph of --links calls on tensors of their own).

  eager     transformers' Qwen3RMSNorm x 2 and apply_rotary_pos_emb: some 26 elementwise kernels
  composed  ops.rmsnorm x 2 + ops.rope: three kernels (what the library had)
  kernel    ops.rope_qknorm: one (csrc/rope_qknorm.hip)

  points    (q heads, kv heads, head_dim) = (32, 8, 128), (40, 8, 128), (64, 8, 128): Qwen3-8B / 14B / 32B; 1 row (a decode step) and 2048
            rows (a prefill), where the kernel's time is also given as a share of the 6.3 TB/s copy ceiling over the bytes the
            expression needs: q and k read and written once, cos and sin read once

The kernel "wins" over a version when its mean is below that version's by more than the spread (the larger max - min of the two versions'
repeated runs).  Prints one JSON line per row.

  python tools/rope_qknorm_bench.py [--links 8] [--seconds 0.3] [--repeats 3]"""
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
SHAPES = ((32, 8, 128), (40, 8, 128), (64, 8, 128))
ROWS = (1, 2048)
EPS = 1e-6
COPY_CEILING = 6.3e12   # bytes / s


def point(args, gen, shape, rows):
    from transformers.models.qwen3.modeling_qwen3 import Qwen3RMSNorm, apply_rotary_pos_emb
    hq, hk, d = shape
    n = args.links
    r = lambda *sh: torch.randn(sh, device=DEV, dtype=torch.float16, generator=gen)
    # the projection outputs [1, S, H, D], as the modules' .view(hidden_shape) hands them over
    qs, ks = [r(1, rows, hq, d) for _ in range(n)], [r(1, rows, hk, d) for _ in range(n)]
    ang = torch.rand(1, rows, d // 2, device=DEV, generator=gen) * 6.2832
    cos, sin = torch.cat((ang, ang), -1).cos().half(), torch.cat((ang, ang), -1).sin().half()
    norms = [Qwen3RMSNorm(d, eps=EPS).to(DEV).half() for _ in range(2)]
    for m in norms:
        m.weight.data.uniform_(0.5, 1.5, generator=gen)
    wq, wk = (m.weight.detach() for m in norms)

    def eager():
        return [apply_rotary_pos_emb(norms[0](q).transpose(1, 2), norms[1](k).transpose(1, 2), cos, sin) for q, k in zip(qs, ks)]

    def composed():
        return [ops.rope(ops.rmsnorm(q, wq, EPS).transpose(1, 2), ops.rmsnorm(k, wk, EPS).transpose(1, 2), cos, sin) for q, k in zip(qs, ks)]

    def kernel():
        return [ops.rope_qknorm(q.transpose(1, 2), k.transpose(1, 2), wq, wk, EPS, cos, sin) for q, k in zip(qs, ks)]

    names = ("eager", "composed", "kernel")
    with torch.no_grad():
        graphs, outs = zip(*(capture(f) for f in (eager, composed, kernel)))
    same_bits = all(torch.equal(a, b) for x, y in zip(outs[1], outs[2]) for a, b in zip(x, y))
    diff = max((a.float() - b.float()).abs().max().item() for x, y in zip(outs[0], outs[2]) for a, b in zip(x, y))
    us = {w: [] for w in names}
    for _ in range(args.repeats):
        for w, g in zip(names, graphs):
            us[w].append(timed(g, n, args.seconds))
    mean = {w: sum(v) / len(v) for w, v in us.items()}
    spread = {w: max(v) - min(v) for w, v in us.items()}
    nbytes = rows * d * 2 * (2 * (hq + hk) + 2)
    rec = dict(shape=list(shape), rows=rows, us={w: [round(x, 3) for x in v] for w, v in us.items()}, mean_us={w: round(x, 3) for w, x in mean.items()},
               spread_us={w: round(x, 3) for w, x in spread.items()},
               wins={w: bool(mean[w] - mean["kernel"] > max(spread[w], spread["kernel"])) for w in names[:2]},
               kernel_equals_composed_bits=same_bits, max_abs_diff_to_eager=diff)
    tail = ""
    if rows > 1:
        rec["bytes"] = nbytes
        rec["share_of_copy_ceiling"] = round(nbytes / COPY_CEILING / (mean["kernel"] * 1e-6), 3)
        tail = f"   {nbytes / 1e6:6.1f} MB: {100 * rec['share_of_copy_ceiling']:4.1f}% of 6.3 TB/s"
    print(f"({hq},{hk},{d}) rows={rows:4d}  eager {mean['eager']:8.2f} (spread {spread['eager']:5.2f})  composed {mean['composed']:7.2f} ({spread['composed']:5.2f})  "
          f"kernel {mean['kernel']:7.2f} ({spread['kernel']:5.2f}) us   x{mean['eager'] / mean['kernel']:5.2f} / x{mean['composed'] / mean['kernel']:4.2f}   "
          f"bits == composed: {same_bits}{tail}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  torch {torch.__version__}  "
          f"links per graph: {args.links}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for shape in SHAPES:
        for rows in ROWS:
            point(args, gen, shape, rows)
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
