#!/usr/bin/env python3
"""A few query rows behind a long cache: ops.attn_chunk (qllm_attn_chunk, csrc/attn_chunk.hip) against the two routes such a call has without
it, fp16, batch 1, in ONE process on one box, the three versions alternating A, B, C, A, B, C, A, B, C (the method of
tools/attn_prefill_bench.py): us per call under graph replay (a hipGraph of --links calls on tensors of their own), the cache update in
every column.

  columns   sdpa      transformers' sdpa_attention_forward behind the bool mask transformers builds
            prefill   ops.attn_prefill with causal = 1 plus that mask
            chunk     ops.attn_chunk with the same arguments
  kinds     static    StaticLayer.update into 4096 positions; mask [1, 1, S, 4096]; the kernels take the length from the layer's device counter
            dynamic   DynamicLayer.update's own statement (torch.cat onto the cached rows); mask [1, 1, S, cached + S]; the host length
  points    (q heads, kv heads, head_dim) = (32, 32, 128), (32, 8, 128), (28, 4, 128); S = 2, 4, 8, 16 behind 1024 and behind 4080 cached tokens;
            128 rows behind 1024 at (32, 32, 128)

A point "wins" when chunk's mean is below BOTH other means by more than the spread (the largest max - min of the three versions).  The
table at the end is what q_layers/fused_attention.py's SPLIT_MAX_ROWS is set from.  Prints one JSON line per row.

  python tools/attn_chunk_bench.py [--links 8] [--seconds 0.2] [--repeats 3]"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qllm_amd import ops  # noqa: E402
from attn_decode_bench import capture  # noqa: E402
from attn_prefill_bench import L_MAX, max_diff, padded_mask, static_layers  # noqa: E402
from swiglu_bench import timed  # noqa: E402

DEV = "cuda:0"
SHAPES = ((32, 32, 128), (32, 8, 128), (28, 4, 128))
POINTS = [(shape, s, behind) for shape in SHAPES for behind in (1024, 4080) for s in (2, 4, 8, 16)] + [((32, 32, 128), 128, 1024)]
results = []


def point(args, gen, shape, s, behind, kind):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    hq, hk, d = shape
    n, total = args.links, behind + s
    module = types.SimpleNamespace(num_key_value_groups=hq // hk, is_causal=True)
    r = lambda *sh: torch.randn(sh, device=DEV, dtype=torch.float16, generator=gen)
    # the projection outputs [1, S, H, D] viewed as [1, H, S, D], as the modules hand them over
    qs, ks, vs = ([r(1, s, h, d).transpose(1, 2) for _ in range(n)] for h in (hq, hk, hk))
    past_k, past_v = r(1, hk, behind, d), r(1, hk, behind, d)
    mask = padded_mask(s, behind, total if kind == "dynamic" else L_MAX)
    sets = []
    for _ in range(3):      # each version updates layers of its own
        layers, lens = static_layers(n, hk, d, gen) if kind == "static" else ([None] * n, None)
        for layer in layers if kind == "static" else ():
            layer.keys[:, :, :behind], layer.values[:, :, :behind] = past_k, past_v
        sets.append((layers, lens))

    def version(which, layers, lens):
        def run():
            if lens is not None:
                lens.fill_(behind)
            outs = []
            for layer, q, k, v in zip(layers, qs, ks, vs):
                kk, vv = (torch.cat([past_k, k], dim=-2), torch.cat([past_v, v], dim=-2)) if kind == "dynamic" else layer.update(k, v)
                length = total if kind == "dynamic" else layer.cumulative_length
                if which == "sdpa":
                    outs.append(sdpa_attention_forward(module, q, kk, vv, mask, dropout=0.0, scaling=d ** -0.5)[0])
                else:
                    outs.append((ops.attn_prefill if which == "prefill" else ops.attn_chunk)(q, kk, vv, length, mask=mask, scaling=d ** -0.5))
            return outs
        return run

    names = ("sdpa", "prefill", "chunk")
    graphs, outs = zip(*(capture(version(w, *sets[i])) for i, w in enumerate(names)))
    diffs = [max_diff(outs[0], outs[2]), max_diff(outs[1], outs[2])]
    us = {w: [] for w in names}
    for _ in range(args.repeats):
        for w, g in zip(names, graphs):
            us[w].append(timed(g, n, args.seconds))
    mean = {w: sum(v) / len(v) for w, v in us.items()}
    spread = max(max(v) - min(v) for v in us.values())
    rec = dict(shape=list(shape), rows=s, behind=behind, kind=kind, launch=ops.attn_chunk_describe(1, hq, hk, d, s, total if kind == "dynamic" else L_MAX),
               us={w: [round(x, 2) for x in v] for w, v in us.items()}, mean_us={w: round(x, 2) for w, x in mean.items()}, spread_us=round(spread, 2),
               wins=bool(min(mean["sdpa"], mean["prefill"]) - mean["chunk"] > spread), max_abs_diff_vs_sdpa=diffs[0], max_abs_diff_vs_prefill=diffs[1])
    results.append(rec)
    print(f"({hq},{hk},{d}) S={s:3d}+{behind:4d} {kind:7s}  sdpa {mean['sdpa']:8.2f}  prefill {mean['prefill']:8.2f}  chunk {mean['chunk']:8.2f} us   "
          f"x{mean['sdpa'] / mean['chunk']:5.2f} / x{mean['prefill'] / mean['chunk']:5.2f}   spread {spread:5.2f} us   "
          f"{'chunk wins' if rec['wins'] else 'within spread / slower'}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  torch {torch.__version__}  "
          f"links per graph: {args.links}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for shape, s, behind in POINTS:
        for kind in ("static", "dynamic"):
            point(args, gen, shape, s, behind, kind)
            torch.cuda.empty_cache()
    print("\nwhere ops.attn_chunk beats both other routes by more than the spread (rows: the largest S with no loss below it):")
    for kind in ("static", "dynamic"):
        for shape in SHAPES:
            for behind in (1024, 4080):
                rows = [r for r in results if r["kind"] == kind and r["shape"] == list(shape) and r["behind"] == behind]
                print(f"  {kind:7s} {tuple(shape)} behind {behind}: " + "  ".join(f"S={r['rows']} {'win' if r['wins'] else 'no'}" for r in rows))


if __name__ == "__main__":
    main()
