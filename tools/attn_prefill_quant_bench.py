#!/usr/bin/env python3
"""Prefill over a quantized static KV cache: the route `prefill="codes_all"` takes (ops.kv_quantize of the new rows, ops.attn_prefill_quant
over the codes in place; csrc/attn_prefill_quant.hip) against the route `prefill="codes"` takes for the same call (QuantStaticLayer.update
-- the same two kv_quantize launches plus two ops.kv_dequantize of every valid position into the scratch pair -- then ops.attn_prefill
over that pair), fp16, batch 1, in ONE process on one box, the two versions alternating A, B, A, B (the method of
tools/attn_chunk_bench.py): us per call under graph replay (a hipGraph of --links calls on layers of their own), the cache update in both
columns.

  points    (q heads, kv heads, head_dim) = (32, 8, 128), (32, 32, 128); 8 and 4 bits; a 2048-row prompt into an empty layer (no mask), a
            128-row chunk behind 1024 and behind 3968 cached tokens (the bool mask transformers builds, [1, 1, 128, 4096])

A point "wins" when the new route's mean is below the old one's by more than the spread (the larger max - min of the two versions' repeated
runs).  Prints one JSON line per row.

  python tools/attn_prefill_quant_bench.py [--links 4] [--seconds 0.3] [--repeats 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.quant_cache import QuantStaticLayer  # noqa: E402
from attn_decode_bench import capture  # noqa: E402
from attn_prefill_bench import L_MAX, max_diff, padded_mask  # noqa: E402
from swiglu_bench import timed  # noqa: E402

DEV = "cuda:0"
SHAPES = ((32, 8, 128), (32, 32, 128))
POINTS = ((2048, 0), (128, 1024), (128, 3968))


def layers_of(n, hk, d, bits, past_k, past_v):
    """n initialised QuantStaticLayers of L_MAX positions that hold the quantised `past` rows (one scratch pair, as in a cache)."""
    scratch, out = {}, []
    for _ in range(n):
        layer = QuantStaticLayer(max_cache_len=L_MAX, bits=bits, scratch=scratch)
        layer.lazy_initialization(past_k[:, :, :1], past_v[:, :, :1])
        if past_k.shape[2]:
            ops.kv_quantize(past_k, layer.k_codes, layer.k_params, bits, 0)
            ops.kv_quantize(past_v, layer.v_codes, layer.v_params, bits, 0)
        out.append(layer)
    return out


def point(args, gen, shape, bits, s, behind):
    hq, hk, d = shape
    n = args.links
    r = lambda *sh: torch.randn(sh, device=DEV, dtype=torch.float16, generator=gen)
    # the projection outputs [1, S, H, D] viewed as [1, H, S, D], as the modules hand them over
    qs, ks, vs = ([r(1, s, h, d).transpose(1, 2) for _ in range(n)] for h in (hq, hk, hk))
    past_k, past_v = r(1, hk, max(behind, 1), d)[:, :, :behind], r(1, hk, max(behind, 1), d)[:, :, :behind]
    mask = padded_mask(s, behind, L_MAX) if behind else None

    def version(which, layers):
        def run():
            outs = []
            for layer, q, k, v in zip(layers, qs, ks, vs):
                layer.cumulative_length.fill_(behind)      # (captured: every replay starts behind the same tokens)
                layer.cumulative_length_int = behind
                if which == "codes":
                    kk, vv = layer.update(k, v)
                    outs.append(ops.attn_prefill(q, kk, vv, layer.cumulative_length, mask=mask, scaling=d ** -0.5))
                else:
                    ops.kv_quantize(k, layer.k_codes, layer.k_params, bits, layer.cumulative_length)
                    ops.kv_quantize(v, layer.v_codes, layer.v_params, bits, layer.cumulative_length)
                    layer.advance(s)
                    outs.append(ops.attn_prefill_quant(q, layer.k_codes, layer.k_params, layer.v_codes, layer.v_params, bits, layer.cumulative_length,
                                                       mask=mask, scaling=d ** -0.5))
            return outs
        return run

    names = ("codes", "codes_all")
    graphs, outs = zip(*(capture(version(w, layers_of(n, hk, d, bits, past_k, past_v))) for w in names))
    diff = max_diff(outs[0], outs[1])
    us = {w: [] for w in names}
    for _ in range(args.repeats):
        for w, g in zip(names, graphs):
            us[w].append(timed(g, n, args.seconds))
    mean = {w: sum(v) / len(v) for w, v in us.items()}
    spread = {w: max(v) - min(v) for w, v in us.items()}
    rec = dict(shape=list(shape), bits=bits, rows=s, behind=behind, launch=ops.attn_prefill_quant_describe(1, hq, hk, d, bits, s, L_MAX),
               us={w: [round(x, 2) for x in v] for w, v in us.items()}, mean_us={w: round(x, 2) for w, x in mean.items()},
               spread_us={w: round(x, 2) for w, x in spread.items()}, wins=bool(mean["codes"] - mean["codes_all"] > max(spread.values())),
               max_abs_diff=diff)
    print(f"({hq},{hk},{d}) bits={bits} S={s:4d}+{behind:4d}  codes {mean['codes']:9.2f}  codes_all {mean['codes_all']:9.2f} us   "
          f"x{mean['codes'] / mean['codes_all']:5.2f}   spread {spread['codes']:6.2f} / {spread['codes_all']:6.2f} us   "
          f"{'codes_all wins' if rec['wins'] else 'within spread / slower'}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  torch {torch.__version__}  "
          f"links per graph: {args.links}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(0)
    for shape in SHAPES:
        for bits in (8, 4):
            for s, behind in POINTS:
                point(args, gen, shape, bits, s, behind)
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
