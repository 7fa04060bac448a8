#!/usr/bin/env python3
"""Prefill attention over the KV cache as one kernel (qllm_attn_prefill, csrc/attn_prefill.hip; ops.attn_prefill) against what transformers
runs there, fp16, in ONE process on one box, the two versions alternating A, B, A, B, A, B (the method of tools/attn_decode_bench.py):

  op      (q heads, kv heads, head_dim) = (32, 32, 128), (32, 8, 128), (28, 4, 128), batch 1, S = 16, 128, 512, 1024, 2048 query rows, us per call
          under graph replay (a hipGraph of --links calls on tensors of their own; fewer links at large S).  Both columns include the cache
          update.  Four eager baselines, each against the kernel on the same tensors:
            (a) dynamic, no mask   DynamicLayer.update's own statement on an empty layer (torch.cat of the empty K / V and the new rows), then
                                   transformers' sdpa_attention_forward with mask None (torch's is_causal)  |  the kernel with the host length
            (b) static, no mask    StaticLayer.update (arange, add, add_, two index_copy_) into 4096 positions, then sdpa with mask None over
                                   all 4096 positions  |  the kernel with the length read from the layer's device counter
            (c) static, padded     the same update, then sdpa behind the bool mask [1, 1, S, 4096] of a prompt left-padded by 3  |  the
                                   kernel with causal = 1 plus that mask; and the same prompt on the dynamic layer (mask [1, 1, S, S])
            (d) chunk              128 rows behind 1024 cached tokens behind the bool mask transformers builds: dynamic (torch.cat onto the
                                   1024 rows, mask [1, 1, 128, 1152]) and static (mask [1, 1, 128, 4096])
          Beside the times: the causal flops 4 D Hq x (visible (row, key) pairs), the kernel's TFLOP/s and its share of the 2.5 PFLOP/s dense
          fp16 peak, and the maximum absolute difference between the two versions' outputs.
  layer   one Llama-2-7B-shaped decoder layer (AWQ 4-bit linears, 128-wide groups, sdpa) at S = 2048 with fuse_mlp, fuse_norm, fuse_residual
          and fuse_rope installed, a StaticCache of 4096 positions and the padded mask of (c), without and with the prefill core.

  --window W   instead of the points above, the sliding layers of a Mistral-shaped config with that window, (32, 8, 128) and (32, 32, 128):
          first prompts of 128, 512, W / 2, W and 2 W rows and a 128-row chunk behind a full window, on a DynamicSlidingWindowLayer (its update's own
          statements: torch.cat of what it kept and the new rows) and on a StaticSlidingWindowLayer of W positions (its update), behind the
          mask transformers builds there: none for the prompts below W on the dynamic layer (and those prompts left-padded by 3 as second
          points), the causal band [1, 1, S, L] otherwise  |  the same update, then ops.attn_prefill(window=W) with the same mask and the
          length the modules hand over.  The table at the end is what the two sliding kinds of PREFILL_ROUTES are set from.

A point "wins" when the kernel's mean is below eager's by more than the spread (the larger of the two versions' max - min).  The table at the
end is what q_layers/fused_attention.py's PREFILL_ROUTES is set from.  Prints one JSON line per row.

  python tools/attn_prefill_bench.py [--links 8] [--seconds 0.15] [--repeats 3] [--no-layer] [--window W]"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qllm_amd import ops  # noqa: E402
from attn_decode_bench import capture  # noqa: E402
from swiglu_bench import ab  # noqa: E402

DEV = "cuda:0"
L_MAX = 4096
PEAK_TFLOPS = 2500.0
PAD = 3
SHAPES = ((32, 32, 128), (32, 8, 128), (28, 4, 128))
ROWS = (16, 128, 512, 1024, 2048)
CHUNK, BEHIND = 128, 1024
results = []


def report(tag, what, shape, s, pairs, a, b, diff):
    hq, hk, d = shape
    ma, mb = sum(a) / len(a), sum(b) / len(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    flops = 4.0 * d * hq * pairs
    tf = flops / mb / 1e6
    rec = dict(config=tag, what=what, shape=list(shape), rows=s, eager_us=[round(v, 2) for v in a], kernel_us=[round(v, 2) for v in b], eager_mean_us=round(ma, 2),
               kernel_mean_us=round(mb, 2), spread_us=round(spread, 2), wins=bool(ma - mb > spread), causal_gflop=round(flops / 1e9, 3), kernel_tflops=round(tf, 1),
               share_of_peak=round(tf / PEAK_TFLOPS, 4), max_abs_diff=diff)
    results.append(rec)
    print(f"{tag:22s} {what:16s} eager {ma:9.2f} us   kernel {mb:9.2f} us   x{ma / mb:5.2f}   spread {spread:6.2f} us   {tf:7.1f} TFLOP/s "
          f"({100 * tf / PEAK_TFLOPS:5.2f} % of peak)   diff {diff:.2e}   {'kernel wins' if rec['wins'] else 'within spread / slower'}", flush=True)
    print("JSON " + json.dumps(rec), flush=True)


def max_diff(ya, yb):
    assert all(bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all()) for a, b in zip(ya, yb))
    diff = max((a.float() - b.float()).abs().max().item() for a, b in zip(ya, yb))
    assert diff < 2e-2, diff
    return diff


def static_layers(n, hk, d, gen):
    from transformers.cache_utils import StaticLayer
    lens = torch.zeros(n, dtype=torch.int64, device=DEV)
    layers = []
    for i in range(n):
        layer = StaticLayer(max_cache_len=L_MAX)
        layer.lazy_initialization(torch.empty(1, hk, 1, d, device=DEV, dtype=torch.float16), torch.empty(1, hk, 1, d, device=DEV, dtype=torch.float16))
        layer.keys.copy_(torch.randn(layer.keys.shape, device=DEV, dtype=torch.float16, generator=gen))
        layer.values.copy_(torch.randn(layer.values.shape, device=DEV, dtype=torch.float16, generator=gen))
        layer.cumulative_length = lens[i]
        layers.append(layer)
    return layers, lens


def padded_mask(s, behind, width):
    """The bool mask of `s` rows behind `behind` cached tokens of a sequence left-padded by PAD, [1, 1, s, width]."""
    j, i = torch.arange(width, device=DEV)[None, :], torch.arange(s, device=DEV)[:, None]
    return ((j <= behind + i) & (j >= PAD)).view(1, 1, s, width)


def op_points(args, gen):
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    for shape in SHAPES:
        hq, hk, d = shape
        module = types.SimpleNamespace(num_key_value_groups=hq // hk, is_causal=True)
        empty = torch.empty(1, hk, 0, d, device=DEV, dtype=torch.float16)
        for s, behind in [(s, 0) for s in ROWS] + [(CHUNK, BEHIND)]:
            n = max(2, min(args.links, 4096 // s))
            print(ops.attn_prefill_describe(1, hq, hk, d, s, L_MAX), f"links {n}", flush=True)
            # the projection outputs [1, S, H, D] viewed as [1, H, S, D], as the modules hand them over
            qs = [torch.randn(1, s, hq, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2) for _ in range(n)]
            ks = [torch.randn(1, s, hk, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2) for _ in range(n)]
            vs = [torch.randn(1, s, hk, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2) for _ in range(n)]
            past_k = torch.randn(1, hk, behind, d, device=DEV, dtype=torch.float16, generator=gen) if behind else empty
            past_v = torch.randn(1, hk, behind, d, device=DEV, dtype=torch.float16, generator=gen) if behind else empty
            la, lens_a = static_layers(n, hk, d, gen)
            lb, lens_b = static_layers(n, hk, d, gen)
            for x, y in zip(la, lb):
                y.keys.copy_(x.keys), y.values.copy_(x.values)
                if behind:
                    for t in (x, y):
                        t.keys[:, :, :behind], t.values[:, :, :behind] = past_k, past_v
            total = behind + s
            pairs = s * behind + s * (s + 1) // 2
            tag = f"({hq},{hk},{d}) S={s}" + (f"+{behind}" if behind else "")
            variants = [("dynamic", None if not behind else padded_mask(s, behind, total)), ("static", None if not behind else padded_mask(s, behind, L_MAX))]
            if not behind:
                variants += [("static", padded_mask(s, 0, L_MAX)), ("dynamic", padded_mask(s, 0, s))]
            for kind, mask in variants:
                masked_pairs = pairs if mask is None else int(mask.sum())      # the (row, key) pairs the call computes on

                def eager():
                    lens_a.fill_(behind)
                    outs = []
                    for layer, q, k, v in zip(la, qs, ks, vs):
                        kk, vv = (torch.cat([past_k, k], dim=-2), torch.cat([past_v, v], dim=-2)) if kind == "dynamic" else layer.update(k, v)
                        outs.append(sdpa_attention_forward(module, q, kk, vv, mask, dropout=0.0, scaling=d ** -0.5)[0])
                    return outs

                def kernel():
                    lens_b.fill_(behind)
                    outs = []
                    for i, (layer, q, k, v) in enumerate(zip(lb, qs, ks, vs)):
                        if kind == "dynamic":
                            kk, vv = torch.cat([past_k, k], dim=-2), torch.cat([past_v, v], dim=-2)
                            outs.append(ops.attn_prefill(q, kk, vv, total, mask=mask, scaling=d ** -0.5))
                        else:
                            kk, vv = layer.update(k, v)
                            outs.append(ops.attn_prefill(q, kk, vv, layer.cumulative_length, mask=mask, scaling=d ** -0.5))
                    return outs

                g_a, y_a = capture(eager)
                g_b, y_b = capture(kernel)
                real = slice(PAD, None) if mask is not None and not behind else slice(None)      # a padded prompt's first rows see no key
                diff = max_diff([y[:, real] for y in y_a], [y[:, real] for y in y_b])
                a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
                report(tag, f"{kind} {'masked' if mask is not None else 'no mask'}", shape, s, masked_pairs, a, b, diff)
                del g_a, g_b, y_a, y_b
            del la, lb, qs, ks, vs
            torch.cuda.empty_cache()


def band_mask(s, behind, width, window, pad=0):
    """The bool mask of `s` rows behind `behind` positions under a sliding window, [1, 1, s, width]: j <= behind + i, j > behind + i - window,
    j >= pad."""
    j, i = torch.arange(width, device=DEV)[None, :], torch.arange(s, device=DEV)[:, None]
    return ((j <= behind + i) & (j > behind + i - window) & (j >= pad)).view(1, 1, s, width)


def sliding_points(args, gen):
    """The --window points: see the module text."""
    from transformers.cache_utils import StaticSlidingWindowLayer
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    from qllm_amd.modeling.q_layers.fused_attention import _length_after_update
    w = args.window
    r = lambda *shape: torch.randn(shape, device=DEV, dtype=torch.float16, generator=gen)
    for shape in ((32, 8, 128), (32, 32, 128)):
        hq, hk, d = shape
        module = types.SimpleNamespace(num_key_value_groups=hq // hk, is_causal=True)
        for s, cached in ((128, 0), (512, 0), (w // 2, 0), (w, 0), (2 * w, 0), (CHUNK, w + 1000)):
            n = max(2, min(args.links, 4096 // s))
            qs = [r(1, s, hq, d).transpose(1, 2) for _ in range(n)]
            ks, vs = [r(1, s, hk, d).transpose(1, 2) for _ in range(n)], [r(1, s, hk, d).transpose(1, 2) for _ in range(n)]
            tag = f"({hq},{hk},{d}) W={w} S={s}" + (f"+{cached}" if cached else "")
            # dynamic: the layer returns what it kept (W - 1 positions once past the window) and the new rows
            kept = min(cached, w - 1)
            past_k, past_v = r(1, hk, kept, d), r(1, hk, kept, d)
            total = kept + s
            masks = [("no mask", None), ("masked", band_mask(s, 0, total, w, PAD))] if s < w and not cached else [("masked", band_mask(s, kept, total, w))]
            for what, mask in masks:
                def dyn(kernel):
                    outs = []
                    for q, k, v in zip(qs, ks, vs):
                        kk, vv = torch.cat([past_k, k], dim=-2), torch.cat([past_v, v], dim=-2)
                        if kernel:
                            outs.append(ops.attn_prefill(q, kk, vv, total, mask=mask, scaling=d ** -0.5, window=w))
                        else:
                            outs.append(sdpa_attention_forward(module, q, kk, vv, mask, dropout=0.0, scaling=d ** -0.5)[0])
                    return outs

                g_a, y_a = capture(lambda: dyn(False))
                g_b, y_b = capture(lambda: dyn(True))
                real = slice(PAD, None) if what == "masked" and s < w and not cached else slice(None)
                diff = max_diff([y[:, real] for y in y_a], [y[:, real] for y in y_b])
                a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
                report(tag, f"dynamic_sliding {what}", shape, s, s * (s + 1) // 2 + s * kept if mask is None else int(mask.sum()), a, b, diff)
                del g_a, g_b, y_a, y_b
            # static: a layer of W positions; it branches on its Python counter, which every call sets first
            lens_a, lens_b = torch.zeros(n, dtype=torch.int64, device=DEV), torch.zeros(n, dtype=torch.int64, device=DEV)
            la, lb = [], []
            for lens, layers in ((lens_a, la), (lens_b, lb)):
                for i in range(n):
                    layer = StaticSlidingWindowLayer(max_cache_len=w, sliding_window=w)
                    layer.lazy_initialization(torch.empty(1, hk, 1, d, device=DEV, dtype=torch.float16), torch.empty(1, hk, 1, d, device=DEV, dtype=torch.float16))
                    layer.cumulative_length = lens[i]
                    layers.append(layer)
            for x, y in zip(la, lb):
                x.keys.copy_(r(*x.keys.shape)), x.values.copy_(r(*x.values.shape))
                y.keys.copy_(x.keys), y.values.copy_(x.values)
            # what the layer returns: its W positions while the rows fit, the new rows alone when an empty layer overflows, W - 1 kept positions
            # and the new rows once it is full
            width, behind = (w, 0) if cached + s <= w else (s, 0) if not cached else (w - 1 + s, w - 1)
            mask = band_mask(s, behind, width, w)

            def stat(kernel, layers, lens):
                lens.fill_(min(cached, w))
                outs = []
                for layer, q, k, v in zip(layers, qs, ks, vs):
                    layer.cumulative_length_int = cached
                    kk, vv = layer.update(k, v)
                    if kernel:
                        outs.append(ops.attn_prefill(q, kk, vv, _length_after_update(layer, "static_sliding", kk), mask=mask, scaling=d ** -0.5, window=w))
                    else:
                        outs.append(sdpa_attention_forward(module, q, kk, vv, mask, dropout=0.0, scaling=d ** -0.5)[0])
                return outs

            g_a, y_a = capture(lambda: stat(False, la, lens_a))
            g_b, y_b = capture(lambda: stat(True, lb, lens_b))
            diff = max_diff(y_a, y_b)
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            report(tag, "static_sliding masked", shape, s, int(mask.sum()), a, b, diff)
            del g_a, g_b, y_a, y_b, la, lb, qs, ks, vs
            torch.cuda.empty_cache()


def layer_point(args, gen):
    import bench
    from transformers import StaticCache
    from qllm_amd.modeling.base import release_reference_layouts
    from qllm_amd.modeling.q_layers import (WQLinear_GEMM, install_fused_attention, install_fused_mlp, install_fused_norm, install_fused_residual,
                                            install_fused_rope, install_sibling_groups, uninstall_fused_attention)
    from rope_bench import decoder_layers
    n, s = 2, 2048
    layers, rot = decoder_layers(n, gen)
    install_sibling_groups(layers, [WQLinear_GEMM])
    release_reference_layouts(layers)
    assert install_fused_mlp(layers, [WQLinear_GEMM]) == n and install_fused_norm(layers, [WQLinear_GEMM]) == 2 * n
    assert install_fused_residual(layers, [WQLinear_GEMM]) == n and install_fused_rope(layers) == n
    cache = StaticCache(config=layers[0].self_attn.config, max_cache_len=L_MAX)
    lens = torch.zeros(n, dtype=torch.int64, device=DEV)
    for i, cl in enumerate(cache.layers[:n]):
        cl.lazy_initialization(torch.empty(1, 32, 1, 128, device=DEV, dtype=torch.float16), torch.empty(1, 32, 1, 128, device=DEV, dtype=torch.float16))
        cl.cumulative_length = lens[i]
    h = torch.randn(1, s, bench.HIDDEN, device=DEV, dtype=torch.float16, generator=gen)
    pos = (torch.arange(s, device=DEV) - PAD).clamp(min=0)[None]
    pe = rot(h, pos)
    mask = padded_mask(s, 0, L_MAX)

    def step():
        lens.fill_(0)
        return [layer(h, attention_mask=mask, position_ids=pos, past_key_values=cache, position_embeddings=pe) for layer in layers]

    g_a, y_a = capture(step)
    assert install_fused_attention(layers, prefill=True) == n
    g_b, y_b = capture(step)
    assert uninstall_fused_attention(layers) == n
    diff = max((a[:, PAD:].float() - b[:, PAD:].float()).abs().max().item() for a, b in zip(y_a, y_b))
    a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
    report("layer w4 g128 S=2048", "static masked", (32, 32, 128), s, s * (s + 1) // 2, a, b, diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=0.15)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-layer", action="store_true")
    ap.add_argument("--window", type=int, default=0, help="the sliding-layer points for this window instead of the full-attention ones")
    args = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  torch {torch.__version__}  "
          f"L_max: {L_MAX}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(7)
    with torch.no_grad():
        if args.window > 0:
            sliding_points(args, gen)
        else:
            op_points(args, gen)
        print("\nModule routing: (cache layer kind, mask) x rows -> eager / kernel at each shape; WIN: faster beyond the spread")
        for what in sorted({r["what"] for r in results}):
            for tag_rows in sorted({(r["rows"], "+" in r["config"]) for r in results if r["what"] == what}):
                rs = [r for r in results if r["what"] == what and (r["rows"], "+" in r["config"]) == tag_rows]
                cells = "  ".join(f"{tuple(r['shape'])}: {'WIN' if r['wins'] else 'no '} x{r['eager_mean_us'] / r['kernel_mean_us']:.2f}" for r in rs)
                print(f"  {what:16s} S={tag_rows[0]:5d}{' behind ' + (str(BEHIND) if not args.window else 'a full window') if tag_rows[1] else '':12s} {cells}", flush=True)
        if not args.no_layer and not args.window:
            layer_point(args, gen)


if __name__ == "__main__":
    main()
