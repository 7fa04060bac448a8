#!/usr/bin/env python3
"""Single-token attention over a static KV cache as one kernel (qllm_attn_decode, csrc/attn_decode.hip; ops.attn_decode) against what
transformers runs there, fp16, in ONE process on one box, the two versions alternating A, B, A, B (the method of tools/rope_bench.py):

  op      (q heads, kv heads, head_dim) = (32, 32, 128), (32, 8, 128), (28, 4, 128), StaticCache-shaped buffers of L_max = 4096 positions,
          kv_len 1, 128, 1024 and 4095 tokens in the cache before the step, us per step under graph replay (a hipGraph of --links steps on
          tensors of their own) --
            eager:   StaticLayer.update (arange, add, add_, two index_copy_) and transformers' sdpa_attention_forward over all 4096
                     positions behind the bool mask transformers builds for such a step (built once, outside the graph)
            kernel:  ops.attn_decode in its append form with the length read from device memory and the same mask, and the add_
          and the valid K / V bytes -- 2 x kv heads x (kv_len + 1) x head_dim x 2 -- per second beside the copy ceiling bench.py quotes.
          Every length lives in one tensor that the graph refills first (one fill per replay for all links, in both versions), so a
          replay is the same step every time and no length walks past the cache.
  layer   one Llama-2-7B-shaped decoder layer (AWQ 4-bit linears, 128-wide groups, sdpa) at one token with fuse_mlp, fuse_norm,
          fuse_residual and fuse_rope installed, without and with install_fused_attention, a StaticCache of 4096 positions holding 1 and
          1024 tokens: us per layer under graph replay, --links layers with weights and cache layers of their own per graph.

The two versions' outputs are compared in every row (maximum absolute difference, printed; both finite).  Prints a table and one JSON line
per row.

  --window W   instead of the points above, the sliding layers of a Mistral-shaped config with that window, (32, 8, 128) and (32, 32, 128):
          the step below the window (W / 4 tokens cached), at it (W - 1 cached: the step fills it) and past it (W + 1000 cached), us per
          step under graph replay --
            dynamic  DynamicSlidingWindowLayer.update's own statements (torch.cat of the W - 1 positions it keeps, or fewer, and the new
                     row), then sdpa with mask None over what it returns  |  the same statements, then ops.attn_decode(window=W)
            static   StaticSlidingWindowLayer.update (index_copy_ until the layer is full; past the window its statements restated: roll,
                     index put and copy_ of the whole buffer at every token), then sdpa over all W positions behind the bool mask  |  the same update, then
                     ops.attn_decode(window=W) with the length the modules hand over; past the window also the update ALONE, which
                     both versions pay.
            ring     that fused static step (update included)  |  a RingSlidingWindowLayer of the same W: ops.attn_decode_ring over the
                     layer's buffers with the total read from the device and the append in the kernel, then the add_ that bumps the
                     total: no update, no roll.  Its output is held, bit for bit, against ops.attn_decode on the linearised positions.

  python tools/attn_decode_bench.py [--links 16] [--seconds 0.4] [--repeats 3] [--window W]"""
import argparse
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import (WQLinear_GEMM, install_fused_attention, install_fused_mlp, install_fused_norm, install_fused_residual,  # noqa: E402
                                        install_fused_rope, install_sibling_groups, uninstall_fused_attention)
from rope_bench import decoder_layers  # noqa: E402
from swiglu_bench import ab, row, timed  # noqa: E402

DEV = "cuda:0"
L_MAX = 4096
_side = None


def capture(fn, warm=2):
    """bench.capture on ONE side stream for the whole run: ops.workspace is per stream, so the warm-up calls create the one every later
    capture finds (a workspace first asked for inside a capture would be zero-filled by every replay)."""
    global _side
    if _side is None:
        _side = torch.cuda.Stream()
    _side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(_side):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=_side):
            out = fn()
    torch.cuda.current_stream().wait_stream(_side)
    g.replay()
    torch.cuda.synchronize()
    return g, out


def static_layers(n, hk, d, gen):
    """n transformers StaticLayers of L_MAX positions with random contents, their lengths the elements of ONE int64 tensor."""
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


def max_diff(tag, ya, yb):
    diff = max((a.float().reshape(-1) - b.float().reshape(-1)).abs().max().item() for a, b in zip(ya, yb))
    ok = all(bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all()) for a, b in zip(ya, yb))
    scale = max(1.0, max(a.float().abs().max().item() for a in ya))
    print(f"{tag}: outputs of {len(ya)} steps finite: {ok}; maximum absolute difference between the two versions {diff:.3e} (largest magnitude {scale:.2f})", flush=True)
    assert ok and diff < 2e-2 * scale, tag
    return diff


def sliding_points(args, gen):
    """The --window points: see the module text."""
    from transformers.cache_utils import StaticSlidingWindowLayer
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    from qllm_amd.modeling.q_layers.fused_attention import _length_after_update
    from qllm_amd.modeling.ring_cache import RingSlidingWindowLayer
    n, w = args.links, args.window
    for hq, hk, d in ((32, 8, 128), (32, 32, 128)):
        print(ops.attn_decode_describe(1, hq, hk, d, w), flush=True)
        module = types.SimpleNamespace(num_key_value_groups=hq // hk, is_causal=True)
        r = lambda *shape: torch.randn(shape, device=DEV, dtype=torch.float16, generator=gen)
        qs = [r(1, 1, hq, d).transpose(1, 2) for _ in range(n)]
        kns, vns = [r(1, 1, hk, d).transpose(1, 2) for _ in range(n)], [r(1, 1, hk, d).transpose(1, 2) for _ in range(n)]
        for where, cached in (("below", w // 4), ("at", w - 1), ("past", w + 1000)):
            tag = f"({hq},{hk},{d}) W={w} {where}"
            # dynamic: the layer keeps the last W - 1 positions (all of them below the window)
            kept = min(cached, w - 1)
            pks, pvs = [r(1, hk, kept, d) for _ in range(n)], [r(1, hk, kept, d) for _ in range(n)]

            def dyn_eager():
                outs = []
                for q, kn, vn, pk, pv in zip(qs, kns, vns, pks, pvs):
                    k, v = torch.cat([pk, kn], dim=-2), torch.cat([pv, vn], dim=-2)
                    outs.append(sdpa_attention_forward(module, q, k, v, None, dropout=0.0, scaling=d ** -0.5, is_causal=False)[0])
                return outs

            def dyn_kernel():
                outs = []
                for q, kn, vn, pk, pv in zip(qs, kns, vns, pks, pvs):
                    k, v = torch.cat([pk, kn], dim=-2), torch.cat([pv, vn], dim=-2)
                    outs.append(ops.attn_decode(q, k, v, k.shape[2], scaling=d ** -0.5, window=w))
                return outs

            g_a, y_a = capture(dyn_eager)
            g_b, y_b = capture(dyn_kernel)
            max_diff(tag + " dynamic", y_a, y_b)
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(tag, "dyn", "eager", "kernel", a, b)
            del g_a, g_b, y_a, y_b, pks, pvs
            # static: layers of W positions; the layer itself branches on its Python counter, so every call sets it first
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
            mask = (torch.arange(w, device=DEV) <= cached).view(1, 1, 1, w)                    # past the window: every position

            last = torch.tensor([-1], dtype=torch.int64, device=DEV)

            def update(layers, lens, kn_vn):
                lens.fill_(min(cached, w))
                out = []
                for layer, (kn, vn) in zip(layers, kn_vn):
                    layer.cumulative_length_int = cached
                    if cached < w:
                        out.append(layer.update(kn, vn))
                        continue
                    # the layer's own statements once it is full, with the index tensor it builds from a Python list at every call
                    # (a host-to-device copy, which a capture does not take) made once above
                    new_keys, new_values = layer.keys.roll(-1, dims=-2), layer.values.roll(-1, dims=-2)
                    new_keys[:, :, last], new_values[:, :, last] = kn, vn
                    layer.keys.copy_(new_keys), layer.values.copy_(new_values)
                    layer.cumulative_length_int = cached + 1
                    out.append((layer.keys, layer.values))
                return out

            def st_eager():
                return [sdpa_attention_forward(module, q, k, v, mask, dropout=0.0, scaling=d ** -0.5)[0] for q, (k, v) in zip(qs, update(la, lens_a, zip(kns, vns)))]

            def st_kernel():
                outs = []
                for q, layer, (k, v) in zip(qs, lb, update(lb, lens_b, zip(kns, vns))):
                    outs.append(ops.attn_decode(q, k, v, _length_after_update(layer, "static_sliding", k), mask=mask, scaling=d ** -0.5, window=w))
                return outs

            g_a, y_a = capture(st_eager)
            g_b, y_b = capture(st_kernel)
            max_diff(tag + " static", y_a, y_b)
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(tag, "stat", "eager", "kernel", a, b)
            if where == "past":
                g_u, _ = capture(lambda: update(lb, lens_b, zip(kns, vns)))
                u = [timed(g_u, n, args.seconds) for _ in range(args.repeats)]
                mu, mb = sum(u) / len(u), sum(b) / len(b)
                rec = dict(config=tag, what="roll", update_alone_us=[round(x, 3) for x in u], update_mean_us=round(mu, 3), kernel_mean_us=round(mb, 3),
                           eager_mean_us=round(sum(a) / len(a), 3), share_of_kernel_step=round(mu / mb, 4))
                print(f"{tag:14s} the layer's update alone (roll, index put, copy_): {mu:.2f} us = {100 * mu / mb:.1f} % of the kernel step", flush=True)
                print("JSON " + json.dumps(rec), flush=True)
                del g_u
            # ring: RingSlidingWindowLayers holding the same positions in slot j mod W; the step is ONE ops.attn_decode_ring (the total
            # from the device, the append in the kernel) and the add_ that bumps the total -- what the modules run on a ring cache --
            # against the fused static step above (update included in both)
            lens_r = torch.zeros(n, dtype=torch.int64, device=DEV)
            lr = []
            for i, x in enumerate(lb):
                layer = RingSlidingWindowLayer(max_cache_len=w, sliding_window=w)
                layer.lazy_initialization(torch.empty(1, hk, 1, d, device=DEV, dtype=torch.float16), torch.empty(1, hk, 1, d, device=DEV, dtype=torch.float16))
                layer.cumulative_length = lens_r[i]
                layer.keys.copy_(x.keys), layer.values.copy_(x.values)
                lr.append(layer)

            def ring_kernel():
                lens_r.fill_(cached)
                outs = []
                for q, layer, kn, vn in zip(qs, lr, kns, vns):
                    outs.append(ops.attn_decode_ring(q, layer.keys, layer.values, layer.cumulative_length, w, k_new=kn, v_new=vn, mask=mask, scaling=d ** -0.5))
                    layer.cumulative_length.add_(1)
                return outs

            g_r, y_r = capture(ring_kernel)
            assert lens_r.tolist() == [cached + 1] * n
            lo = max(0, cached + 1 - w)
            idx = torch.arange(lo, lo + w, device=DEV) % w                                    # the linearised copy: W positions from lo on, cached + 1 - lo of them valid
            want = [ops.attn_decode(q, layer.keys.index_select(2, idx), layer.values.index_select(2, idx), cached + 1 - lo, mask=mask, scaling=d ** -0.5)
                    for q, layer in zip(qs, lr)]                                             # the linear call of max_len = W: the very bits
            assert all(torch.equal(a, b) for a, b in zip(y_r, want)), tag
            max_diff(tag + " ring (against the linearised call)", y_r, want)
            a, b = ab(g_b, g_r, n, args.seconds, args.repeats)
            row(tag, "ring", "static", "ring", a, b)
            del g_a, g_b, g_r, y_a, y_b, y_r, la, lb, lr
            torch.cuda.empty_cache()


def main():
    from transformers.integrations.sdpa_attention import sdpa_attention_forward
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window", type=int, default=0, help="the sliding-layer points for this window instead of the full-attention ones")
    args = ap.parse_args()
    n = args.links
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  "
          f"torch {torch.__version__}  steps per graph: {n}  L_max: {L_MAX}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(7)
    if args.window > 0:
        with torch.no_grad():
            sliding_points(args, gen)
        return
    with torch.no_grad():
        for hq, hk, d in ((32, 32, 128), (32, 8, 128), (28, 4, 128)):
            print(ops.attn_decode_describe(1, hq, hk, d, L_MAX), flush=True)
            module = types.SimpleNamespace(num_key_value_groups=hq // hk, is_causal=True)
            la, lens_a = static_layers(n, hk, d, gen)
            lb, lens_b = static_layers(n, hk, d, gen)
            for x, y in zip(la, lb):
                y.keys.copy_(x.keys), y.values.copy_(x.values)
            qs = [torch.randn(1, 1, hq, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2) for _ in range(n)]
            kns = [torch.randn(1, 1, hk, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2) for _ in range(n)]
            vns = [torch.randn(1, 1, hk, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2) for _ in range(n)]
            for kv_len in (1, 128, 1024, 4095):
                tag = f"({hq},{hk},{d}) {kv_len}"
                mask = (torch.arange(L_MAX, device=DEV) <= kv_len).view(1, 1, 1, L_MAX)

                def eager():
                    lens_a.fill_(kv_len)
                    outs = []
                    for layer, q, kn, vn in zip(la, qs, kns, vns):
                        k, v = layer.update(kn, vn)
                        outs.append(sdpa_attention_forward(module, q, k, v, mask, dropout=0.0, scaling=d ** -0.5)[0])
                    return outs

                def kernel():
                    lens_b.fill_(kv_len)
                    outs = []
                    for i, (layer, q, kn, vn) in enumerate(zip(lb, qs, kns, vns)):
                        outs.append(ops.attn_decode(q, layer.keys, layer.values, lens_b[i], kn, vn, mask=mask))
                        lens_b[i].add_(1)
                    return outs

                g_a, y_a = capture(eager)
                g_b, y_b = capture(kernel)
                max_diff(tag, y_a, y_b)
                assert lens_a.tolist() == lens_b.tolist() == [kv_len + 1] * n
                assert all(torch.equal(x.keys[:, :, kv_len], y.keys[:, :, kv_len]) for x, y in zip(la, lb))
                a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
                row(tag, "op", "eager", "kernel", a, b)
                valid = 2 * hk * (kv_len + 1) * d * 2
                us = sum(b) / len(b)
                rec = dict(config=tag, what="bytes", valid_kv_bytes=valid, kernel_us=round(us, 3), eager_us=round(sum(a) / len(a), 3), gb_per_s=round(valid / us / 1e3, 1),
                           copy_ceiling_gb_per_s=bench.HBM_COPY_GBPS, share_of_copy_ceiling=round(valid / us / 1e3 / bench.HBM_COPY_GBPS, 4))
                print(f"{tag:18s} valid K/V {valid / 1e6:.3f} MB in {us:.2f} us: {rec['gb_per_s']:.0f} GB/s, {100 * rec['share_of_copy_ceiling']:.2f} % of the "
                      f"{bench.HBM_COPY_GBPS:.0f} GB/s copy ceiling", flush=True)
                print("JSON " + json.dumps(rec), flush=True)
                del g_a, g_b, y_a, y_b
            del la, lb, qs, kns, vns
            torch.cuda.empty_cache()
        # one decoder layer, the other four fusions on
        from transformers import StaticCache
        layers, rot = decoder_layers(n, gen)
        install_sibling_groups(layers, [WQLinear_GEMM])
        from qllm_amd.modeling.base import release_reference_layouts
        release_reference_layouts(layers)
        assert install_fused_mlp(layers, [WQLinear_GEMM]) == n and install_fused_norm(layers, [WQLinear_GEMM]) == 2 * n
        assert install_fused_residual(layers, [WQLinear_GEMM]) == n and install_fused_rope(layers) == n
        cfg = layers[0].self_attn.config
        cache = StaticCache(config=cfg, max_cache_len=L_MAX)
        lens = torch.zeros(n, dtype=torch.int64, device=DEV)
        for i, cl in enumerate(cache.layers):
            cl.lazy_initialization(torch.empty(1, 32, 1, 128, device=DEV, dtype=torch.float16), torch.empty(1, 32, 1, 128, device=DEV, dtype=torch.float16))
            cl.keys.copy_(torch.randn(cl.keys.shape, device=DEV, dtype=torch.float16, generator=gen))
            cl.values.copy_(torch.randn(cl.values.shape, device=DEV, dtype=torch.float16, generator=gen))
            cl.cumulative_length = lens[i]
        h = torch.randn(1, 1, bench.HIDDEN, device=DEV, dtype=torch.float16, generator=gen)
        for kv_len in (1, 1024):
            pos = torch.tensor([[kv_len]], device=DEV)
            pe = rot(h, pos)
            mask = (torch.arange(L_MAX, device=DEV) <= kv_len).view(1, 1, 1, L_MAX)

            def step():
                lens.fill_(kv_len)
                return [layer(h, attention_mask=mask, position_ids=pos, past_key_values=cache, position_embeddings=pe) for layer in layers]

            g_a, y_a = capture(step)
            assert install_fused_attention(layers) == n
            g_b, y_b = capture(step)
            assert uninstall_fused_attention(layers) == n
            max_diff(f"layer {kv_len}", y_a, y_b)
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(f"w4 g128 kv={kv_len}", "layer", "4 fused", "+ attn", a, b)
            del g_a, g_b


if __name__ == "__main__":
    main()
