#!/usr/bin/env python3
"""The rotary embedding of q and k as one kernel (qllm_rope, csrc/rope.hip; ops.rope) against the eager expression of transformers'
apply_rotary_pos_emb, fp16, in ONE process on one box, the two versions alternating A, B, A, B (the method of tools/swiglu_bench.py):

  one row    (q heads, k heads, head_dim) = (32, 32, 128), (32, 8, 128), (28, 4, 128) at one token, q and k as the attention forward hands
             them over ([1, H, 1, D] views of the projections' outputs), us per call --
               graph:  a hipGraph of --links calls on tensors of their own, replayed for at least --seconds per timing
               plain:  --plain-calls launches from Python behind one synchronise (host clock): what a model without graphs pays
  2048 rows  (32, 32, 128): us per call under graph replay (four sets of tensors, 0.5 GB in all: more than the 256 MB Infinity Cache) and
             the bytes the algorithm moves -- q, k read once, q_out, k_out written once, the two tables read once -- per second, beside
             the float4-copy ceiling bench.py quotes
  layer      one Llama-2-7B-shaped decoder layer (transformers' LlamaDecoderLayer, sdpa, AWQ 4-bit linears with 128-wide groups) at one
             token with fuse_mlp, fuse_norm and fuse_residual installed, without and with fuse_rope: us per layer under graph replay,
             --links layers with weights of their own per graph.  No KV cache: the attention core sees one key (it is the same in both
             versions; what differs is the rotary embedding in front of it)

The two versions' outputs are asserted bit-identical in every row.  Prints a table and one JSON line per row.

  python tools/rope_bench.py [--links 32] [--seconds 0.5] [--repeats 3] [--plain-calls 2000]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import (WQLinear_GEMM, install_fused_mlp, install_fused_norm, install_fused_residual, install_fused_rope,  # noqa: E402
                                        install_sibling_groups, uninstall_fused_rope)
from swiglu_bench import ab, row  # noqa: E402

DEV = "cuda:0"


def eager_rope(q, k, cos, sin, unsqueeze_dim=1):
    """transformers' apply_rotary_pos_emb (Llama, Mistral, Qwen2), expression for expression."""
    def rotate_half(x):
        x1 = x[..., : x.shape[-1] // 2]
        x2 = x[..., x.shape[-1] // 2:]
        return torch.cat((-x2, x1), dim=-1)
    cos = cos.unsqueeze(unsqueeze_dim)
    sin = sin.unsqueeze(unsqueeze_dim)
    return (q * cos) + (rotate_half(q) * sin), (k * cos) + (rotate_half(k) * sin)


def inputs(rows, hq, hk, d, sets, gen):
    """`sets` x (q, k, cos, sin): q / k [1, H, rows, D] views of [1, rows, H, D] memory, cos / sin [1, rows, D] of real angles."""
    out = []
    for _ in range(sets):
        q = torch.randn(1, rows, hq, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2)
        k = torch.randn(1, rows, hk, d, device=DEV, dtype=torch.float16, generator=gen).transpose(1, 2)
        ang = torch.rand(1, rows, d // 2, device=DEV, generator=gen) * 6.2832
        ang = torch.cat((ang, ang), -1)
        out.append((q, k, ang.cos().half(), ang.sin().half()))
    return out


def same(tag, ya, yb):
    """The two versions' outputs, call by call: the same bits, and the same strides in every dimension longer than one."""
    pairs = [(a, b) for pa, pb in zip(ya, yb) for a, b in zip(pa, pb)]
    bits = all(torch.equal(a, b) for a, b in pairs)
    strides = all([st for n, st in zip(a.shape, a.stride()) if n > 1] == [st for n, st in zip(b.shape, b.stride()) if n > 1] for a, b in pairs)
    print(f"{tag}: outputs of {len(ya)} calls bit-identical between the two versions: {bits}; same strides: {strides}", flush=True)
    assert bits and strides, tag


def plain_us(fn, sets, calls):
    """us per call of `calls` launches from Python, host clock around the loop and one synchronise."""
    for s in sets[:8]:
        fn(*s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(calls):
        fn(*sets[i % len(sets)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / calls


def decoder_layers(n, gen):
    """n LlamaDecoderLayers of Llama-2-7B's shape whose seven linears are AWQ q_layers with random weights, and the rotary module."""
    import transformers
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding
    cfg = transformers.LlamaConfig(hidden_size=bench.HIDDEN, intermediate_size=bench.INTER, num_hidden_layers=n, num_attention_heads=32,
                                   num_key_value_heads=32, vocab_size=32, max_position_embeddings=4096)
    cfg._attn_implementation = "sdpa"
    layers = torch.nn.ModuleList()
    for i in range(n):
        with torch.device("meta"):
            layer = LlamaDecoderLayer(cfg, i)
        for parent, name, K, N in ((layer.self_attn, "q_proj", bench.HIDDEN, bench.HIDDEN), (layer.self_attn, "k_proj", bench.HIDDEN, bench.HIDDEN),
                                   (layer.self_attn, "v_proj", bench.HIDDEN, bench.HIDDEN), (layer.self_attn, "o_proj", bench.HIDDEN, bench.HIDDEN),
                                   (layer.mlp, "gate_proj", bench.HIDDEN, bench.INTER), (layer.mlp, "up_proj", bench.HIDDEN, bench.INTER),
                                   (layer.mlp, "down_proj", bench.INTER, bench.HIDDEN)):
            setattr(parent, name, bench.make_layer(WQLinear_GEMM, K, N, DEV, gen))
        for norm in (layer.input_layernorm, layer.post_attention_layernorm):
            norm.weight = torch.nn.Parameter((torch.rand(bench.HIDDEN, device=DEV, generator=gen) * 0.4 + 0.8).half(), requires_grad=False)
        layers.append(layer.eval())
    return layers, LlamaRotaryEmbedding(cfg).to(DEV)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plain-calls", type=int, default=2000)
    args = ap.parse_args()
    n = args.links
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  "
          f"torch {torch.__version__}  calls per graph: {n}", flush=True)
    gen = torch.Generator(device=DEV).manual_seed(7)
    with torch.no_grad():
        # one row
        for hq, hk, d in ((32, 32, 128), (32, 8, 128), (28, 4, 128)):
            tag = f"1 x ({hq},{hk},{d})"
            sets = inputs(1, hq, hk, d, n, gen)
            g_a, y_a = bench.capture(lambda: [eager_rope(*s) for s in sets])
            g_b, y_b = bench.capture(lambda: [ops.rope(*s) for s in sets])
            same(tag, y_a, y_b)
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(tag, "graph", "eager", "kernel", a, b)
            del g_a, g_b
            a, b = [], []
            for _ in range(args.repeats):
                a.append(plain_us(eager_rope, sets, args.plain_calls))
                b.append(plain_us(ops.rope, sets, args.plain_calls))
            row(tag, "plain", "eager", "kernel", a, b)
        # 2048 rows: bytes per second
        rows, hq, hk, d = 2048, 32, 32, 128
        tag = f"{rows} x ({hq},{hk},{d})"
        sets = inputs(rows, hq, hk, d, 4, gen)
        g_a, y_a = bench.capture(lambda: [eager_rope(*s) for s in sets])
        g_b, y_b = bench.capture(lambda: [ops.rope(*s) for s in sets])
        same(tag, y_a, y_b)
        a, b = ab(g_a, g_b, len(sets), args.seconds, args.repeats)
        row(tag, "graph", "eager", "kernel", a, b)
        moved = 2 * 2 * rows * (hq + hk) * d + 2 * 2 * rows * d          # q, k in and out; cos, sin in: 2-byte elements
        us = sum(b) / len(b)
        rec = dict(config=tag, what="bytes", bytes_moved=moved, kernel_us=round(us, 3), gb_per_s=round(moved / us / 1e3, 1), copy_ceiling_gb_per_s=bench.HBM_COPY_GBPS,
                   share_of_copy_ceiling=round(moved / us / 1e3 / bench.HBM_COPY_GBPS, 3))
        print(f"{tag:14s} bytes moved {moved / 1e6:.1f} MB in {us:.2f} us: {rec['gb_per_s']:.0f} GB/s, {100 * rec['share_of_copy_ceiling']:.1f} % of the "
              f"{bench.HBM_COPY_GBPS:.0f} GB/s copy ceiling", flush=True)
        print("JSON " + json.dumps(rec), flush=True)
        del g_a, g_b, y_a, y_b, sets
        torch.cuda.empty_cache()
        # one decoder layer, the other three fusions on
        layers, rot = decoder_layers(n, gen)
        install_sibling_groups(layers, [WQLinear_GEMM])
        from qllm_amd.modeling.base import release_reference_layouts
        release_reference_layouts(layers)
        assert install_fused_mlp(layers, [WQLinear_GEMM]) == n and install_fused_norm(layers, [WQLinear_GEMM]) == 2 * n
        assert install_fused_residual(layers, [WQLinear_GEMM]) == n
        h = torch.randn(1, 1, bench.HIDDEN, device=DEV, dtype=torch.float16, generator=gen)
        pos = torch.tensor([[17]], device=DEV)
        pe = rot(h, pos)
        step = lambda: [layer(h, attention_mask=None, position_ids=pos, position_embeddings=pe) for layer in layers]  # noqa: E731
        g_a, y_a = bench.capture(step)
        assert install_fused_rope(layers) == n
        g_b, y_b = bench.capture(step)
        assert uninstall_fused_rope(layers) == n
        ok = all(torch.equal(x, y) and bool(torch.isfinite(x.float()).all()) for x, y in zip(y_a, y_b))
        print(f"layer: outputs of {n} layers finite and bit-identical between the two versions: {ok}", flush=True)
        assert ok
        a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
        row("awq w4 g128 M=1", "layer", "3 fused", "+ rope", a, b)


if __name__ == "__main__":
    main()
