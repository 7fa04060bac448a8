#!/usr/bin/env python3
"""A/B of the fused residual add (qllm_linear_forward_residual; csrc/strip1_resid.hip, csrc/strip1_swiglu_resid.hip) at Llama-2-7B's shapes
(4096 / 11008), one row, fp16, in ONE process on one box, the two versions alternating A, B, A, B (the method of tools/swiglu_bench.py):

  oproj    the attention's output segment, us per link --
             unfused: r + o_proj(x)                      (the launch, then the elementwise add: what the decoder layer evaluates today)
             fused:   o_proj.forward_residual(x, r)      (one launch)
  mlp      the MLP segment with the fused MLP installed, us per link --
             unfused: r + mlp(n)                         (grouped gate/up launch, SWIGLU down_proj launch, the elementwise add)
             fused:   down_proj.forward_swiglu_residual(gate_proj(n), up_proj(n), r)   (two launches)
  layer    both segments through the modules, us per link: a decoder layer without its attention core and with identity norms --
             unfused: uninstall_fused_residual           (the parent commit's sequence)
             fused:   install_fused_residual
  o / down the o_proj (down_proj) launch alone on fixed inputs, us per launch: the plain (SWIGLU) form against its RESID form -- the
           epilogue's own cost, apart from the kernel it saves

Each version is a hipGraph of --links links with weights of their own (nothing stays in L2 from one to the next; every link reads the same
fixed unit-normal inputs, so the activations stay finite, and the two versions' outputs are asserted finite and bit-identical link by
link), warmed up on its own and replayed for at least --seconds per timing; --repeats timings per version.  Prints a table and one JSON line per row.

  python tools/residual_bench.py [--links 32] [--seconds 0.5] [--repeats 3]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import (QuantLinearHQQ, WQLinear_GEMM, install_fused_mlp, install_fused_residual,  # noqa: E402
                                        install_sibling_groups, uninstall_fused_residual)
from swiglu_bench import LlamaMLP, ab, row  # noqa: E402


class LlamaAttention(torch.nn.Module):
    """The attention's last step under its Llama name: o_proj of whatever the core produced (the core itself is not what is measured)."""

    def __init__(self, cls, dev, gen, bits, group):
        super().__init__()
        self.o_proj = bench.make_layer(cls, bench.HIDDEN, bench.HIDDEN, dev, gen, bits=bits, group=group)

    def forward(self, hidden_states, **kwargs):
        return self.o_proj(hidden_states), None


class LlamaDecoderLayer(torch.nn.Module):
    """transformers' decoder-layer data flow around the two launches with a residual behind them (the class name and the annotation are
    what install_fused_residual looks for)."""

    def __init__(self, cls, dev, gen, bits, group):
        super().__init__()
        self.self_attn = LlamaAttention(cls, dev, gen, bits, group)
        self.mlp = LlamaMLP(cls, dev, gen, bits, group)
        self.input_layernorm, self.post_attention_layernorm = torch.nn.Identity(), torch.nn.Identity()

    def forward(self, hidden_states: torch.Tensor, **kwargs) -> torch.Tensor:
        residual = hidden_states
        hidden_states = self.input_layernorm(hidden_states)
        hidden_states, _ = self.self_attn(hidden_states=hidden_states, **kwargs)
        hidden_states = residual + hidden_states
        residual = hidden_states
        hidden_states = self.post_attention_layernorm(hidden_states)
        hidden_states = self.mlp(hidden_states)
        return residual + hidden_states


class Chain(torch.nn.Module):
    def __init__(self, cls, n, dev, bits, group):
        super().__init__()
        gen = torch.Generator(device=dev).manual_seed(7)
        self.layers = torch.nn.ModuleList([LlamaDecoderLayer(cls, dev, gen, bits, group) for _ in range(n)])
        self.groups = install_sibling_groups(self, [cls])
        from qllm_amd.modeling.base import release_reference_layouts
        release_reference_layouts(self)
        assert install_fused_mlp(self, [cls]) == n   # (the MLP segment is measured with the fused MLP in place)

    # Every link reads the SAME fixed unit-normal tensors and keeps an output of its own: random weights that preserve magnitude would
    # double the variance per link of a real chain (fp16 overflows before link 30), and the outputs of the two versions are compared.
    # The launches of one stream run one after the other either way.
    def forward(self, h):
        return [layer(h) for layer in self.layers]

    def oproj(self, x, r, fused):
        return [layer.self_attn.o_proj.forward_residual(x, r) if fused else r + layer.self_attn.o_proj(x) for layer in self.layers]

    def mlp(self, n, r, fused):
        return [layer.mlp.down_proj.forward_swiglu_residual(layer.mlp.gate_proj(n), layer.mlp.up_proj(n), r) if fused else r + layer.mlp(n)
                for layer in self.layers]


def compared(tag, what, ya, yb):
    """The two versions' outputs, link by link: all finite, and the same bits."""
    finite = all(bool(torch.isfinite(t.float()).all()) for t in ya + yb)
    same = all(torch.equal(a, b) for a, b in zip(ya, yb))
    print(f"{tag} {what}: outputs of {len(ya)} links finite: {finite}; bit-identical between the two versions: {same}", flush=True)
    assert finite and same, (tag, what)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--links", type=int, default=32)
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    n = args.links
    print(f"device: {torch.cuda.get_device_name(0)}  CUs: {torch.cuda.get_device_properties(0).multi_processor_count}  "
          f"torch {torch.__version__}  links per graph: {n}", flush=True)
    configs = (("awq w4 g128", WQLinear_GEMM, 4, 128), ("hqq w4 g64", QuantLinearHQQ, 4, 64), ("hqq w3 g64", QuantLinearHQQ, 3, 64))
    for name, cls, bits, group in configs:
        tag = f"{name} M=1"
        with torch.no_grad():
            chain = Chain(cls, n, dev, bits, group)
            h = torch.randn(1, 1, bench.HIDDEN, device=dev, dtype=torch.float16)
            res = torch.randn(1, 1, bench.HIDDEN, device=dev, dtype=torch.float16)
            first = chain.layers[0]
            wo, wd = first.self_attn.o_proj.native_descriptor(0), first.mlp.down_proj.native_descriptor(0)
            print(f"{tag}: o_proj {ops.residual_describe(wo, 1)}; down_proj {ops.residual_describe(wd, 1, True)}", flush=True)
            # the two segments, as the decoder layer evaluates them today and through the fused methods
            for what, fn in (("oproj", chain.oproj), ("mlp", chain.mlp)):
                g_a, y_a = bench.capture(lambda: fn(h, res, False))
                g_b, y_b = bench.capture(lambda: fn(h, res, True))
                compared(tag, what, y_a, y_b)
                a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
                row(tag, what, "unfused", "fused", a, b)
                del g_a, g_b
            # both segments through the modules
            g_a, y_a = bench.capture(lambda: chain(h))
            assert install_fused_residual(chain, [cls]) == n
            g_b, y_b = bench.capture(lambda: chain(h))
            assert uninstall_fused_residual(chain) == n
            compared(tag, "layer", y_a, y_b)
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(tag, "layer", "unfused", "fused", a, b)
            del g_a, g_b
            # the launches alone, on fixed inputs
            x = torch.randn(1, bench.HIDDEN, device=dev, dtype=torch.float16)
            r = torch.randn(1, bench.HIDDEN, device=dev, dtype=torch.float16)
            gt = torch.randn(1, bench.INTER, device=dev, dtype=torch.float16)
            ut = torch.randn(1, bench.INTER, device=dev, dtype=torch.float16)
            os_ = [layer.self_attn.o_proj.native_descriptor(0) for layer in chain.layers]
            ds = [layer.mlp.down_proj.native_descriptor(0) for layer in chain.layers]
            g_a, _ = bench.capture(lambda: [ops.linear_forward(w, x) for w in os_][-1])
            g_b, _ = bench.capture(lambda: [ops.linear_forward_residual(w, x, r) for w in os_][-1])
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(tag, "o", "plain", "resid", a, b)
            del g_a, g_b
            g_a, _ = bench.capture(lambda: [ops.linear_forward_swiglu(w, gt, ut) for w in ds][-1])
            g_b, _ = bench.capture(lambda: [ops.linear_forward_swiglu_residual(w, gt, ut, r) for w in ds][-1])
            a, b = ab(g_a, g_b, n, args.seconds, args.repeats)
            row(tag, "down", "swiglu", "resid", a, b)
            del g_a, g_b, chain
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
