#!/usr/bin/env python3
"""Mint golden vectors for the HQQ quantizer (qllm_hqq_quantize) from the REFERENCE's own Python, in the build container only:
    python tests/golden/make_goldens_hqq_quant.py

Same rules as make_goldens.py: /root/reference is imported read-only, only DATA is written.  The reference's quantizer
(qllm/quantization/hqq/_hqq_quantizer.py) is configured the way HQQQuant.do_quantize configures it (axis=1, channel_wise, optimize,
round_zero).  Its quantize() calls the proximal solver with the default device='cuda' (fp16 arithmetic); the solver is wrapped here to
run with device='cpu' -- its fp32 path -- and to hand out what it returns (s, z) and the error of every round it ran (read through its
own `verbose` print, at full precision).

Fixtures land in tests/golden/hqq_quant/ (a directory of their own: the layer fixtures next to this script are enumerated by glob).
Fields of hqqq_*.npz:
  bits, groupsize, N, K, w_dtype ("float16" | "bfloat16": the dtype W is exactly representable in)
  W [N,K] f32; s_inv [N,G] f32 = the solver's s (the INVERSE of the stored scale); zero [N,G] f32 = its final z
  Wq [N,K] u8 = clamp(rint(W s_inv + zero)); rounds_run; round_err [rounds_run] f64 (float(mean |W - Wr|) of each round)
  err_opt = mean |W - Wdq| of that run; err_rtn = the same with optimize=False
  zero_rev [N,G] f32 = the final z of a second run on W with each group's elements reversed (the solver's own summation-order noise)
  seed, stop_margin (see margin())
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "hqq_quant")
sys.path.insert(0, HERE)
from make_goldens import import_reference  # noqa: E402

CASES = [
    # name, bits, g, N, K, dtype, flat group
    ("hqqq_w2_g64", 2, 64, 64, 256, torch.float16, False),
    ("hqqq_w3_g64", 3, 64, 64, 256, torch.float16, False),
    ("hqqq_w4_g64", 4, 64, 64, 256, torch.float16, False),
    ("hqqq_w8_g64", 8, 64, 64, 256, torch.float16, False),
    ("hqqq_w4_g128_n48", 4, 128, 48, 384, torch.float16, False),
    ("hqqq_w4_g64_bf16", 4, 64, 64, 256, torch.bfloat16, False),
    ("hqqq_w3_g64_flat", 3, 64, 64, 256, torch.float16, True),
]


def reference_run(mod, W, bits, g, optimize):
    """One quantize() of the reference on the fp32 matrix W.  Returns (s, z, round errors, dequantised W)."""
    layer = torch.nn.Linear(W.shape[1], W.shape[0], bias=False)
    layer.weight.data = W.clone()
    qz = mod.InternalHQQQuantizer(layer)
    qz.configure(bits, channel_wise=True, group_size=g, optimize=optimize, round_zero=True, axis=1)
    got, errs = {}, []
    solver = qz.optimize_weights_proximal

    def on_cpu(**kw):
        got["s"], got["z"] = solver(device="cpu", verbose=True, **kw)
        return got["s"], got["z"]

    qz.optimize_weights_proximal = on_cpu
    keep = mod.np, getattr(mod, "print", None)
    mod.np = types.SimpleNamespace(round=lambda v, n: errs.append(float(v)))   # the solver's own `current_error`, unrounded
    mod.print = lambda *a, **k: None
    try:
        with torch.no_grad():
            scale, zero = qz.quantize()
    finally:
        mod.np = keep[0]
        if keep[1] is None:
            del mod.print
    G = W.shape[1] // g
    if optimize:
        s, z = got["s"].reshape(-1, G), got["z"].reshape(-1, G)
        assert torch.equal(1.0 / s, scale) and torch.equal(z, zero)
    else:
        s, z = None, zero
    return s, z, errs, layer.weight.data.clone()


def make_case(mod, case, seed):
    _, bits, g, N, K, dtype, _ = case
    W = draw(case, seed)
    G = K // g
    s, z, errs, wdq = reference_run(mod, W, bits, g, True)
    _, _, _, wdq_rtn = reference_run(mod, W, bits, g, False)
    w_rev = W.reshape(N, G, g).flip(-1).reshape(N, K).contiguous()
    _, z_rev, errs_rev, _ = reference_run(mod, w_rev, bits, g, True)
    max_v = 2 ** bits - 1
    se, ze = s.repeat_interleave(g, 1), z.repeat_interleave(g, 1)
    wq = torch.round(W * se + ze).clamp(0, max_v)
    assert torch.equal((wq - ze) / se, wdq)
    return dict(bits=bits, groupsize=g, N=N, K=K, w_dtype=str(dtype).split(".")[1], W=W.numpy(), s_inv=s.numpy(), zero=z.numpy(),
                Wq=wq.numpy().astype(np.uint8), rounds_run=len(errs), round_err=np.asarray(errs, np.float64),
                err_opt=float((W - wdq).abs().mean()), err_rtn=float((W - wdq_rtn).abs().mean()), zero_rev=z_rev.numpy(),
                rounds_rev=len(errs_rev))


MARGIN = 3e-5   # relative; the fp32 mean of 16384 values is good to ~1e-7


def margin(e, iters=20):
    """How clearly the loop control went the way it went: the smallest relative gap over the comparisons that decide rounds_run (the
    decreases that let the loop go on and, for an early stop, the one that ended it).  The error flattens as the solver converges, so
    that gap is small by nature: over 300 seeds per case the best ones reach 5e-5 .. 3e-4, never 1e-3."""
    e = np.asarray(e)
    n = len(e)
    gaps = [(e[i] - e[i + 1]) / e[i + 1] for i in range(n - 2)]
    if n < iters:
        gaps.append((e[-1] - e[:-1].min()) / e[:-1].min())
    return min(gaps)


def draw(case, seed):
    _, bits, g, N, K, dtype, flat = case
    gen = torch.Generator().manual_seed(seed)
    W = (0.02 * torch.randn((N, K), generator=gen)).to(dtype).float()
    if flat:
        W[5, g:2 * g] = W[5, g]          # one group with max == min: s clamps at 2e4
    return W


def main():
    import_reference()
    from qllm.quantization.hqq import _hqq_quantizer as mod
    os.makedirs(OUT, exist_ok=True)
    done = []
    for i, case in enumerate(CASES):
        # the seed whose stop decision is the clearest; the g128 case is the one asked to run all 20 rounds
        want_full = case[0] == "hqqq_w4_g128_n48"
        ranked = []
        for seed in range(300):
            errs = reference_run(mod, draw(case, seed), case[1], case[2], True)[2]
            if (len(errs) == 20) == want_full:
                ranked.append((margin(errs), seed))
        ranked.sort(reverse=True)
        for m, seed in ranked:
            d = make_case(mod, case, seed)
            agree = float((np.abs(d["zero"] - d["zero_rev"]) <= 1e-3).mean())
            if m > MARGIN and d.pop("rounds_rev") == d["rounds_run"] and agree >= 0.99:
                break
        else:
            raise SystemExit(f"{case[0]}: no acceptable seed")
        d["seed"], d["stop_margin"] = seed, m
        done.append(d)
        path = os.path.join(OUT, case[0] + ".npz")
        np.savez_compressed(path, **d)
        print(f"{case[0]:20s} {os.path.getsize(path) / 1024:7.1f} KiB seed={seed} rounds={d['rounds_run']:2d} margin={m:.1e} err_opt={d['err_opt']:.6e} "
              f"err_rtn={d['err_rtn']:.6e} zero agree(rev)={agree:.4f} max|dz|={np.abs(d['zero'] - d['zero_rev']).max():.2e}")
    assert any(d["rounds_run"] < 20 for d in done) and any(d["rounds_run"] == 20 for d in done), [d["rounds_run"] for d in done]


if __name__ == "__main__":
    main()
