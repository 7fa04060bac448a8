#!/usr/bin/env python3
"""Time the GPTQ quantizer per layer on the device: the Hessian factorisation (torch) and the fused column solver (qllm_gptq_quantize),
against a per-column torch loop of the same algorithm on the same inputs (six small launches per column: what the fused kernel
replaces).  Events around each leg, one warm-up, `--repeats` timed runs, median reported.

    python tools/gptq_quantize_bench.py [--shapes 4096x4096,4096x11008,11008x4096] [--repeats 3] [--no-loop]

--static-groups times, instead of the torch loop, the static-groups solver (qllm_gptq_quantize_static) next to qllm_gptq_quantize on the
same inputs in the same run, alternating, with the torch work each path needs around its kernel (dynamic + act-order: W[:, perm] before,
codes[inv] and wq[:, inv] after; static: perm as int32), and then what the feature is for: the batch-1 forward of a 4096 x 4096 4-bit
g128 layer quantized plain, with act-order, and with act-order + static groups (events around 200 graph-free calls after a warm-up,
median of three), each next to its qllm_plan_describe line.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qllm_amd import _lib, ops  # noqa: E402
from qllm_amd.quantization import gptq  # noqa: E402

DEV = "cuda:0"


def column_loop(W, U, bits, g):
    """GPTQ's column walk written with torch tensors: blocks of 128, group parameters at group starts from the block-boundary state."""
    W = W.float().clone()
    N, K = W.shape
    maxq = 2 ** bits - 1
    Q = torch.zeros_like(W)
    zero_t = torch.zeros(N, device=W.device)
    for i1 in range(0, K, 128):
        i2 = min(i1 + 128, K)
        W1 = W[:, i1:i2].clone()
        Err = torch.zeros_like(W1)
        U1 = U[i1:i2, i1:i2]
        for i in range(i2 - i1):
            if (i1 + i) % g == 0:
                blk = W[:, i1 + i:i1 + i + g]
                xmin, xmax = torch.minimum(blk.min(1)[0], zero_t), torch.maximum(blk.max(1)[0], zero_t)
                flat = (xmin == 0) & (xmax == 0)
                xmin, xmax = torch.where(flat, -torch.ones_like(xmin), xmin), torch.where(flat, torch.ones_like(xmax), xmax)
                scale = (xmax - xmin) / maxq
                zero = torch.round(-xmin / scale)
            w = W1[:, i]
            q = scale * (torch.clamp(torch.round(w / scale) + zero, 0, maxq) - zero)
            Q[:, i1 + i] = q
            err = (w - q) / U1[i, i]
            W1[:, i:] -= err.unsqueeze(1).matmul(U1[i, i:].unsqueeze(0))
            Err[:, i] = err
        W[:, i2:] -= Err.matmul(U[i1:i2, i2:])
    return Q


def timed(fn, repeats):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts), out


def static_leg(W, w, U, perm, repeats):
    """One line: both solvers on the same (W, U, perm), alternating, and the torch side of each path."""
    K = W.shape[1]
    p32 = perm.int() if perm is not None else None
    t_d, t_s = [], []
    for _ in range(repeats):
        t_d.append(timed(lambda: ops.gptq_quantize(w, U, 4, 128, False), 1)[0])
        t_s.append(timed(lambda: ops.gptq_quantize_static(W, U, p32, 4, 128, False, check_perm=False), 1)[0])
    codes, _, _, wq, _ = ops.gptq_quantize(w, U, 4, 128, False)
    torch_d = torch_s = 0.0
    if perm is not None:
        inv = torch.argsort(perm)
        torch_d = timed(lambda: W[:, perm].contiguous(), repeats)[0] + timed(lambda: (codes[inv].contiguous(), wq[:, inv].contiguous()), repeats)[0]
        torch_s = timed(lambda: perm.int(), repeats)[0]
    d, s = statistics.median(t_d), statistics.median(t_s)
    return (f"qllm_gptq_quantize {d:.3f} ms [{min(t_d):.3f}..{max(t_d):.3f}] + torch {torch_d:.3f} ms | qllm_gptq_quantize_static {s:.3f} ms "
            f"[{min(t_s):.3f}..{max(t_s):.3f}] + torch {torch_s:.3f} ms | static / dynamic kernel x{s / d:.3f}, with torch x{(s + torch_s) / (d + torch_d):.3f}")


def forward_leg(N=4096, K=4096, calls=200):
    """Batch-1 forward of one layer quantized three ways, from the same weights and Hessian."""
    gen = torch.Generator().manual_seed(N + K)
    W = (0.02 * torch.randn((N, K), generator=gen)).half()
    r = K // 8
    X = ((torch.randn((2048, r), generator=gen) @ (torch.randn((r, K), generator=gen) / r ** 0.5) + 0.35 * torch.randn((2048, K), generator=gen))
         * torch.exp(0.8 * torch.randn(K, generator=gen))).half().to(DEV)
    H, _ = gptq.accumulate_hessian(None, 0, X)
    del X
    x = torch.randn((1, K), generator=gen).half().to(DEV)
    layers = {}
    for name, kw in (("plain", {}), ("act-order", dict(act_order=True)), ("act-order + static groups", dict(act_order=True, static_groups=True))):
        lin = torch.nn.Linear(K, N, bias=False).half()
        lin.weight.data = W.clone()
        layers[name] = gptq.quantize_linear(lin, H, 4, 128, device=DEV, **kw)
        with torch.no_grad():
            for _ in range(20):
                layers[name](x)
    torch.cuda.synchronize()
    times = {name: [] for name in layers}
    with torch.no_grad():
        for _ in range(3):
            for name, layer in layers.items():     # (alternating: the three share whatever else the machine is doing)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(calls):
                    layer(x)
                b.record()
                torch.cuda.synchronize()
                times[name].append(a.elapsed_time(b) / calls * 1e3)
    for name, layer in layers.items():
        act = layer._resolve_act_order()
        w = layer.native_descriptor(0) if act else layer.decode_descriptor()      # act-order: the row-sorted native copy behind the gather
        plan = ("column gather of x + " if act else "") + (ops.plan_describe([w], 1) if w is not None else "(no native copy)")
        t = times[name]
        print(f"forward M=1 N={N} K={K} w4 g128 {name}: {statistics.median(t):.2f} us per call [{min(t):.2f}..{max(t):.2f}]  act_order={act}  "
              f"loss {layer.gptq_loss:.4e}  plan: {plan}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4096x4096,4096x11008,11008x4096", help="NxK (out_features x in_features), comma-separated")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--no-loop", action="store_true")
    ap.add_argument("--static-groups", action="store_true", help="time qllm_gptq_quantize_static next to qllm_gptq_quantize, and the forward")
    a = ap.parse_args()
    info = _lib.device_info(0)
    print(f"device: {info['arch']} {info['compute_units']} CUs; torch {torch.__version__}")
    for shape in a.shapes.split(","):
        N, K = (int(v) for v in shape.split("x"))
        gen = torch.Generator().manual_seed(N + K)
        W = (0.02 * torch.randn((N, K), generator=gen)).half().to(DEV)
        r = K // 8
        X = ((torch.randn((2048, r), generator=gen) @ (torch.randn((r, K), generator=gen) / r ** 0.5) + 0.35 * torch.randn((2048, K), generator=gen))
             * torch.exp(0.8 * torch.randn(K, generator=gen))).half().to(DEV)
        H, _ = gptq.accumulate_hessian(None, 0, X)
        del X
        for act in (False, True):
            h = H.clone()
            w, perm = W, None
            if act:
                perm = torch.argsort(torch.diag(h), descending=True)
                w, h = W[:, perm].contiguous(), h[perm][:, perm]
            idx = torch.arange(K, device=DEV)
            h[idx, idx] += 0.01 * torch.mean(torch.diag(h))
            t_fac = timed(lambda: gptq._factor(h), a.repeats)
            U, where = t_fac[3]
            if a.static_groups:
                print(f"N={N} K={K} act_order={int(act)}: " + static_leg(W, w, U, perm, a.repeats), flush=True)
                continue
            t_k = timed(lambda: ops.gptq_quantize(w, U, 4, 128, False), a.repeats)
            t_rtn = timed(lambda: ops.gptq_quantize(w, None, 4, 128, False), a.repeats)
            n_wg, tri = (N + 15) // 16, sum(128 * min(128, K - c) * 4 for b in range(0, K, 128) for c in range(b, K, 128))
            line = (f"N={N} K={K} act_order={int(act)}: factorisation ({where}) {t_fac[0]:.2f} ms [{t_fac[1]:.2f}..{t_fac[2]:.2f}]  "
                    f"qllm_gptq_quantize {t_k[0]:.3f} ms [{t_k[1]:.3f}..{t_k[2]:.3f}]  (u=NULL {t_rtn[0]:.3f} ms)  "
                    f"U tiles streamed {tri / 2 ** 20:.0f} MiB x {n_wg} blocks = {tri * n_wg / 2 ** 30:.1f} GiB -> {tri * n_wg / t_k[0] / 1e9:.2f} TB/s")
            if not a.no_loop:
                t_l = timed(lambda: column_loop(w, U, 4, 128), 1)
                wq = t_k[3][3]
                diff = float((t_l[3].to(wq.dtype) != wq).float().mean())     # the loop's fp32 values, rounded as the kernel rounds its own
                line += f"  torch column loop {t_l[0]:.1f} ms = x{t_l[0] / t_k[0]:.0f}  (dequantized weights differing from the loop's: {diff:.3%})"
            print(line, flush=True)
    if a.static_groups:
        forward_leg()


if __name__ == "__main__":
    main()
