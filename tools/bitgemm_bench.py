#!/usr/bin/env python3
"""The fused 2..8-bit prefill kernel (csrc/bitgemm.hip, ops.linear_forward_bitgemm) against what served these calls before it: the
library's dequant kernel + a dense fp16 GEMM (the modules' fallback, the reference's branch (B), quant_linear_gptq.py:81-85).
Llama-2-7B shapes, GPTQ g128, 2 / 5 / 6 / 7 / 8 bits, M = 257 .. 4096, plus 8-bit act-order layers (gather_columns + the kernel on the
row-sorted copy -- the gather is inside the fused leg -- against dequant with g_idx + GEMM).  Prints the markdown table of
profiles/bitgemm.md with the fused leg's TFLOP/s, per row count the smallest speed-up over all shapes and widths, and the line
QLLM_BITGEMM_MIN_M_DEFAULT follows from them.
    python tools/bitgemm_bench.py                      (everything)
    python tools/bitgemm_bench.py 2,8 257,2048         (widths, row counts)
    python tools/bitgemm_bench.py --act-order          (the 8-bit act-order rows only)
Method (tools/bitpanel_bench.py's): one process, hipGraph replay; the two legs walk weight copies of their OWN (320 MiB of packed words
per leg where 48 copies reach that, against 256 MiB of Infinity Cache), their order alternates round by round, every timed window is
`window_ms` of replays at least; median (min .. max) of the rounds, per layer."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import QuantLinearGPTQ  # noqa: E402

dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(5)
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096))
MARGIN = 1.05   # boxes differ by +-1.5 %: the fused call has to win by 5 % (the rule of profiles/bitpanel.md)


def run(bits_list, rows, act_order, worst, rounds=5, window_ms=80.0):
    print("| layer | bits | K | N | M | geometry | copies / leg | fused us | fused TFLOP/s | dequant + GEMM us | speed-up |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for bits in bits_list:
        for (K, N) in SHAPES:
            wbytes = K * N * bits // 8
            ncopy = max(2, min(48, ((320 << 20) + wbytes - 1) // wbytes))
            new, old, layers = [], [], []
            for leg in (new, old):
                for _ in range(ncopy):
                    l = bench.make_layer(QuantLinearGPTQ, K, N, dev, gen, act_order=act_order, bits=bits, group=128)
                    layers.append(l)
                    if act_order:
                        l._resolve_act_order()
                        leg.append(l._ao_descriptor(0, mid_batch=True) if leg is new else l._descriptor(l.g_idx, 0))
                    else:
                        leg.append(l._descriptor(None, 0))
            for M in rows:
                x = torch.randn(M, K, device=dev, dtype=torch.float16)

                def leg_new():
                    for w in new:
                        y = ops.linear_forward_bitgemm(w[0], ops.gather_columns(x, w[1])) if act_order else ops.linear_forward_bitgemm(w, x)
                    return y

                def leg_old():
                    for w in old:
                        y = torch.matmul(x, ops.dequant(w, dev, torch.float16))
                    return y

                legs = {"new": leg_new, "old": leg_old}
                graphs = {k: bench.capture(fn)[0] for k, fn in legs.items()}
                iters = {k: max(3, int(window_ms / bench.time_events(g.replay, 2, warm=1)) + 1) for k, g in graphs.items()}
                t = {k: [] for k in legs}
                for r in range(rounds):
                    for k in (("new", "old") if r % 2 == 0 else ("old", "new")):
                        t[k].append(bench.time_events(graphs[k].replay, iters[k], warm=1) / ncopy * 1e3)
                med = {k: statistics.median(v) for k, v in t.items()}
                cell = lambda k: f"{med[k]:.1f} ({min(t[k]):.1f} .. {max(t[k]):.1f})"  # noqa: E731
                geo = ops.bitgemm_describe(new[0][0] if act_order else new[0], M).replace("bitgemm ", "").replace(f"bits={bits} tile=256x128 ", "")
                speed = med["old"] / med["new"]
                if speed < worst.setdefault(M, (float("inf"), None))[0]:
                    worst[M] = (speed, f"{bits} bits {K} x {N}{' act-order' if act_order else ''}")
                print(f"| {'act-order' if act_order else 'plain'} | {bits} | {K} | {N} | {M} | {geo} | {ncopy} | {cell('new')} | "
                      f"{2.0 * M * K * N / med['new'] * 1e-6:.0f} | {cell('old')} | {speed:.2f}x |", flush=True)
                del graphs
            del new, old, layers
            torch.cuda.empty_cache()
    print(flush=True)


def summary(worst):
    print("| M | smallest speed-up | where |")
    print("|---|---|---|")
    for m in sorted(worst):
        print(f"| {m} | {worst[m][0]:.2f}x | {worst[m][1]} |")
    line = 0
    for m in sorted(worst, reverse=True):   # the smallest measured M from which every larger measured M wins by the margin too
        if m < 257 or worst[m][0] < MARGIN:
            break
        line = m
    print(f"\nQLLM_BITGEMM_MIN_M_DEFAULT by the rule (>= {MARGIN:.2f}x on every shape and width at that M and every larger measured M): {line}", flush=True)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bits_list = tuple(int(b) for b in args[0].split(",")) if args else (2, 5, 6, 7, 8)
    rows = tuple(int(m) for m in args[1].split(",")) if len(args) > 1 else (257, 512, 1024, 2048, 4096)
    worst = {}
    if "--act-order" in sys.argv:
        run((8,), rows, True, worst)
    else:
        run(bits_list, rows, False, worst)
        if not args:
            run((8,), rows, True, worst)
    summary(worst)
