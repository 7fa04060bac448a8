#!/usr/bin/env python3
"""The fused mid-batch kernel (csrc/bitpanel.hip, ops.linear_forward_bitpanel) against what served these calls before it: the library's
dequant kernel + a dense fp16 GEMM (the modules' fallback, the reference's branch (B), quant_linear_gptq.py:81-85).  Llama-2-7B shapes,
GPTQ g128, 2 / 5 / 6 / 7 / 8 bits, M = 17 .. 512, plus 8-bit act-order layers (gather_columns + the kernel on the row-sorted copy against
dequant with g_idx + GEMM).  Prints the markdown table of profiles/bitpanel.md and, per row count, the smallest speed-up over all shapes
and widths -- the line QLLM_BITPANEL_MAX_M is set from.
    python tools/bitpanel_bench.py                      (everything)
    python tools/bitpanel_bench.py 2,8 17,64            (widths, row counts)
    python tools/bitpanel_bench.py --act-order          (the 8-bit act-order rows only)
    python tools/bitpanel_bench.py --ingest [2,8 17,64] (A/B of the kernel's two ingests of the packed words: straight into registers, the
                                                         default, against staged through LDS, QLLM_BITPANEL_LDS = 1; same method)
Method: one process, hipGraph replay; the two legs walk weight copies of their OWN (320 MiB of packed words per leg where 48 copies
reach that, against 256 MiB of Infinity Cache: 2-bit 4096 x 4096 layers stay at 192 MiB and are partly warm for both legs), their order
alternates round by round, every timed window is `window_ms` of replays at least; median (min .. max) of the rounds, per layer."""
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


def run(bits_list, rows, act_order, rounds=5, window_ms=80.0):
    worst = {m: (float("inf"), None) for m in rows}
    print("| layer | bits | K | N | M | geometry | copies / leg | fused us | dequant + GEMM us | speed-up |")
    print("|---|---|---|---|---|---|---|---|---|---|")
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
                        leg.append(l._ao_descriptor(0) if leg is new else l._descriptor(l.g_idx, 0))
                    else:
                        leg.append(l._descriptor(None, 0))
            for M in rows:
                x = torch.randn(M, K, device=dev, dtype=torch.float16)

                def leg_new():
                    for w in new:
                        y = ops.linear_forward_bitpanel(w[0], ops.gather_columns(x, w[1])) if act_order else ops.linear_forward_bitpanel(w, x)
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
                cell = lambda k: f"{med[k]:.2f} ({min(t[k]):.2f} .. {max(t[k]):.2f})"  # noqa: E731
                geo = ops.bitpanel_describe(new[0][0] if act_order else new[0], M).replace("bitpanel ", "").replace(f"bits={bits} cols=64 ", "")
                speed = med["old"] / med["new"]
                if speed < worst[M][0]:
                    worst[M] = (speed, f"{bits} bits {K} x {N}{' act-order' if act_order else ''}")
                print(f"| {'act-order' if act_order else 'plain'} | {bits} | {K} | {N} | {M} | {geo} | {ncopy} | {cell('new')} | {cell('old')} | {speed:.2f}x |",
                      flush=True)
                del graphs
            del new, old, layers
            torch.cuda.empty_cache()
    print()
    print("| M | smallest speed-up | where |")
    print("|---|---|---|")
    for m in rows:
        print(f"| {m} | {worst[m][0]:.2f}x | {worst[m][1]} |")
    print(flush=True)


def run_ingest(bits_list, rows, rounds=5, window_ms=80.0):
    """The same layers through the two ingests: one graph each (the knob is read when the call is made, so it is part of the capture)."""
    print("| bits | K | N | M | geometry | copies / leg | direct loads us | LDS-staged us | LDS / direct |")
    print("|---|---|---|---|---|---|---|---|---|")
    for bits in bits_list:
        for (K, N) in SHAPES:
            wbytes = K * N * bits // 8
            ncopy = max(2, min(48, ((320 << 20) + wbytes - 1) // wbytes))
            layers = {k: [bench.make_layer(QuantLinearGPTQ, K, N, dev, gen, bits=bits, group=128) for _ in range(ncopy)] for k in ("direct", "lds")}
            descs = {k: [l._descriptor(None, 0) for l in v] for k, v in layers.items()}
            for M in rows:
                x = torch.randn(M, K, device=dev, dtype=torch.float16)
                graphs = {}
                for k in descs:
                    ops.set_knob("QLLM_BITPANEL_LDS", 1 if k == "lds" else 0)
                    try:
                        graphs[k] = bench.capture(lambda k=k: [ops.linear_forward_bitpanel(w, x) for w in descs[k]][-1])[0]
                    finally:
                        ops.reset_knobs()
                iters = {k: max(3, int(window_ms / bench.time_events(g.replay, 2, warm=1)) + 1) for k, g in graphs.items()}
                t = {k: [] for k in graphs}
                for r in range(rounds):
                    for k in (("direct", "lds") if r % 2 == 0 else ("lds", "direct")):
                        t[k].append(bench.time_events(graphs[k].replay, iters[k], warm=1) / ncopy * 1e3)
                med = {k: statistics.median(v) for k, v in t.items()}
                cell = lambda k: f"{med[k]:.2f} ({min(t[k]):.2f} .. {max(t[k]):.2f})"  # noqa: E731
                geo = ops.bitpanel_describe(descs["direct"][0], M).replace("bitpanel ", "").replace(f"bits={bits} cols=64 ", "")
                print(f"| {bits} | {K} | {N} | {M} | {geo} | {ncopy} | {cell('direct')} | {cell('lds')} | {med['lds'] / med['direct']:.2f} |", flush=True)
                del graphs
            del layers, descs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    bits_list = tuple(int(b) for b in args[0].split(",")) if args else (2, 5, 6, 7, 8)
    rows = tuple(int(m) for m in args[1].split(",")) if len(args) > 1 else (17, 32, 64, 128, 256, 512)
    if "--ingest" in sys.argv:
        run_ingest(bits_list, rows)
    elif "--act-order" in sys.argv:
        run((8,), rows, True)
    else:
        run(bits_list, rows, False)
        if not args:
            run((8,), rows, True)
