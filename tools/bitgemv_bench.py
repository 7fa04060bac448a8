#!/usr/bin/env python3
"""The bit-stream matvec (csrc/bitgemv.hip, round 6) against what served these widths until round 5: the library's dequant kernel + a
dense fp16 GEMM (the reference's branch (B), quant_linear_gptq.py:81-85).  Llama-2-7B shapes, HQQ g64 (HQQ's default widths include 2 and
8) and GPTQ g128, M = 1 / 4 / 16, hipGraph replay over rotating layer copies (HBM-cold).  Prints a markdown table.
    python tools/bitgemv_bench.py > profiles/r06_bitgemv.md
--act-order: the one-launch act-order decode (csrc/bitgemv_ao.hip) at 8 and 2 bits, M = 1 / 16 (and 7 bits, M = 16), against its
alternatives; the table of profiles/bitgemv_actorder.md.
    python tools/bitgemv_bench.py --act-order
    python tools/bitgemv_bench.py --act-order 2,5,8 1,2,4,8      (other widths / row counts: the table behind the module's rule)
--group: one grouped launch (csrc/bitgemv_group.hip) against the member launches one after the other, q/k/v, gate/up and a GQA triple;
the table of profiles/bitgemv_group.md and the row count behind QLLM_BITGROUP_MAX_M_DEFAULT.
    python tools/bitgemv_bench.py --group"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from qllm_amd import ops  # noqa: E402
from qllm_amd.modeling.q_layers import QuantLinearGPTQ, QuantLinearHQQ  # noqa: E402

dev = torch.device("cuda:0")
gen = torch.Generator(device=dev).manual_seed(3)


def act_order_leg(cases=((8, (1, 16)), (2, (1, 16)), (7, (16,))), rounds=7, window_ms=200.0):
    """(a) qllm_linear_forward_permuted on the row-sorted copy; (b) gather_columns + the plain matvec on it (two launches); (c) the plain
    matvec alone; (d) what served these layers before: dequant with g_idx + a dense GEMM.  (c) is the SORTED COPY fed an unpermuted x,
    not a separately built non-act-order layer: same kernel, same bytes, same time -- its numbers mean nothing.
    One process, hipGraph replay.  Every leg walks copies of ITS OWN (a / b / c never touch one another's weights, d reads the
    originals), >= 1 GiB of packed weights per leg at 8 bits and >= 512 MiB at 2 bits against 256 MiB of Infinity Cache, so no leg
    finds weights that it or the leg before it left there.  The order of the legs rotates round by round; every timed window is
    `window_ms` of replays at least (the count is set per leg from a trial).  Median (min .. max) per layer.
    7 bits x 16 rows is here for its own reason: its gathering form keeps one unit's words in flight where the plain twin (c) keeps two."""
    import statistics
    print("| bits | K | N | M | copies / leg | (a) one launch us | (b) gather + matvec us | (c) plain layer us | (d) dequant + GEMM us | (d)/(a) | (a)-(c) us | (a)-(b) us |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for bits, Ms in cases:
        for (K, N) in ((4096, 4096), (4096, 11008), (11008, 4096)):
            wbytes = K * N * bits // 8
            ncopy = min(128, ((1 << 30) + wbytes - 1) // wbytes)
            srt, orig, layers = {}, [], []   # (the layers own what the descriptors point to; d reads the originals of a's layers)
            for k in "abc":
                srt[k] = []
                for _ in range(ncopy):
                    l = bench.make_layer(QuantLinearGPTQ, K, N, dev, gen, act_order=True, bits=bits, group=128)
                    l._resolve_act_order()
                    layers.append(l)
                    srt[k].append(l._ao_descriptor(0))
                    if k == "a":
                        orig.append(l._descriptor(l.g_idx, 0))
            for M in Ms:
                x = torch.randn(M, K, device=dev, dtype=torch.float16)

                def leg_a():
                    for w, p in srt["a"]:
                        y = ops.linear_forward_permuted(w, p, x)
                    return y

                def leg_b():
                    for w, p in srt["b"]:
                        y = ops.linear_forward(w, ops.gather_columns(x, p))
                    return y

                def leg_c():
                    for w, _ in srt["c"]:
                        y = ops.linear_forward(w, x)
                    return y

                def leg_d():
                    for w in orig:
                        y = torch.matmul(x, ops.dequant(w, dev, torch.float16))
                    return y

                legs = {"a": leg_a, "b": leg_b, "c": leg_c, "d": leg_d}
                graphs = {k: bench.capture(fn)[0] for k, fn in legs.items()}
                iters = {k: max(5, int(window_ms / bench.time_events(gph.replay, 3, warm=2)) + 1) for k, gph in graphs.items()}
                t = {k: [] for k in legs}
                order = list(legs)
                for r in range(rounds):
                    for k in order[r % 4:] + order[:r % 4]:
                        t[k].append(bench.time_events(graphs[k].replay, iters[k], warm=2) / ncopy * 1e3)
                med = {k: statistics.median(v) for k, v in t.items()}
                cell = lambda k: f"{med[k]:.2f} ({min(t[k]):.2f} .. {max(t[k]):.2f})"  # noqa: E731
                print(f"| {bits} | {K} | {N} | {M} | {ncopy} | {cell('a')} | {cell('b')} | {cell('c')} | {cell('d')} | {med['d'] / med['a']:.1f}x | "
                      f"{med['a'] - med['c']:+.2f} | {med['a'] - med['b']:+.2f} |", flush=True)
                del graphs
            del srt, orig, layers
            torch.cuda.empty_cache()


def group_leg(widths=(2, 5, 8), Ms=(1, 2, 4, 8, 16), rounds=5, window_ms=60.0):
    """(a) ONE ops.linear_forward_bitgroup for the siblings; (b) their ops.linear_forward calls one after the other -- what served these
    groups before.  Same kernel body, same splits, same bits (tests/test_bitgemv_group_gpu.py): the difference is launch boundaries
    against how the members' blocks share the CUs.  One process, hipGraph replay over rotating copies of the group (>= 512 MiB of
    packed weights per pass, at most 64 groups, against 256 MiB of Infinity Cache: both legs walk the same copies, and a pass has
    evicted its own head before the next one starts).  The legs alternate round by round; every timed window is `window_ms` of
    replays at least.  Median (min .. max) per GROUP.  spread(a) = max - min of (a)'s windows: the noise a difference has to beat."""
    import statistics
    sets = (("q/k/v", 4096, (4096, 4096, 4096)), ("gate/up", 4096, (11008, 11008)), ("GQA q/k/v", 4096, (4096, 1024, 1024)))
    print("| bits | group | M | copies | geometry of (a) | (a) one launch us | (b) member launches us | (b)-(a) us | spread(a) us | (a) lost |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    lost_at = {}
    for bits in widths:
        for name, K, ns in sets:
            gbytes = sum(K * n * bits // 8 for n in ns)
            ncopy = max(4, min(64, ((512 << 20) + gbytes - 1) // gbytes))
            layers = [[bench.make_layer(QuantLinearGPTQ, K, n, dev, gen, bits=bits, group=128) for n in ns] for _ in range(ncopy)]
            groups = [[l.decode_descriptor() for l in grp] for grp in layers]
            for M in Ms:
                x = torch.randn(M, K, device=dev, dtype=torch.float16)

                def leg_a():
                    for descs in groups:
                        y = ops.linear_forward_bitgroup(descs, x)
                    return y

                def leg_b():
                    for descs in groups:
                        for w in descs:
                            y = ops.linear_forward(w, x)
                    return y

                legs = {"a": leg_a, "b": leg_b}
                graphs = {k: bench.capture(fn)[0] for k, fn in legs.items()}
                iters = {k: max(3, int(window_ms / bench.time_events(gph.replay, 2, warm=1)) + 1) for k, gph in graphs.items()}
                t = {k: [] for k in legs}
                for r in range(rounds):
                    for k in ("ab" if r % 2 == 0 else "ba"):
                        t[k].append(bench.time_events(graphs[k].replay, iters[k], warm=1) / ncopy * 1e3)
                med = {k: statistics.median(v) for k, v in t.items()}
                spread = max(t["a"]) - min(t["a"])
                lost = med["a"] - med["b"] > spread
                if lost:
                    lost_at.setdefault(M, []).append((bits, name))
                cell = lambda k: f"{med[k]:.2f} ({min(t[k]):.2f} .. {max(t[k]):.2f})"  # noqa: E731
                print(f"| {bits} | {name} | {M} | {ncopy} | {ops.bitgroup_describe(groups[0], M)[9:]} | {cell('a')} | {cell('b')} | "
                      f"{med['b'] - med['a']:+.2f} | {spread:.2f} | {'yes' if lost else ''} |", flush=True)
                del graphs
            del layers, groups
            torch.cuda.empty_cache()
    best = 0
    for M in Ms:   # the largest measured row count with no lost cell at it or below it
        if M in lost_at:
            break
        best = M
    print()
    print(f"cells where (a) lost: {lost_at if lost_at else 'none'}")
    print(f"largest measured row count up to which no cell lost: {best}")


if "--group" in sys.argv:
    group_leg()
    sys.exit(0)
if "--act-order" in sys.argv:
    # (--act-order BITS,.. ROWS,..: other widths and row counts, e.g. `--act-order 2,5,8 1,2,4,8` for the table behind the module's rule)
    extra = sys.argv[sys.argv.index("--act-order") + 1:]
    if extra:
        act_order_leg(tuple((int(b), tuple(int(m) for m in extra[1].split(","))) for b in extra[0].split(",")), rounds=5)
    else:
        act_order_leg()
    sys.exit(0)
print("| layout | bits | K | N | M | plan | fused us | GB/s (packed bytes) | of 8 TB/s | dequant + GEMM us | speed-up |")
print("|---|---|---|---|---|---|---|---|---|---|---|")
quick = "--quick" in sys.argv   # (A/B runs: HQQ only, widths 2 / 5 / 8, no dequant + GEMM leg)
for cls, g, zeros in ((QuantLinearHQQ, 64, "f16"),) if quick else ((QuantLinearHQQ, 64, "f16"), (QuantLinearGPTQ, 128, "packed")):
    for bits in (2, 5, 8) if quick else (2, 5, 6, 7, 8):
        for (K, N) in ((4096, 4096), (4096, 11008), (11008, 4096)):
            wbytes = K * N * bits // 8
            ncopy = max(2, min(24, (512 << 20) // wbytes + 1))
            layers = [bench.make_layer(cls, K, N, dev, gen, bits=bits, group=g) for _ in range(ncopy)]
            for M in (1, 4, 16):
                x = torch.randn(M, K, device=dev, dtype=torch.float16)
                res = {}
                for tag, on in (("fused", 1),) if quick else (("fused", 1), ("dequant", 0)):
                    ops.set_knob("QLLM_BITGEMV", on)
                    try:
                        plan = ops.plan_describe([layers[0].decode_descriptor()], M) if on else None
                        gph, _ = bench.capture(lambda: [l(x) for l in layers])
                        res[tag] = bench.time_events(gph.replay, 10, warm=3) / ncopy
                        del gph
                        if on:
                            res["plan"] = plan
                    finally:
                        ops.reset_knobs()
                G = K // g
                nbytes = wbytes + G * N * 2 + (G * N * 2 if zeros == "f16" else G * N * bits // 8) + 2 * M * K + 2 * M * N
                res.setdefault("dequant", float("nan"))
                print(f"| {cls.__name__[11:]} g{g} | {bits} | {K} | {N} | {M} | {res['plan']} | {res['fused'] * 1e3:.2f} | {nbytes / res['fused'] / 1e6:.0f} | "
                      f"{nbytes / res['fused'] / 1e6 / 8000:.3f} | {res['dequant'] * 1e3:.2f} | {res['dequant'] / res['fused']:.1f}x |", flush=True)
            del layers
            torch.cuda.empty_cache()
