"""Outputs of the batch-1 decode kernel (csrc/strip1_kernel.hpp) as bit-exact fixtures: tests/golden/strip1_parent/<case>.npz.

Run on the MI355X at the commit whose results are to be pinned (python tools/make_strip1_fixtures.py [out_dir]);
tests/test_strip1_bitstable_gpu.py regenerates the same inputs from the seeds below and asserts torch.equal against the stored outputs.
Only outputs are stored (fp16 / bf16 bit patterns as uint16); weights and activations are drawn through gpu_util.synth / randx.

A case is one set of weights; its file holds one array per variant key "<act>_b<bias>_c<add_zero_bias>"."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT_DIR = os.path.join(ROOT, "tests", "golden", "strip1_parent")
DEV = "cuda:0"

# (K, N, plan line prefix after "strip1 "): the smallest shapes that reach each form of the 4-bit g128 table
G128 = [(256, 64, "nw=4 round=8 grid"), (1024, 64, "nw=4 round=8 exact grid"), (2048, 64, "nw=4 round=16 exact grid"),
        (4096, 64, "nw=4 round=32 exact grid"),                                          # two 16-byte chunks of x per lane
        (4096, 4112, "nw=8 round=16 exact grid"), (5120, 4112, "nw=8 round=24 grid"),    # 257 strips: more blocks than CUs
        (11008, 64, "nw=15 round=24 grid")]
ZKS = {"packed": ("GPTQ", "asym"), "f16": ("HQQ", "asym"), "sym": ("GPTQ", "sym")}


def cases():
    """[(name, spec)]: spec = dict(kind, bits, g, K, widths, zk, M, plan, compats)"""
    out = []
    for K, N, plan in G128:
        for zk in ZKS:
            out.append(("g128_k%d_n%d_%s" % (K, N, zk), dict(bits=4, g=128, K=K, widths=(N,), zk=zk, M=1, plan="strip1 " + plan,
                                                              compats=(0, 1) if zk == "packed" else (0,))))
    out.append(("grouped_k1024", dict(bits=4, g=128, K=1024, widths=(16, 48, 32), zk="packed", M=1,
                                      plan="strip1 nw=4 round=8 exact grid=strips x 3", compats=(0, 1))))
    for K, plan in ((256, "nw=4 round=8 g64 grid"), (4096, "nw=4 round=32 exact g64 grid")):
        for zk in ZKS:
            out.append(("g64_k%d_%s" % (K, zk), dict(bits=4, g=64, K=K, widths=(64,), zk=zk, M=1, plan="strip1 " + plan, compats=(0,))))
    for zk in ("packed", "f16"):
        out.append(("rows4_k1152_m3_%s" % zk, dict(bits=4, g=128, K=1152, widths=(64,), zk=zk, M=3, plan="strip1 nw=4 round=16 rows=4 grid",
                                                   compats=(0,))))
    for g, plan in ((128, "nw=4 round=8 exact bits=3 grid"), (64, "nw=4 round=8 exact g64 bits=3 grid")):
        for zk in ZKS:
            out.append(("b3_g%d_k1024_%s" % (g, zk), dict(bits=3, g=g, K=1024, widths=(64,), zk=zk, M=1, plan="strip1 " + plan, compats=(0,))))
    return out


def _seed(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) % 100003


def run_case(name, spec):
    """{variant key: uint16 array [M, sum(widths)]} from the kernel, after asserting the case's plan line."""
    from gpu_util import randx, synth, to_layer
    from qllm_amd import ops
    layout, zkind = ZKS[spec["zk"]]
    K, M, seed = spec["K"], spec["M"], _seed(name)
    ds = [synth(layout, spec["bits"], spec["g"], K, n, zkind, False, True, seed=seed + 7 * i) for i, n in enumerate(spec["widths"])]
    x = torch.from_numpy(randx(M, K, seed=seed + 1)).to(DEV)
    res = {}
    for bias in (1, 0):
        if not bias:
            ds = [dict(d, bias=None) for d in ds]      # (the bias is synth's last draw: same weights without it)
        layers = [to_layer(d, DEV) for d in ds]
        for compat in spec["compats"]:
            keep = []
            if spec["zk"] == "sym":
                ws = []
                for l, d in zip(layers, ds):
                    l._descriptor(None, 0)
                    src = ops.make_weight("GPTQ", l.qweight, l.scales, None, None, l.bias, K, d["N"], spec["g"], spec["bits"], compat)
                    w, k = ops.repack_native(*src)[0:2]
                    ws.append(w)
                    keep.append((src, k))
            else:
                ws = [l.native_descriptor(compat) for l in layers]
            line = ops.plan_describe(ws, M)
            assert line.startswith(spec["plan"]), (name, line)
            for act, xt in (("f16", x), ("bf16", x.to(torch.bfloat16))):
                ys = ops.linear_forward_grouped(ws, xt) if len(ws) > 1 else [ops.linear_forward(ws[0], xt)]
                y = torch.cat([t.view(M, -1) for t in ys], dim=1)
                assert y.dtype == xt.dtype
                res["%s_b%d_c%d" % (act, bias, compat)] = y.view(torch.int16).cpu().numpy().view(np.uint16)
    return res


def main():
    out_dir = sys.argv[1] if len(sys.argv) > 1 else OUT_DIR
    os.makedirs(out_dir, exist_ok=True)
    bad = []
    for name, spec in cases():
        try:
            np.savez(os.path.join(out_dir, name + ".npz"), **run_case(name, spec))
            print("wrote", name, flush=True)
        except AssertionError as e:   # (a plan line that is not the case's: report every one, write nothing for it)
            bad.append(name)
            print("FAILED", name, e, flush=True)
    if bad:
        sys.exit("cases not written: " + " ".join(bad))


if __name__ == "__main__":
    main()
