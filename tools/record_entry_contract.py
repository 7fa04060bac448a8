#!/usr/bin/env python
"""Record what the host side of the C ABI answers: tests/golden/entry_contract.json, replayed by tests/test_entry_contract_cpu.py.

    python tools/record_entry_contract.py [--out tests/golden/entry_contract.json]

Every entry with a check of its own (the bit family, the grouped / fused-norm / describe entries around it) is called with fake,
aligned, never-dereferenced pointers (tests/capi_fakes.py) and one record is kept per call: entry, arguments, knob overrides, and the
status with the exact qllm_last_error() text, the describe text or the byte count.  A forward entry is recorded only with arguments the
library REFUSES (asserted here: nothing is written otherwise); describe and workspace-size entries, pure host code, also where they
serve.  Needs no GPU; geometry is recorded for 256 compute units (QLLM_NUM_CU is set before the library loads).  Run it on the commit
whose behaviour is to be pinned -- a refactoring of csrc/capi.hip is then checked by replaying the file, not by recording it again."""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
os.environ["QLLM_NUM_CU"] = "256"

import capi_fakes as F  # noqa: E402
from qllm_amd import _lib  # noqa: E402

AWQ, HQQ, NATIVE = _lib.LAYOUT_AWQ_GEMM, _lib.LAYOUT_HQQ, _lib.LAYOUT_NATIVE
CASES = []


def case(entry, knobs=None, **args):
    c = {"entry": entry, "args": args, **({"knobs": knobs} if knobs else {})}
    if c not in CASES:   # (the lists below overlap here and there)
        CASES.append(c)


def w(**fields):
    return [fields]


# what bitpanel_refusal / bitgemm_refusal / bitgemv_ok turn down, one descriptor per reason
MISALIGNED = [dict(qweight=F.QWEIGHT + 2), dict(scales=F.SCALES + 1), dict(qzeros=F.QZEROS + 2), dict(bias=3)]
PANEL_REFUSED = [dict(bits=4, layout=AWQ), dict(bits=4, layout=NATIVE), dict(K=1040), dict(g=48), dict(layout=HQQ, N=1001),
                 dict(layout=HQQ, qzeros=F.QZEROS + 2), dict(K=1 << 20), dict(K=1 << 20, N=64)] + MISALIGNED
GEMM_REFUSED = [dict(bits=4, layout=AWQ), dict(bits=4, layout=NATIVE), dict(K=4128), dict(g=48), dict(N=4100), dict(K=1 << 20)] + MISALIGNED
GEMV_REFUSED = [dict(bits=4, layout=AWQ), dict(bits=4, N=64, layout=NATIVE), dict(K=1040, g=1040), dict(g=48), dict(layout=HQQ, N=1001),
                dict(layout=HQQ, qzeros=F.QZEROS + 2), dict(qweight=F.QWEIGHT + 2), dict(scales=F.SCALES + 1), dict(K=1 << 20, N=8192)]
INVALID_LAYERS = [dict(qweight=None), dict(scales=None), dict(bits=9), dict(bits=1), dict(K=0), dict(g=4), dict(layout=7), dict(azb=2),
                  dict(K=4100, bits=5)]
# host-only served cases: every (bits, K, N, group size); the row counts cycle through them, the workspace flag alternates
SERVED = [dict(bits=b, K=k, N=n, g=(k if g == 0 else g)) for b, k, n, g in itertools.product((2, 7, 8), (256, 4096), (64, 4096), (32, 128, 0))]
ROW_EDGES = (17, 32, 33, 64, 65, 128, 129)


def single_layer_family(name, fwd_m, refused, rows_outside, rows_at_edges, served_rows, knob):
    """qllm_linear_forward_<name>, qllm_<name>_workspace_bytes, qllm_<name>_describe"""
    fwd, size, desc = f"qllm_linear_forward_{name}", f"qllm_{name}_workspace_bytes", f"qllm_{name}_describe"
    # the forward entry: refusals only
    case(fwd, w=None, m=fwd_m)
    for bad in INVALID_LAYERS:
        case(fwd, w=w(**bad), m=fwd_m)
    case(fwd, w=w(), m=fwd_m, x=None)
    case(fwd, w=w(), m=fwd_m, y=None)
    for m in (0, -1):
        case(fwd, w=w(), m=m)
    for dt in (7, _lib.DT_F32, -1):
        case(fwd, w=w(), m=fwd_m, dt=dt)
    case(fwd, w=w(), m=fwd_m, x=F.X + 8)
    case(fwd, w=w(), m=fwd_m, y=F.Y + 8, x=None)       # (a misaligned y alone is refused by bitgemm only: keep the call refused everywhere)
    case(fwd, w=w(g_idx=28672), m=fwd_m)
    case(fwd, {knob: 0}, w=w(), m=fwd_m)
    for m in rows_outside:
        case(fwd, w=w(), m=m)
    for bad in refused:
        case(fwd, w=w(**bad), m=fwd_m)
    # two faults at once: which check fires first
    case(fwd, w=w(), m=0, x=None)
    case(fwd, w=w(bits=9), m=fwd_m, x=None)
    case(fwd, w=w(), m=fwd_m, dt=7, x=F.X + 8)
    case(fwd, w=w(), m=-1, dt=7)
    case(fwd, {knob: 0}, w=w(g_idx=28672), m=fwd_m)
    case(fwd, {knob: 0}, w=w(), m=rows_outside[0])
    case(fwd, {knob: 0}, w=w(K=1040), m=fwd_m)
    case(fwd, w=w(g_idx=28672), m=fwd_m, dt=7)
    case(fwd, w=w(g_idx=28672), m=rows_outside[0])
    case(fwd, w=w(K=1040, g=48), m=rows_outside[0])
    case(fwd, w=w(bits=4, layout=AWQ, K=1040), m=fwd_m)
    # describe and the workspace size: the same refusals, and what they answer where the entry serves
    case(desc, w=w(), m=fwd_m, buf=False)
    case(desc, w=w(), m=fwd_m, buflen=0)
    case(desc, w=None, m=fwd_m)
    case(desc, w=w(bits=9), m=0)
    case(desc, w=w(), m=0, buf=False)
    for host in (desc, size):
        case(host, w=None, m=fwd_m)
        for bad in INVALID_LAYERS[:4]:
            case(host, w=w(**bad), m=fwd_m)
        for m in (0, -1) + tuple(rows_at_edges):
            case(host, w=w(), m=m)
        case(host, w=w(g_idx=28672), m=fwd_m)
        case(host, {knob: 0}, w=w(), m=fwd_m)
        case(host, {knob: 0}, w=w(g_idx=28672), m=fwd_m)
        case(host, {knob: 0}, w=w(), m=rows_outside[0])
        for bad in refused:
            case(host, w=w(**bad), m=fwd_m)
    for i, layer in enumerate(SERVED):
        m = served_rows[i % len(served_rows)]
        case(desc, w=[layer], m=m, have_ws=1 - i // len(served_rows) % 2)
        case(size, w=[layer], m=m)
    for m in ROW_EDGES + (256, 257, 512, 2048):
        for have_ws in (1, 0):
            case(desc, w=w(), m=m, have_ws=have_ws)
        case(size, w=w(bits=5, N=11008), m=m)


single_layer_family("bitpanel", 64, PANEL_REFUSED, (16, 513), (16, 17, 512, 513), ROW_EDGES, "QLLM_BITPANEL")
single_layer_family("bitgemm", 300, GEMM_REFUSED, (128, 1), (128, 129), (129, 257, 513, 2048), "QLLM_BITGEMM")
# bitgemm's own: the activation types, both alignments, the activations' 2 GiB
for args in (dict(dt=_lib.DT_BF16), dict(dt=_lib.DT_BF16, m=128), dict(dt=_lib.DT_BF16, x=F.X + 8), dict(y=F.Y + 8), dict(x=F.X + 8, y=F.Y + 8),
             dict(dt=_lib.DT_F16_IN_BF16_OUT, x=F.X + 8), dict(dt=_lib.DT_F16_IN_BF16_OUT, m=128)):
    case("qllm_linear_forward_bitgemm", w=w(), **{"m": 300, **args})
case("qllm_linear_forward_bitgemm", {"QLLM_BITGEMM": 0}, w=w(), m=300, dt=_lib.DT_BF16)
for host in ("qllm_linear_forward_bitgemm", "qllm_bitgemm_describe", "qllm_bitgemm_workspace_bytes"):
    case(host, w=w(K=65536, N=64), m=16385)
    case(host, w=w(K=65536, N=64, g=48), m=16385)

# ---- the grouped bit-stream entry --------------------------------------------------------------------------------------------------------
FWD, SIZE, DESC = "qllm_linear_forward_bitgroup", "qllm_bitgroup_workspace_bytes", "qllm_bitgroup_describe"
PAIR = [dict(), dict(N=1024)]
case(FWD, w=PAIR, ys=None)
case(FWD, w=None, n=2, ys=[F.Y, F.Y + F.Y_STRIDE])
case(FWD, w=None, n=2, ys=None)
case(FWD, w=PAIR, ys=None, n=0)
for n_layers in (1, 2, 3, 4, 5):
    case(FWD, w=[dict()] * n_layers, m=17)
case(FWD, w=PAIR, n=0)
case(FWD, w=[dict()] * 5)
case(FWD, w=PAIR, n=-1)
for bad in INVALID_LAYERS:
    case(FWD, w=[dict(), bad])
for m in (0, -1, 17, 64):
    case(FWD, w=PAIR, m=m)
case(FWD, w=PAIR, x=None)
case(FWD, w=PAIR, ys=[F.Y, None])
case(FWD, w=PAIR, ys=[None, F.Y])
case(FWD, w=PAIR, dt=7)
case(FWD, w=PAIR, x=F.X + 8)
DISAGREE = [dict(K=2048), dict(bits=5), dict(g=64), dict(azb=1)]
for other in DISAGREE:
    case(FWD, w=[dict(), other])
case(FWD, w=[dict(bits=4), dict(bits=4, layout=AWQ)])          # the layout family alone
case(FWD, w=[dict(bits=4, layout=NATIVE), dict(bits=4)])
case(FWD, w=[dict(), dict(g_idx=28672)])
case(FWD, w=[dict(g_idx=28672), dict()])
case(FWD, {"QLLM_BITGROUP": 0}, w=PAIR)
for bad in GEMV_REFUSED:
    case(FWD, w=[bad, bad])
    case(FWD, w=[bad])
case(FWD, w=[dict(), dict(layout=HQQ, N=1001)])
# two faults at once
case(FWD, w=PAIR, n=0, m=0)
case(FWD, w=PAIR, x=None, m=17)
case(FWD, w=PAIR, x=None, m=0)
case(FWD, w=[dict(), dict(bits=9)], m=0)
case(FWD, w=[dict(), dict(K=2048, g_idx=28672)])
case(FWD, w=[dict(), dict(K=2048)], m=0)
case(FWD, w=[dict(), dict(K=2048), dict(g_idx=28672)])
case(FWD, {"QLLM_BITGROUP": 0}, w=[dict(), dict(g_idx=28672)])
case(FWD, {"QLLM_BITGROUP": 0}, w=[dict(), dict(bits=5)])
case(FWD, {"QLLM_BITGROUP": 0}, w=PAIR, m=17)
case(FWD, {"QLLM_BITGROUP": 0}, w=PAIR, x=None)
case(FWD, w=[dict(K=1040, g=1040)] * 2, m=17)
case(DESC, w=PAIR, buf=False)
case(DESC, w=PAIR, buflen=0)
case(DESC, w=None, n=2, buf=False)
for host in (DESC, SIZE):
    case(host, w=None, n=2)
    case(host, w=PAIR, n=0)
    case(host, w=[dict()] * 5)
    case(host, w=[dict(), dict(bits=9)])
    for m in (0, -1, 16, 17):
        case(host, w=PAIR, m=m)
    for other in DISAGREE + [dict(g_idx=28672)]:
        case(host, w=[dict(), other])
    case(host, w=[dict(bits=4), dict(bits=4, layout=AWQ)])
    case(host, {"QLLM_BITGROUP": 0}, w=PAIR)
    case(host, {"QLLM_BITGROUP": 0}, w=PAIR, m=17)
    case(host, {"QLLM_BITGROUP": 0}, w=[dict(), dict(g_idx=28672)])
    case(host, {"QLLM_BITGROUP_MAX_M": 0}, w=PAIR, m=16)
    for bad in GEMV_REFUSED:
        case(host, w=[bad, bad])
    case(host, w=[dict(), dict(layout=HQQ)])
for i, layer in enumerate(SERVED):
    group = [layer, dict(layer, N=1024), dict(layer, N=64), layer][: 1 + i % 4]
    m = (1, 16, 2, 8)[i % 4]
    case(DESC, w=group, m=m, have_ws=1 - i // 4 % 2)
    case(SIZE, w=group, m=m)
for ns in ((4096, 4096, 4096), (11008, 11008), (4096, 1024, 1024), (1024, 4096, 1024)):
    for m in (1, 16):
        case(DESC, w=[dict(bits=5, N=n) for n in ns], m=m)
        case(SIZE, w=[dict(bits=5, N=n) for n in ns], m=m)

# ---- the gathering matvec (its parameter block is the plain matvec's) ----------------------------------------------------------------------
PERMUTED = "qllm_linear_forward_permuted"
for args in (dict(w=None), dict(w=w(bits=9)), dict(w=w(g_idx=28672)), dict(w=w(), perm=None), dict(w=w(), perm=F.PERM + 8), dict(w=w(), x=None),
             dict(w=w(), y=None), dict(w=w(), m=0), dict(w=w(), m=17), dict(w=w(), dt=7), dict(w=w(), x=F.X + 8), dict(w=w(K=1040, g=1040)),
             dict(w=w(bits=4, layout=AWQ)), dict(w=w(g_idx=28672), perm=None), dict(w=w(), perm=None, x=None), dict(w=w(), x=None, m=17)):
    case(PERMUTED, **args)
case(PERMUTED, {"QLLM_BITGEMV": 0}, w=w())
case(PERMUTED, {"QLLM_BITGEMV": 0}, w=w(), m=17)
case(PERMUTED, {"QLLM_BITGEMV": 0}, w=w(), x=None)

# ---- the planner's grouped entry and qllm_plan_describe --------------------------------------------------------------------------------------
GROUPED, PLAN = "qllm_linear_forward_grouped", "qllm_plan_describe"
Q4 = dict(bits=4)
case(GROUPED, w=None, n=2)
case(GROUPED, w=[Q4, Q4], ys=None)
case(GROUPED, w=None, n=2, ys=None)
case(GROUPED, w=[Q4, Q4], n=0)
case(GROUPED, w=[Q4] * 9)
case(GROUPED, w=[Q4, Q4], n=0, ys=None)
case(GROUPED, w=[Q4], x=None)                                    # a group of one is the plain call
case(GROUPED, w=[dict(bits=5)], m=64)
case(GROUPED, w=[dict(bits=9)])
for bad in INVALID_LAYERS:
    case(GROUPED, w=[Q4, bad])
case(GROUPED, w=[Q4, Q4], x=None)
case(GROUPED, w=[Q4, Q4], ys=[F.Y, None])
case(GROUPED, w=[Q4, Q4], ys=[None, F.Y])
for m in (0, -1):
    case(GROUPED, w=[Q4, Q4], m=m)
case(GROUPED, w=[Q4, Q4], dt=7)
case(GROUPED, w=[Q4, Q4], x=F.X + 8)
case(GROUPED, w=[Q4, dict(bits=9)], ys=[None, F.Y])              # layer by layer: the first layer's output before the second's descriptor
case(GROUPED, w=[Q4, dict(bits=9)], x=None)
case(GROUPED, w=[dict(bits=9), Q4], x=None)
case(GROUPED, w=[Q4, dict(bits=9)], ys=[F.Y, None])
case(GROUPED, w=[Q4, Q4], m=0, dt=7)
case(GROUPED, w=[dict(), dict(N=1024)])                          # 8 bits: the planner's refusal
case(GROUPED, w=[Q4, dict(bits=4, K=2048)])
case(GROUPED, w=[dict(bits=5), dict(bits=5)], m=64)
for args in (dict(w=None, n=1), dict(w=[Q4], buf=False), dict(w=[Q4], buflen=63), dict(w=[Q4], n=0), dict(w=[Q4] * 9), dict(w=[Q4], m=0),
             dict(w=[Q4], m=-1), dict(w=[Q4, dict(bits=9)]), dict(w=[Q4], n=0, m=0), dict(w=[dict(bits=9)], m=0), dict(w=None, n=0),
             dict(w=[Q4, dict(bits=4, K=2048)]), dict(w=[Q4, dict(bits=4, g=64)])):
    case(PLAN, **args)
for layers in ([Q4], [Q4, Q4], [dict()], [dict(bits=5)], [dict(), dict(N=1024)], [dict(bits=4, layout=NATIVE)], [dict(bits=4, layout=NATIVE)] * 3):
    for m in (1, 16, 64, 300):
        case(PLAN, w=layers, m=m, have_ws=1)
    case(PLAN, w=layers, m=300, have_ws=0)

# ---- the fused RMSNorm launch and the two "refused: " describe entries -----------------------------------------------------------------------
NORM, NORM_DESC, SWIGLU_DESC = "qllm_linear_forward_rmsnorm", "qllm_rmsnorm_describe", "qllm_swiglu_describe"
G2 = [Q4, Q4]                                                    # GPTQ layout: decide_rmsnorm refuses it, nothing is ever launched
case(NORM, w=None, n=2)
case(NORM, w=G2, ys=None)
case(NORM, w=G2, n=0)
case(NORM, w=[Q4] * 9)
case(NORM, w=G2, norm_weight=None)
case(NORM, w=G2, n=0, norm_weight=None)
case(NORM, w=G2, ys=None, norm_weight=None)
for bad in INVALID_LAYERS:
    case(NORM, w=[Q4, bad])
case(NORM, w=G2, x=None)
case(NORM, w=G2, ys=[F.Y, None])
for m in (0, -1, 2):
    case(NORM, w=G2, m=m)
case(NORM, w=G2, dt=7)
case(NORM, w=G2, x=F.X + 8)
case(NORM, w=G2, ys=[F.Y, F.X])
case(NORM, w=G2, ys=[F.NORM_WEIGHT, F.Y])
case(NORM, w=G2, norm_weight=F.NORM_WEIGHT + 8)
case(NORM, w=G2, rstd=F.RSTD + 2)
case(NORM, w=G2, eps=-1.0)
case(NORM, w=[dict(K=36, g=36), dict(K=36, g=36)])
case(NORM, w=G2)
case(NORM, w=[Q4])
case(NORM, w=[dict(bits=4, layout=NATIVE), Q4])
case(NORM, w=[dict(bits=4, layout=NATIVE), dict(bits=4, layout=NATIVE, K=2048)])
case(NORM, w=[dict(bits=4, layout=NATIVE)] * 2, m=2)
case(NORM, w=[dict(bits=4, layout=NATIVE, g=32)] * 2)
# two faults at once
case(NORM, w=[Q4, dict(bits=9)], ys=[F.X, F.Y])                  # layer by layer: the first layer's alias before the second's descriptor
case(NORM, w=[Q4, dict(bits=9)], ys=[None, F.Y])
case(NORM, w=[Q4, dict(bits=9)], norm_weight=None)
case(NORM, w=G2, ys=[F.Y, F.X], norm_weight=F.NORM_WEIGHT + 8)
case(NORM, w=G2, norm_weight=F.NORM_WEIGHT + 8, rstd=F.RSTD + 2)
case(NORM, w=G2, rstd=F.RSTD + 2, eps=-1.0)
case(NORM, w=[dict(K=36, g=36)] * 2, eps=-1.0)
case(NORM, w=[dict(K=36, g=36)] * 2, m=2)
NATIVE4 = dict(bits=4, layout=NATIVE)
for args in (dict(w=None, n=1), dict(w=[NATIVE4], buf=False), dict(w=[NATIVE4], buflen=63), dict(w=[NATIVE4], n=0), dict(w=[NATIVE4] * 9),
             dict(w=[NATIVE4], m=0), dict(w=[NATIVE4], m=-1), dict(w=[NATIVE4, dict(bits=9)]), dict(w=[NATIVE4], n=0, m=0),
             dict(w=[dict(bits=9)], m=0), dict(w=[NATIVE4, dict(bits=4, layout=NATIVE, N=40)]), dict(w=[dict(bits=9), dict(bits=4, layout=NATIVE, N=40)]),
             dict(w=[NATIVE4], m=2), dict(w=G2), dict(w=[NATIVE4, Q4]), dict(w=[NATIVE4, dict(NATIVE4, K=2048)]), dict(w=[NATIVE4, dict(NATIVE4, g=64)]),
             dict(w=[dict(NATIVE4, g=32)] * 2), dict(w=[NATIVE4]), dict(w=[NATIVE4] * 2), dict(w=[NATIVE4, dict(NATIVE4, N=11008), dict(NATIVE4, N=1024)]),
             dict(w=[dict(NATIVE4, g=64)] * 2), dict(w=[dict(bits=3, layout=NATIVE)] * 2), dict(w=[dict(NATIVE4, K=11008)])):
    case(NORM_DESC, **args)
case(NORM_DESC, {"QLLM_STRIP1": 0}, w=[NATIVE4] * 2)
for args in (dict(w=None), dict(w=[NATIVE4], buf=False), dict(w=[NATIVE4], buflen=63), dict(w=[NATIVE4], m=0), dict(w=[NATIVE4], m=-1),
             dict(w=[dict(bits=9)]), dict(w=[dict(bits=9)], m=0), dict(w=None, m=0), dict(w=[dict(bits=4, layout=NATIVE, N=40)]), dict(w=[Q4]),
             dict(w=[dict()]), dict(w=[NATIVE4]), dict(w=[NATIVE4], m=2), dict(w=[NATIVE4], m=4), dict(w=[NATIVE4], m=5),
             dict(w=[dict(NATIVE4, g=64)]), dict(w=[dict(NATIVE4, g=64)], m=2), dict(w=[dict(bits=3, layout=NATIVE)]), dict(w=[dict(NATIVE4, K=11008)])):
    case(SWIGLU_DESC, **args)
case(SWIGLU_DESC, {"QLLM_STRIP1": 0}, w=[NATIVE4])

# ---- the column gather: what the entry refuses, and every form its rule can answer ----------------------------------------------------------
GATHER, GATHER_DESC = "qllm_gather_columns", "qllm_gather_describe"
for args in (dict(x=None), dict(perm=None), dict(y=None), dict(m=-1), dict(k=0), dict(dt=7), dict(x=F.X + 8), dict(perm=F.PERM + 8), dict(y=F.Y + 8),
             dict(y=F.X), dict(k=12), dict(k=28680), dict(k=4), dict(m=-1, x=None), dict(m=-1, dt=7), dict(k=12, dt=7), dict(k=12, y=F.X),
             dict(k=12, m=0), dict(k=12, x=F.X + 8)):
    case(GATHER, **args)
for args in (dict(buf=False), dict(buflen=0), dict(m=-1), dict(k=0), dict(k=-8), dict(m=-1, buf=False), dict(k=12), dict(k=28680), dict(k=12, m=-1),
             dict(m=0), dict(m=0, k=12)):
    case(GATHER_DESC, **args)
for k in (8, 264, 4096, 4104, 8192, 8200, 12288, 12296, 16384, 16392, 24576, 28672):
    for m in (1, 2, 3, 15, 31, 63, 64, 65, 300, 1027, 2047, 2048, 2050, 4095, 4099, 16390):
        case(GATHER_DESC, m=m, k=k)
        if m >= 64:
            case(GATHER_DESC, {"QLLM_GATHER_ROWS": 0}, m=m, k=k)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "entry_contract.json"))
    out = ap.parse_args().out
    lib = _lib.load()
    records = []
    for c in CASES:
        got = F.call_with_knobs(lib, c["entry"], c["args"], c.get("knobs"))
        if c["entry"] in F.FORWARD_ENTRIES:   # only what is refused before any device work
            assert got["rc"] in (_lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_WORKSPACE), (c, got)
        records.append({**c, "got": got})
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r, sort_keys=True) for r in records) + "\n]\n")
    print(f"{len(records)} records -> {out}")


if __name__ == "__main__":
    main()
