#!/usr/bin/env python3
"""The planner's decisions as a table: one line per (descriptor, grouping, M, workspace) with the status of qllm_plan_describe, the plan
text (or qllm_last_error()) and, for single layers, qllm_workspace_bytes_act for fp16 and bf16 activations.  Pure host code: fake
aligned pointers, no GPU.  A change that is meant to leave every plan alone is checked by running this on the build before and the
build after and diffing the two outputs:

    python tools/plan_table.py --out before.txt [--lib path/to/libqllm_mi355x.so]

Descriptors that validation rejects stay in the table with their status and text.  The line count and the sha256 of the table go to
stderr."""
import argparse
import ctypes as C
import hashlib
import os
import sys

LAYOUTS = ("GPTQ", "AWQ", "HQQ", "NATIVE", "F16Z")   # the values of QLLM_LAYOUT_*, in order
GPTQ, AWQ, HQQ, NATIVE, F16Z = range(5)
BITS = (2, 3, 4, 8)
GROUPS = (32, 64, 128, 256)
SHAPES = ((4096, 4096), (4096, 11008), (11008, 4096), (4096, 1024), (8192, 1024), (8192, 28672), (28672, 8192), (5120, 13824),
          (4544, 4672), (18176, 4544), (1088, 320), (18944, 3584), (36864, 1024), (2112, 4096), (65536, 65536), (4096, 4000),
          (4096, 64), (128, 4096))
MS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 48, 64, 65, 100, 128, 129, 256, 300, 383, 384, 512, 767, 768, 1024, 2048, 2304, 8192)
# fake, aligned device pointers: nothing here dereferences them
QWEIGHT, SCALES, QZEROS, G_IDX = 0x10000, 0x20000, 0x30000, 0x40000
# the second layer of a pair: the same storage family with the other kind of zero points / the other family
ZERO_SIBLING = {GPTQ: HQQ, AWQ: GPTQ, HQQ: GPTQ, NATIVE: F16Z, F16Z: NATIVE}
OTHER_FAMILY = {GPTQ: NATIVE, AWQ: NATIVE, HQQ: F16Z, NATIVE: GPTQ, F16Z: HQQ}
# every settable planner threshold with one non-default value inside its range
KNOBS = (("QLLM_STRIP1_3BIT", 0), ("QLLM_STRIP1_MAX_M", 1), ("QLLM_STRIP1", 0), ("QLLM_STRIP1", 2), ("QLLM_PANEL", 0),
         ("QLLM_PANEL_MIN_M", 33), ("QLLM_PANEL_GROUP_MIN_M", 33), ("QLLM_GEMM2", 0), ("QLLM_GEMM3", 0), ("QLLM_GEMM2_MIN_M", 129),
         ("QLLM_GEMM3_MIN_M", 256), ("QLLM_GEMM2_SPLITK", 0), ("QLLM_GEMM3_TAIL", 0), ("QLLM_GEMM3_GROUP", 0), ("QLLM_GEMM3_BF16", 0),
         ("QLLM_SKINNY_MAX_M", 16), ("QLLM_STRIP_MIN", 512), ("QLLM_BITGEMV", 0))
LLAMA7B = ((4096, 4096), (4096, 11008), (11008, 4096))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", help="the library to ask (default: the one in the package directory)")
    ap.add_argument("--out", help="write the table here (default: standard output)")
    args = ap.parse_args()
    if args.lib:
        os.environ["QLLM_MI355X_LIB"] = os.path.abspath(args.lib)
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from qllm_amd import _lib

    lib = _lib.load()
    out = open(args.out, "w") if args.out else sys.stdout
    sha, lines = hashlib.sha256(), 0
    buf = C.create_string_buffer(512)
    describe, ws_bytes, last_error = lib.qllm_plan_describe, lib.qllm_workspace_bytes_act, lib.qllm_last_error

    def layer(layout, bits, g, zeros, gidx, K, N):
        needs_zeros = layout in (AWQ, HQQ, F16Z)
        return _lib.QllmWeight(QWEIGHT, SCALES, QZEROS if (zeros or needs_zeros) else None, G_IDX if gidx else None, None, K, N, g, bits, layout, 0)

    def emit(tag, ws):
        nonlocal lines
        arr = (_lib.QllmWeight * len(ws))(*ws)
        chunk = []
        for m in MS:
            sizes = ""
            if len(ws) == 1:
                sizes = " ws_f16=%d ws_bf16=%d" % (ws_bytes(arr, m, _lib.DT_F16), ws_bytes(arr, m, _lib.DT_BF16))
            for have in (0, 1):
                rc = describe(arr, len(ws), m, have, buf, 512)
                text = buf.value.decode() if rc == 0 else last_error().decode()
                chunk.append("%s M=%d ws=%d rc=%d %s%s\n" % (tag, m, have, rc, text, sizes))
        data = "".join(chunk)
        sha.update(data.encode())
        out.write(data)
        lines += len(chunk)

    def groupings(layout, bits, g, zeros, gidx, K, N):
        w = layer(layout, bits, g, zeros, gidx, K, N)
        yield "single", [w]
        yield "x2", [w, w]
        yield "x3", [w, w, w]
        yield "gqa", [w, layer(layout, bits, g, zeros, gidx, K, N // 4), layer(layout, bits, g, zeros, gidx, K, N // 4)]
        yield "zero-pair", [w, layer(ZERO_SIBLING[layout], bits, g, zeros, gidx, K, N)]
        yield "mixed-pair", [w, layer(OTHER_FAMILY[layout], bits, g, zeros, gidx, K, N)]

    # ---- section 1: the product of the descriptor axes -------------------------------------------------------------------------
    for layout in range(5):
        for bits in BITS:
            for g in GROUPS:
                for zeros in (1, 0):
                    for gidx in (0, 1):
                        for K, N in SHAPES:
                            for name, ws in groupings(layout, bits, g, zeros, gidx, K, N):
                                emit("%s b%d g%d z%d a%d %dx%d %s" % (LAYOUTS[layout], bits, g, zeros, gidx, K, N, name), ws)
    # ---- section 2: every settable threshold moved once, on the Llama-2-7B shapes -----------------------------------------------
    for knob, value in KNOBS:
        lib.qllm_reset_knobs()
        rc = lib.qllm_set_knob(knob.encode(), value)
        for layout in (GPTQ, HQQ, NATIVE, F16Z):
            for bits in (3, 4, 8):
                for g in (64, 128):
                    for K, N in LLAMA7B:
                        for name, ws in groupings(layout, bits, g, 1, 0, K, N):
                            emit("%s=%d(rc=%d) %s b%d g%d %dx%d %s" % (knob, value, rc, LAYOUTS[layout], bits, g, K, N, name), ws)
    lib.qllm_reset_knobs()
    if args.out:
        out.close()
    print("%d lines, sha256 %s" % (lines, sha.hexdigest()), file=sys.stderr)


if __name__ == "__main__":
    main()
