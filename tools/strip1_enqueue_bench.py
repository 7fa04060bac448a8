"""The host cost of one eager batch-1 launch: wall time of CALLS back-to-back qllm_linear_forward calls on one native-layout layer
(K = 4096, N = 4096: the batch-1 kernel's nw=4 round=32 exact form), called through the C entry with preallocated buffers and ended by
one synchronise -- what csrc/strip1_forms.hpp's picker and launch site cost per call, as far as a kernel of ~3.5 us lets it show.
A/B two builds with QLLM_MI355X_LIB, alternating processes (profiles/strip1_forms.md).

    python tools/strip1_enqueue_bench.py [--calls 4000] [--reps 7]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gpu_util import synth, to_layer  # noqa: E402
from qllm_amd import _lib, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=4000)
    ap.add_argument("--reps", type=int, default=7, help="timings; the first is a warm-up and is left out of median / min")
    args = ap.parse_args()
    dev = "cuda:0"
    layer = to_layer(synth("GPTQ", 4, 128, 4096, 4096, "asym", False, False, seed=1), dev)
    w = layer.native_descriptor(0)
    plan = ops.plan_describe([w], 1)
    assert plan.startswith("strip1 nw=4 round=32 exact"), plan
    lib = _lib.load()
    x = torch.randn(1, 4096, device=dev).half()
    y = torch.empty(1, 4096, device=dev, dtype=torch.float16)
    want = ops.linear_forward(w, x)
    ws = ops.workspace(x.device, lib.qllm_workspace_bytes_act(C.byref(w), 1, _lib.DT_F16))
    call_args = (C.byref(w), C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), 1, _lib.DT_F16, C.c_void_p(ws.data_ptr()), ws.numel(),
                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    fn = lib.qllm_linear_forward
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            rc = fn(*call_args)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e6 / args.calls)
        assert rc == 0, _lib.last_error()
    assert torch.equal(y, want)
    print("strip1_enqueue lib=%s plan='%s' calls=%d us_per_call median=%.3f min=%.3f all=%s"
          % (os.path.basename(_lib.LIB_PATH), plan, args.calls, float(np.median(times[1:])), min(times[1:]), " ".join("%.3f" % t for t in times)))


if __name__ == "__main__":
    main()
