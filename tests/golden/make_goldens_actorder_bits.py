#!/usr/bin/env python3
"""Mint the act-order fixtures at the widths without a strip kernel (2 / 5 / 6 / 7 / 8 bits) with the REFERENCE's own Python, exactly as
make_goldens.py does for the others (same shims, same make_case, same fields).

Run in the build container only:   python tests/golden/make_goldens_actorder_bits.py
They go to tests/golden/actorder_bits/: the top level of tests/golden is globbed by conftest.golden_names(), and these belong to
tests/test_bitgemv_actorder_*.py alone.  Only DATA is written.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_goldens import import_reference, make_case  # noqa: E402

OUT = os.path.join(HERE, "actorder_bits")

CASES = [
    # name, layout, bits, g, K, N, zero_kind, act_order, bias, compat  (at least four groups each)
    ("gptq_w2_g64_actorder", "GPTQ", 2, 64, 256, 128, "asym", True, False, 0),
    ("gptq_w5_g64_actorder_bias", "GPTQ", 5, 64, 256, 128, "asym", True, True, 0),
    ("gptq_w6_g128_actorder", "GPTQ", 6, 128, 512, 128, "asym", True, False, 0),
    ("gptq_w7_g64_actorder", "GPTQ", 7, 64, 256, 128, "asym", True, False, 0),
    ("gptq_w8_g128_actorder_sym", "GPTQ", 8, 128, 512, 128, "sym", True, False, 0),
]


def main():
    ref = import_reference()
    os.makedirs(OUT, exist_ok=True)
    for i, case in enumerate(CASES):
        data = make_case(ref, *case, seed=4321 + i)
        path = os.path.join(OUT, case[0] + ".npz")
        np.savez_compressed(path, **data)
        print(f"{case[0]:32s} {os.path.getsize(path) / 1024:8.1f} KiB  y.absmax={np.abs(data['y']).max():.3f}")


if __name__ == "__main__":
    main()
