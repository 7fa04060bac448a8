#!/usr/bin/env python3
"""Mint golden vectors for the GPTQ quantizer with static groups (qllm_gptq_quantize_static, gptq_quantize_weight(static_groups=True))
from the REFERENCE's own Python, in the build container only:
    python tests/golden/make_goldens_gptq_static.py

The rules, the way the reference's GPTQ object is driven (CPU, fp32), the draw() recipe and the fields are make_goldens_gptq_quant.py's;
fasterquant runs with static_groups=True.  Fixtures land in tests/golden/gptq_static/gptqs_*.npz with the additional fields
  static_groups = 1
  dyn_diff: the share of codes that differ from the reference's own static_groups=False run on the same inputs
and with scale / zero [N,G] in the original group numbering (they depend on W alone), g_idx == arange(K) // groupsize.

Accepted per fixture: the reference against itself with the batches fed in reverse changes <= 0.2 % of the codes; neighbours of the sorted
diag(H) are > 1e-4 apart (relative); the output error is < 0.75 x round-to-nearest's; g_idx is trivial; >= 10 % of the codes differ from
the dynamic run's (static groups is another algorithm, not the same one under another name)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gptq_static")
sys.path.insert(0, HERE)
from make_goldens import import_reference  # noqa: E402
from make_goldens_gptq_quant import BATCHES, MAX_REV_DIFF, MIN_DIAG_GAP, draw, out_err, rtn  # noqa: E402

CASES = [
    # name, bits, g, N, K, act_order, sym, dtype, dead channel
    ("gptqs_w4_g128_actorder", 4, 128, 64, 384, True, False, torch.float16, None),
    ("gptqs_w4_g128", 4, 128, 64, 256, False, False, torch.float16, None),
    ("gptqs_w4_g32_actorder_n48", 4, 32, 48, 256, True, False, torch.float16, None),
    ("gptqs_w3_g64_actorder_sym", 3, 64, 64, 256, True, True, torch.float16, None),
    ("gptqs_w4_g64_k320_dead_actorder", 4, 64, 64, 320, True, False, torch.float16, 77),
    ("gptqs_w4_g128_actorder_bf16", 4, 128, 64, 256, True, False, torch.bfloat16, None),
]
MIN_DYN_DIFF = 0.10      # share of codes that differ from the reference's dynamic-groups run


def reference_run(mod, case, W, X, order, static_groups):
    """One fasterquant of the reference; returns (codes in original order, scale, zero, g_idx, error, U, perm, diag(H) with dead = 1)."""
    _, bits, g, N, K, act, sym, dtype, dead = case
    layer = torch.nn.Linear(K, N, bias=False)
    layer.weight.data = W.clone()
    q = mod.GPTQ(layer)
    q.quantizer.configure(bits, perchannel=True, sym=sym, mse=False)
    for b in order:
        q.add_batch(X[b], None)
    d = torch.diag(q.H).clone()
    d[d == 0] = 1
    perm = torch.argsort(d, descending=True) if act else torch.arange(K)
    got = {}
    chol = torch.linalg.cholesky

    def wrapped(A, *a, **kw):
        out = chol(A, *a, **kw)
        if kw.get("upper"):
            got["U"] = out.clone()
        return out

    keep = torch.cuda.synchronize, mod.GPTQ.print_loss
    torch.linalg.cholesky = wrapped
    torch.cuda.synchronize = lambda *a, **k: None
    mod.GPTQ.print_loss = lambda self, **kw: None
    try:
        with torch.no_grad():
            scale, zero, g_idx, error = q.fasterquant(percdamp=.01, groupsize=g, actorder=act, static_groups=static_groups)
    finally:
        torch.linalg.cholesky = chol
        torch.cuda.synchronize, mod.GPTQ.print_loss = keep
    Q = layer.weight.data.float()
    gi = g_idx.long()
    codes = torch.round(Q / scale[:, gi] + zero[:, gi])
    assert torch.equal(scale[:, gi] * (codes - zero[:, gi]), Q) and codes.min() >= 0 and codes.max() <= 2 ** bits - 1
    return codes.to(torch.uint8), scale, zero, g_idx, float(error), got["U"], perm, d


def make_case(mod, qmod, case, seed):
    name, bits, g, N, K, act, sym, dtype, dead = case
    W, X = draw(case, seed)
    codes, scale, zero, g_idx, error, U, perm, d = reference_run(mod, case, W, X, range(BATCHES), True)
    codes_rev = reference_run(mod, case, W, X, reversed(range(BATCHES)), True)[0]
    codes_dyn = reference_run(mod, case, W, X, range(BATCHES), False)[0]
    rev = float((codes != codes_rev).float().mean())
    dyn = float((codes != codes_dyn).float().mean())
    ds = torch.sort(d, descending=True)[0].double()
    gap = float(((ds[:-1] - ds[1:]) / ds[:-1]).min()) if act else 1.0
    Wz = W.clone()
    if dead is not None:
        Wz[:, dead] = 0
    gi = g_idx.long()
    Wq = scale[:, gi] * (codes.float() - zero[:, gi])
    e_gptq, e_rtn = out_err(Wz, Wq, X), out_err(Wz, rtn(qmod, case, Wz), X)
    trivial = torch.equal(g_idx.long(), torch.arange(K) // g)
    ok = rev <= MAX_REV_DIFF and gap > MIN_DIAG_GAP and e_gptq < 0.75 * e_rtn and trivial and dyn >= MIN_DYN_DIFF
    return ok, dict(bits=bits, groupsize=g, N=N, K=K, sym=int(sym), act_order=int(act), static_groups=1, w_dtype=str(dtype).split(".")[1],
                    W=W.numpy(), X=X.numpy(), U=np.ascontiguousarray(U.numpy()), perm=perm.numpy().astype(np.int64),
                    g_idx=g_idx.numpy().astype(np.int32), codes=codes.numpy(), scale=scale.numpy(), zero=zero.numpy(), error=error,
                    codes_rev=codes_rev.numpy(), dyn_diff=dyn, rtn_out_err=e_rtn, gptq_out_err=e_gptq, seed=seed), (rev, gap, dyn)


def main():
    import_reference()
    from qllm.quantization.gptq import gptq as mod
    from qllm.quantization.gptq import _gptq_quantizer as qmod
    os.makedirs(OUT, exist_ok=True)
    for i, case in enumerate(CASES):
        for seed in range(100 * i, 100 * i + 20):
            ok, d, (rev, gap, dyn) = make_case(mod, qmod, case, seed)
            if ok:
                break
        else:
            raise SystemExit(f"{case[0]}: no acceptable seed")
        path = os.path.join(OUT, case[0] + ".npz")
        np.savez_compressed(path, **d)
        print(f"{case[0]:34s} {os.path.getsize(path) / 1024:7.1f} KiB seed={seed} rev-diff={rev:.4%} diag-gap={gap:.1e} dyn-diff={dyn:.2%} "
              f"error={d['error']:.5e} gptq/rtn out err={d['gptq_out_err'] / d['rtn_out_err']:.3f}")


if __name__ == "__main__":
    main()
