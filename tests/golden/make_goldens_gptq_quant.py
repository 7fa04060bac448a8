#!/usr/bin/env python3
"""Mint golden vectors for the GPTQ quantizer (qllm_gptq_quantize, qllm_amd/quantization/gptq.py) from the REFERENCE's own Python, in
the build container only:
    python tests/golden/make_goldens_gptq_quant.py

Same rules as make_goldens.py: the reference is imported read-only, only DATA is written.  The reference's GPTQ object
(qllm/quantization/gptq/gptq.py) is driven the way GPTQQuant.do_quantize drives it: configure(bits, perchannel=True, sym, mse=False),
add_batch per calibration batch, fasterquant(percdamp=.01, groupsize, actorder).  fasterquant's torch.cuda.synchronize() and print_loss
are replaced by no-ops in this process; U is captured by wrapping torch.linalg.cholesky for its upper=True call.  Everything runs on the
CPU in fp32.

Fixtures land in tests/golden/gptq_quant/gptqq_*.npz.  Fields:
  bits, groupsize (the real size: K for the reference's -1), N, K, sym, act_order, w_dtype ("float16" | "bfloat16" | exactly representable)
  W [N,K] f32 (original column order, dead columns NOT yet zeroed); X [6,1,64,K] f16 (the calibration batches, in feeding order)
  U [K,K] f32: the upper Cholesky factor of the inverse damped Hessian, in PROCESSING order (permuted for act-order)
  perm [K] i64 (identity without act-order); g_idx [K] i32
  codes [N,K] u8, scale [N,G] f32, zero [N,G] f32 in the reference's ORIGINAL column order / group numbering; error (its summed loss)
  codes_rev [N,K] u8: the reference's codes when the six batches are fed in reverse order (its own rounding noise through H)
  rtn_out_err, gptq_out_err: tr(D H D^T) in fp64, D = W (dead columns zeroed) - dequantized weights, H = 2/n sum X^T X in fp64, for
  round-to-nearest on min/max group parameters and for the reference's result
  seed
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "gptq_quant")
sys.path.insert(0, HERE)
from make_goldens import import_reference  # noqa: E402

CASES = [
    # name, bits, g (-1: K), N, K, act_order, sym, dtype, dead channel
    ("gptqq_w4_g128", 4, 128, 64, 256, False, False, torch.float16, None),
    ("gptqq_w4_g128_actorder", 4, 128, 64, 384, True, False, torch.float16, None),
    ("gptqq_w3_g64", 3, 64, 64, 256, False, False, torch.float16, None),
    ("gptqq_w4_g32_actorder", 4, 32, 48, 256, True, False, torch.float16, None),
    ("gptqq_w4_g128_sym", 4, 128, 64, 256, False, True, torch.float16, None),
    ("gptqq_w2_g64", 2, 64, 64, 256, False, False, torch.float16, None),
    ("gptqq_w8_g128", 8, 128, 64, 256, False, False, torch.float16, None),
    ("gptqq_w4_gK", 4, -1, 64, 256, False, False, torch.float16, None),
    ("gptqq_w4_g64_k320_dead", 4, 64, 64, 320, False, False, torch.float16, 77),
    ("gptqq_w4_g128_bf16", 4, 128, 64, 256, False, False, torch.bfloat16, None),
]
BATCHES, TOKENS = 6, 64
MAX_REV_DIFF = 0.002     # share of codes the reference changes when the batches come in reverse order
MIN_DIAG_GAP = 1e-4      # relative gap between neighbours of the sorted diag(H): perm cannot flip between machines


def draw(case, seed):
    _, bits, g, N, K, act, sym, dtype, dead = case
    gen = torch.Generator().manual_seed(seed)
    W = (0.02 * torch.randn((N, K), generator=gen)).to(dtype).float()
    # correlated channels of unequal size: a few shared factors mixed into every channel, per-channel noise, log-normal channel scales
    r = K // 8
    f = torch.randn((BATCHES, 1, TOKENS, r), generator=gen)
    mix = torch.randn((r, K), generator=gen) / r ** 0.5
    noise = 0.35 * torch.randn((BATCHES, 1, TOKENS, K), generator=gen)
    ch = torch.exp(0.8 * torch.randn(K, generator=gen))
    X = ((f @ mix + noise) * ch)
    if dead is not None:
        X[..., dead] = 0
    return W, X.to(torch.float16)


def reference_run(mod, case, W, X, order):
    """One fasterquant of the reference; returns (codes in original order, scale, zero, g_idx, error, U, perm)."""
    _, bits, g, N, K, act, sym, dtype, dead = case
    layer = torch.nn.Linear(K, N, bias=False)
    layer.weight.data = W.clone()
    q = mod.GPTQ(layer)
    q.quantizer.configure(bits, perchannel=True, sym=sym, mse=False)
    for b in order:
        q.add_batch(X[b], None)
    H0 = q.H.clone()
    d = torch.diag(H0).clone()
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
            scale, zero, g_idx, error = q.fasterquant(percdamp=.01, groupsize=g, actorder=act, static_groups=False)
    finally:
        torch.linalg.cholesky = chol
        torch.cuda.synchronize, mod.GPTQ.print_loss = keep
    Q = layer.weight.data.float()
    gi = g_idx.long()
    codes = torch.round(Q / scale[:, gi] + zero[:, gi])
    assert torch.equal(scale[:, gi] * (codes - zero[:, gi]), Q) and codes.min() >= 0 and codes.max() <= 2 ** bits - 1
    return codes.to(torch.uint8), scale, zero, g_idx, float(error), got["U"], perm, d


def out_err(Wz, Wq, X):
    H = np.zeros((X.shape[-1],) * 2)
    for b in range(X.shape[0]):
        x = X[b].reshape(-1, X.shape[-1]).double().numpy()
        H += x.T @ x
    H *= 2.0 / X.shape[0]
    D = Wz.double().numpy() - Wq.double().numpy()
    return float(np.einsum("nk,kj,nj->", D, H, D))


def rtn(qmod, case, Wz):
    _, bits, g, N, K, act, sym, dtype, dead = case
    g = K if g == -1 else g
    qz = qmod.InternalGPTQQuantizer()
    qz.configure(bits, perchannel=True, sym=sym, mse=False)
    out = torch.empty_like(Wz)
    for c in range(0, K, g):
        qz.find_params(Wz[:, c:c + g], weight=True)
        out[:, c:c + g] = qz.quantize(Wz[:, c:c + g])
    return out


def make_case(mod, qmod, case, seed):
    name, bits, g, N, K, act, sym, dtype, dead = case
    W, X = draw(case, seed)
    codes, scale, zero, g_idx, error, U, perm, d = reference_run(mod, case, W, X, range(BATCHES))
    codes_rev = reference_run(mod, case, W, X, reversed(range(BATCHES)))[0]
    rev = float((codes != codes_rev).float().mean())
    ds = torch.sort(d, descending=True)[0].double()
    gap = float(((ds[:-1] - ds[1:]) / ds[:-1]).min()) if act else 1.0
    Wz = W.clone()
    if dead is not None:
        Wz[:, dead] = 0
    gi = g_idx.long()
    Wq = scale[:, gi] * (codes.float() - zero[:, gi])
    e_gptq, e_rtn = out_err(Wz, Wq, X), out_err(Wz, rtn(qmod, case, Wz), X)
    ok = rev <= MAX_REV_DIFF and gap > MIN_DIAG_GAP and e_gptq < 0.75 * e_rtn
    return ok, dict(bits=bits, groupsize=K if g == -1 else g, N=N, K=K, sym=int(sym), act_order=int(act), w_dtype=str(dtype).split(".")[1],
                    W=W.numpy(), X=X.numpy(), U=np.ascontiguousarray(U.numpy()), perm=perm.numpy().astype(np.int64), g_idx=g_idx.numpy().astype(np.int32),
                    codes=codes.numpy(), scale=scale.numpy(), zero=zero.numpy(), error=error, codes_rev=codes_rev.numpy(),
                    rtn_out_err=e_rtn, gptq_out_err=e_gptq, seed=seed), (rev, gap)


def main():
    import_reference()
    from qllm.quantization.gptq import gptq as mod
    from qllm.quantization.gptq import _gptq_quantizer as qmod
    os.makedirs(OUT, exist_ok=True)
    for i, case in enumerate(CASES):
        for seed in range(100 * i, 100 * i + 20):
            ok, d, (rev, gap) = make_case(mod, qmod, case, seed)
            if ok:
                break
        else:
            raise SystemExit(f"{case[0]}: no acceptable seed")
        path = os.path.join(OUT, case[0] + ".npz")
        np.savez_compressed(path, **d)
        print(f"{case[0]:26s} {os.path.getsize(path) / 1024:7.1f} KiB seed={seed} rev-diff={rev:.4%} diag-gap={gap:.1e} error={d['error']:.5e} "
              f"gptq/rtn out err={d['gptq_out_err'] / d['rtn_out_err']:.3f}")


if __name__ == "__main__":
    main()
