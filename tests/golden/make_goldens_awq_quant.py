#!/usr/bin/env python3
"""Mint golden vectors for the AWQ quantizer (qllm_awq_clip_search, qllm_awq_quantize, qllm_amd/quantization/awq.py) from the REFERENCE's
own Python, in the build container only:
    python tests/golden/make_goldens_awq_quant.py

Same rules as make_goldens_gptq_quant.py: the reference is imported read-only, only DATA is written, everything runs on the CPU in fp32.
What is driven: auto_clip_layer, pseudo_quantize_tensor and InternalAWQuantizer.auto_scale_block (its inner _search_module_scale) of
qllm/quantization/awq/_awq_quantizer.py.  Two things of this process stand in for a device: get_model_specific_quant_layer (the group list
that auto_scale_block receives) is substituted by the groups of the small module below, and Tensor.cpu copies during the scale search
-- _search_module_scale keeps `v.cpu()` of the state dict as its backup, which on a device is a copy and on the CPU would alias the
weights that fc.weight.mul_ then changes in place.

Fixtures land in tests/golden/awq_quant/.  awqq_*.npz (clip search and pseudo-quantizer, N = 64 rows, T = 128 tokens, n_sample_token = 64):
  bits, groupsize, N, K, w_dtype, seed
  W [N,K] f32 (exactly representable in w_dtype); X [T,K] f16
  best_max [N,G] f32: auto_clip_layer's result; best_idx [N,G] i32: the candidate it stands for (best_max == org * float32(1 - idx / 20))
  err64 [N,G,10] f64: the ten candidates' errors, quantization in fp32, the output error accumulated in fp64
  col_scale [K] f32
  per variant v in ("plain", "scale", "clip", "scale_clip"): codes_v [N,K] u8, scales_v / zeros_v [N,G] f32, wq_v [N,K] f32 --
  pseudo_quantize_tensor(clamp(W * col_scale, -best_max, best_max), get_scale_zp=True), wq divided by col_scale again
awqs_mlp.npz (scale search; bits 4, group 128, hidden 128, intermediate 256, 96 tokens):
  gate, up [256,128] f16, down [128,256] f16, x [96,128] f16
  s_mlp [128] f32 / s_down [256] f32: the reference's scales of the (gate, up) group inspected through the whole MLP and of down_proj alone
  ratio_mlp, ratio_down: the ratio they belong to; loss64_mlp / loss64_down [20] f64: the losses of the twenty ratios in fp64
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "awq_quant")
sys.path.insert(0, HERE)
from make_goldens import import_reference  # noqa: E402

CASES = [
    # name, bits, g, K, dtype
    ("awqq_w4_g128", 4, 128, 256, torch.float16),
    ("awqq_w3_g64", 3, 64, 256, torch.float16),
    ("awqq_w4_g32", 4, 32, 256, torch.float16),
    ("awqq_w4_g128_k384", 4, 128, 384, torch.float16),
    ("awqq_w4_g128_bf16", 4, 128, 256, torch.bfloat16),
]
N, T, N_SAMPLE, N_GRID, N_CAND = 64, 128, 64, 20, 10
MAX_BYTES = 632 * 1024    # no fixture larger than the largest one there is


def draw(K, dtype, seed):
    """Like the GPTQ fixtures: small normal weights; correlated input channels of unequal size."""
    gen = torch.Generator().manual_seed(seed)
    W = (0.02 * torch.randn((N, K), generator=gen)).to(dtype).float()
    r = K // 8
    f = torch.randn((T, r), generator=gen)
    mix = torch.randn((r, K), generator=gen) / r ** 0.5
    X = (f @ mix + 0.35 * torch.randn((T, K), generator=gen)) * torch.exp(0.8 * torch.randn(K, generator=gen))
    s = torch.exp(0.5 * torch.randn(K, generator=gen)).float()
    return W, X.half().float(), s


def clip_errors64(mod, W, X, bits, g, cfg):
    """The ten candidates' errors per (row, group): the reference's arithmetic up to q (fp32), the output error in fp64."""
    G = W.shape[1] // g
    xs = X[0::X.shape[0] // N_SAMPLE].double().reshape(-1, G, g)
    w = W.reshape(N, G, g)
    org = w.abs().amax(dim=-1, keepdim=True)
    errs = []
    for i in range(N_CAND):
        m = org * (1 - i / N_GRID)
        q = mod.pseudo_quantize_tensor(torch.clamp(w, -m, m), bits, cfg)
        d = (q - w).double()
        errs.append(torch.einsum("tjg,njg->ntj", xs, d).pow(2).mean(dim=1))
    return torch.stack(errs, dim=-1), org.squeeze(-1)


def make_clip_case(mod, case, seed):
    name, bits, g, K, dtype = case
    cfg = types.SimpleNamespace(zero_point=True, q_group_size=g)
    W, X, s = draw(K, dtype, seed)
    G = K // g
    best_max = mod.auto_clip_layer(W.clone(), X.clone(), bits, cfg, n_grid=N_GRID, max_shrink=0.5, n_sample_token=N_SAMPLE).squeeze(-1)
    err64, org = clip_errors64(mod, W, X, bits, g, cfg)
    idx = torch.round((1 - best_max / org) * N_GRID).to(torch.int32)
    factors = torch.tensor([1 - i / N_GRID for i in range(N_CAND)], dtype=torch.float32)
    exact = torch.equal(org * factors[idx.long()], best_max)
    ok = exact and torch.equal(err64.argmin(dim=-1).to(torch.int32), idx)
    d = dict(bits=bits, groupsize=g, N=N, K=K, w_dtype=str(dtype).split(".")[1], seed=seed, W=W.numpy(), X=X.numpy().astype(np.float16),
             best_max=best_max.numpy(), best_idx=idx.numpy(), err64=err64.numpy(), col_scale=s.numpy())
    maxq = 2 ** bits - 1
    for v, (use_s, use_c) in dict(plain=(0, 0), scale=(1, 0), clip=(0, 1), scale_clip=(1, 1)).items():
        val = W * s.view(1, -1) if use_s else W.clone()
        if use_c:
            m = best_max.unsqueeze(-1)
            val = torch.clamp(val.reshape(N, G, g), -m, m).reshape(N, K)
        wq, sc, z = mod.pseudo_quantize_tensor(val, bits, cfg, get_scale_zp=True)
        sk, zk = sc.repeat_interleave(g, 1), z.repeat_interleave(g, 1)
        codes = torch.clamp(torch.round(val / sk) + zk, 0, maxq)
        assert torch.equal((codes - zk) * sk, wq)
        if use_s:
            wq = wq / s.view(1, -1)
        d.update({f"codes_{v}": codes.numpy().astype(np.uint8), f"scales_{v}": sc.numpy(), f"zeros_{v}": z.numpy(), f"wq_{v}": wq.numpy()})
    return ok, d


class MLP(torch.nn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
        self.gate_proj = torch.nn.Linear(hidden, inter, bias=False)
        self.up_proj = torch.nn.Linear(hidden, inter, bias=False)
        self.down_proj = torch.nn.Linear(inter, hidden, bias=False)
        self.act = torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act(self.gate_proj(x)) * self.up_proj(x))


class Block(torch.nn.Module):
    def __init__(self, hidden, inter):
        super().__init__()
        self.norm = torch.nn.LayerNorm(hidden)
        self.mlp = MLP(hidden, inter)


def losses64(mod, inspect, fcs, x, bits, g, cfg):
    """The twenty ratios' scales (fp32, the reference's formula) and losses: quantization in fp32, the module's output in fp64."""
    weight = torch.cat([fc.weight.data for fc in fcs], dim=0)
    w_mean, x_mean = mod.get_weight_scale(weight, q_group_size=g), mod.get_act_scale(x)
    orig = [fc.weight.data.clone() for fc in fcs]
    inspect.double()
    org_out = inspect(x.double())
    out, scales = [], []
    for i in range(N_GRID):
        r = i / N_GRID
        s = (x_mean.pow(r) / (w_mean.pow(1 - r) + 1e-4)).clamp(min=1e-4).view(-1)
        s = s / (s.max() * s.min()).sqrt()
        for fc, w in zip(fcs, orig):
            fc.weight.data = (mod.pseudo_quantize_tensor(w * s.view(1, -1), bits, cfg) / s.view(1, -1)).double()
        out.append(float((org_out - inspect(x.double())).pow(2).mean()))
        scales.append(s)
    inspect.float()
    for fc, w in zip(fcs, orig):
        fc.weight.data = w
    return scales, np.array(out)


def make_scale_case(mod, seed):
    bits, g, hidden, inter, tokens = 4, 128, 128, 256, 96
    cfg = types.SimpleNamespace(zero_point=True, q_group_size=g)
    gen = torch.Generator().manual_seed(seed)
    block = Block(hidden, inter)
    mlp = block.mlp
    for lin in (mlp.gate_proj, mlp.up_proj, mlp.down_proj):
        lin.weight.data = (torch.randn(lin.weight.shape, generator=gen) / lin.in_features ** 0.5).half().float()
    x = (torch.randn((tokens, hidden), generator=gen) * torch.exp(0.8 * torch.randn(hidden, generator=gen))).half().float()
    saved = {k: v.clone() for k, v in block.state_dict().items()}
    with torch.no_grad():
        x_down = mlp.act(mlp.gate_proj(x)) * mlp.up_proj(x)
        groups = [dict(prev_op=block.norm, layers=[mlp.gate_proj, mlp.up_proj], inp=x, module2inspect=mlp),
                  dict(prev_op=mlp.up_proj, layers=[mlp.down_proj], inp=x_down)]
        quantizer = mod.InternalAWQuantizer()
        quantizer.configure(bits, cfg)
        keep = mod.get_model_specific_quant_layer, torch.Tensor.cpu
        mod.get_model_specific_quant_layer = lambda **kw: groups
        torch.Tensor.cpu = lambda self, *a, **k: self.clone()
        try:
            found = quantizer.auto_scale_block(block, {}, input_feat={}, model_type="none")
        finally:
            mod.get_model_specific_quant_layer, torch.Tensor.cpu = keep
        assert all(torch.equal(v, saved[k]) for k, v in block.state_dict().items())     # the reference restored its weights
        d = dict(bits=bits, groupsize=g, seed=seed, gate=mlp.gate_proj.weight.data.numpy().astype(np.float16),
                 up=mlp.up_proj.weight.data.numpy().astype(np.float16), down=mlp.down_proj.weight.data.numpy().astype(np.float16),
                 x=x.numpy().astype(np.float16))
        ok = True
        for key, (_, _, s_ref), inspect, fcs, inp in (("mlp", found[0], mlp, groups[0]["layers"], x),
                                                      ("down", found[1], mlp.down_proj, groups[1]["layers"], x_down)):
            scales, loss = losses64(mod, inspect, fcs, inp, bits, g, cfg)
            at = int(np.argmin([float((s - s_ref).abs().max()) for s in scales]))
            order = np.argsort(loss)
            ok = ok and torch.equal(scales[at], s_ref) and order[0] == at and loss[order[0]] <= 0.99 * loss[order[1]]
            d.update({f"s_{key}": s_ref.numpy(), f"ratio_{key}": at / N_GRID, f"loss64_{key}": loss})
    return ok, d


def save(name, d):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **d)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, (name, size)
    return size


def main():
    import_reference()
    from qllm.quantization.awq import _awq_quantizer as mod
    os.makedirs(OUT, exist_ok=True)
    for i, case in enumerate(CASES):
        for seed in range(100 * i, 100 * i + 40):
            ok, d = make_clip_case(mod, case, seed)
            if ok:
                break
        else:
            raise SystemExit(f"{case[0]}: no acceptable seed")
        print(f"{case[0]:20s} {save(case[0], d) / 1024:7.1f} KiB seed={seed} clipped groups {float((d['best_idx'] > 0).mean()):.1%}")
    for seed in range(900, 940):
        ok, d = make_scale_case(mod, seed)
        if ok:
            break
    else:
        raise SystemExit("awqs_mlp: no acceptable seed")
    print(f"{'awqs_mlp':20s} {save('awqs_mlp', d) / 1024:7.1f} KiB seed={seed} ratios mlp {d['ratio_mlp']} down {d['ratio_down']}")


if __name__ == "__main__":
    main()
