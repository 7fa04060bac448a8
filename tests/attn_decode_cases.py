"""What tests/test_attn_decode_cpu.py and tests/test_attn_decode_gpu.py share: the float64 oracle, the eager yardstick, the torch
restatement of the op that the CPU module tests count calls with, and the shapes."""
import re

import torch

HEADS = ((1, 1), (4, 4), (8, 2), (28, 4), (32, 8))
DIMS = (64, 128)
BATCHES = (1, 3)
DTYPES = (torch.float16, torch.bfloat16)


def parse_describe(text):
    """{tile, splits, chunk, group} of a qllm_attn_decode_describe answer."""
    assert text.startswith("attn_decode "), text
    return {k: int(v) for k, v in re.findall(r"(tile|splits|chunk|group)=(\d+)", text)}


def oracle(q, k, v, n, scaling, visible=None):
    """float64 attention of q [B, Hq, D] over the first n positions of k / v [B, Hkv, L, D] (CPU tensors of any type), keys hidden where
    `visible` [B, L] is False: [B, Hq, D] float64."""
    b, hq, d = q.shape
    hk = k.shape[1]
    kk, vv = k[:, :, :n].double(), v[:, :, :n].double()
    s = torch.einsum("bkgd,bknd->bkgn", q.double().reshape(b, hk, hq // hk, d), kk) * scaling      # the heads of a group share their kv head
    if visible is not None:
        s = s.masked_fill(~visible[:, None, None, :n], float("-inf"))
    return torch.einsum("bkgn,bknd->bkgd", torch.softmax(s, dim=-1), vv).reshape(b, hq, d)


def eager(q, k, v, n, scaling, additive=None):
    """transformers' eager_attention_forward arithmetic in the activation type on the CPU: repeat_kv, matmul * scaling (rounded), + mask,
    softmax in fp32 rounded to the type, matmul (rounded).  q [B, Hq, D] -> [B, Hq, D]."""
    b, hq, d = q.shape
    g = hq // k.shape[1]
    kk = k[:, :, :n].repeat_interleave(g, dim=1)
    vv = v[:, :, :n].repeat_interleave(g, dim=1)
    w = torch.matmul(q[:, :, None], kk.transpose(2, 3)) * scaling
    if additive is not None:
        w = w + additive[:, None, None, :n]
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    return torch.matmul(w, vv)[:, :, 0]


def restated(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None, *, out=None, plan=None):
    """ops.attn_decode restated in torch (any device): fp32 softmax over the valid keys, the append included.  Same signature."""
    heads = 1 if q.shape[2] == 1 else 2
    q3 = q.squeeze(2 if heads == 1 else 1)
    n = int(length)
    if k_new is not None:
        k_cache[:, :, n] = k_new.squeeze(2 if k_new.shape[2] == 1 else 1)
        v_cache[:, :, n] = v_new.squeeze(2 if v_new.shape[2] == 1 else 1)
        n += 1
    b, hq, d = q3.shape
    g = hq // k_cache.shape[1]
    kk = k_cache[:, :, :n].float().repeat_interleave(g, dim=1)
    vv = v_cache[:, :, :n].float().repeat_interleave(g, dim=1)
    s = torch.einsum("bhd,bhnd->bhn", q3.float(), kk) * (d ** -0.5 if scaling is None else scaling)
    if mask is not None:
        m2 = mask.reshape(mask.shape[0], -1)[:, :n]
        s = s.masked_fill(~m2[:, None], float("-inf")) if m2.dtype == torch.bool else s + m2[:, None].float()
    return torch.einsum("bhn,bhnd->bhd", torch.softmax(s, dim=-1), vv).to(q.dtype)
