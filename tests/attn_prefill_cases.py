"""What tests/test_attn_prefill_cpu.py, tests/test_attn_prefill_inputs_cpu.py, tests/test_attn_prefill_gpu.py and
tests/test_attn_prefill_modules_gpu.py share: the float64 oracle of ops.attn_prefill, its fp32 restatements, the eager yardstick, the
tolerance `bound`, the launch geometry, and the builders of the exact inputs (selection, uniform).

Conventions.  q [B, Hq, S, D]; k, v [B, Hkv, L, D]; n = kv_len counts the valid positions INCLUDING the S new rows; query row i sits at
position n - S + i; mask None, [B or 1, S, L'] or [B or 1, 1, S, L'], bool (True = visible) or additive in the activation type (a value <=
the type's lowest finite number hides the key); outputs [B, S, Hq, D].  A row with no visible key gives zeros."""
import re

import torch

from attn_decode_cases import FACTOR, halfulp

DIMS = (64, 128)
DTYPES = (torch.float16, torch.bfloat16)
GROUPS = ((1, 1), (8, 2), (7, 1), (8, 1))      # (Hq, Hkv): no grouping, G = 4, an odd G, the largest G
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}   # one rounding to the type, relative


def parse_describe(text):
    """{q_tile, kv_tile, group, grid} of a qllm_attn_prefill_describe answer."""
    assert text.startswith("attn_prefill "), text
    out = {k: int(v) for k, v in re.findall(r"(q_tile|kv_tile|group)=(\d+)", text)}
    out["grid"] = tuple(int(x) for x in re.search(r"grid=(\d+)x(\d+)x(\d+)", text).groups())
    return out


def tiles(b=1, hq=1, hk=1, d=64, s=2, lmax=2):
    """(q_tile, kv_tile) of the launch: pure host code, read from the library and never hard-coded in a test."""
    from qllm_amd import ops
    g = parse_describe(ops.attn_prefill_describe(b, hq, hk, d, s, lmax))
    return g["q_tile"], g["kv_tile"]


def visibility(b, s, n, causal=True, mask=None, dtype=None):
    """(visible [B, S, n] bool, bias [B, S, n] float64): causality (key j counts for row i iff j <= n - s + i) and the mask."""
    j, i = torch.arange(n)[None, None, :], torch.arange(s)[None, :, None]
    vis = (j <= n - s + i) if causal else torch.ones(1, s, n, dtype=torch.bool)
    vis = vis.expand(b, s, n).clone()
    bias = torch.zeros(b, s, n, dtype=torch.float64)
    if mask is not None:
        m3 = (mask[:, 0] if mask.dim() == 4 else mask)[:, :, :n].expand(b, s, n)
        if m3.dtype == torch.bool:
            vis &= m3
        else:
            hidden = m3 <= torch.finfo(m3.dtype).min
            vis &= ~hidden
            bias = torch.where(hidden, torch.zeros((), dtype=torch.float64), m3.double())
    return vis, bias


def _weights(q, k, n, scaling, causal, mask, ftype):
    """softmax weights [B, Hkv, G, S, n] in `ftype` (rows with no visible key: zeros) from scores computed in `ftype`."""
    b, hq, s, d = q.shape
    hk = k.shape[1]
    vis, bias = visibility(b, s, n, causal, mask)
    sc = torch.einsum("bkgsd,bknd->bkgsn", q.to(ftype).reshape(b, hk, hq // hk, s, d), k[:, :, :n].to(ftype)) * scaling + bias.to(ftype)[:, None, None]
    sc = sc.masked_fill(~vis[:, None, None], float("-inf"))
    dead = ~vis.any(dim=-1)[:, None, None, :, None]
    w = torch.softmax(sc.masked_fill(dead, 0.0), dim=-1)
    return w.masked_fill(dead, 0.0)


def oracle(q, k, v, n, scaling, causal=True, mask=None, weights=False):
    """float64 attention: [B, S, Hq, D] float64; with `weights` also sum_j p_j |v_j| [B, S, Hq, D], the scale of `bound`'s middle term."""
    b, hq, s, d = q.shape
    w = _weights(q, k, n, scaling, causal, mask, torch.float64)
    vv = v[:, :, :n].double()
    out = torch.einsum("bkgsn,bknd->bsgkd", w, vv).permute(0, 1, 3, 2, 4).reshape(b, s, hq, d)
    if not weights:
        return out
    return out, torch.einsum("bkgsn,bknd->bsgkd", w, vv.abs()).permute(0, 1, 3, 2, 4).reshape(b, s, hq, d)


def restated32(q, k_cache, v_cache, length, mask=None, causal=True, scaling=None):
    """ops.attn_prefill in plain fp32 before the last rounding (scores, softmax and sums in fp32, P NOT rounded): [B, S, Hq, D] float32."""
    b, hq, s, d = q.shape
    n = int(length)
    w = _weights(q, k_cache, n, d ** -0.5 if scaling is None else scaling, causal, mask, torch.float32)
    return torch.einsum("bkgsn,bknd->bsgkd", w, v_cache[:, :, :n].float()).permute(0, 1, 3, 2, 4).reshape(b, s, hq, d)


def restated(q, k_cache, v_cache, length, mask=None, causal=True, scaling=None, *, out=None, plan=None):
    """ops.attn_prefill restated in torch (any device).  Same signature; [B, S, Hq, D] of q's type."""
    return restated32(q, k_cache, v_cache, length, mask, causal, scaling).to(q.dtype)


def kernel32(q, k, v, n, scaling, causal=True, mask=None):
    """The kernel's arithmetic restated in fp32 on the CPU: fp32 scores in the log2 domain, the maximum taken over the whole row, P =
    exp2(s - max) rounded to the activation type as the P.V operand, the denominator summed from the UNROUNDED fp32 P, fp32 sums, one
    division: [B, S, Hq, D] float32 before the store's rounding."""
    b, hq, s, d = q.shape
    hk = k.shape[1]
    vis, bias = visibility(b, s, n, causal, mask)
    sc = torch.einsum("bkgsd,bknd->bkgsn", q.float().reshape(b, hk, hq // hk, s, d), k[:, :, :n].float())
    sc = (sc * torch.tensor(scaling, dtype=torch.float32) + bias.float()[:, None, None]) * torch.tensor(1.4426950408889634, dtype=torch.float32)
    sc = sc.masked_fill(~vis[:, None, None], float("-inf"))
    mx = sc.amax(dim=-1, keepdim=True).clamp(min=-1e30)
    p = torch.exp2(sc - mx)
    l = p.sum(dim=-1)
    acc = torch.einsum("bkgsn,bknd->bkgsd", p.to(q.dtype).float(), v[:, :, :n].float())
    o = torch.where(l[..., None] > 0, acc / l[..., None].clamp(min=1e-38), torch.zeros((), dtype=torch.float32))
    return o.permute(0, 3, 1, 2, 4).reshape(b, s, hq, d)


def eager(q, k, v, n, scaling, causal=True, mask=None):
    """transformers' eager_attention_forward arithmetic in the activation type on the CPU: repeat_kv, matmul * scaling (rounded), + the
    additive mask (finfo.min where hidden), softmax in fp32 rounded to the type, matmul (rounded): [B, S, Hq, D]."""
    b, hq, s, d = q.shape
    g = hq // k.shape[1]
    vis, bias = visibility(b, s, n, causal, mask)
    add = torch.where(vis, bias, torch.full((), float(torch.finfo(q.dtype).min), dtype=torch.float64)).to(q.dtype)
    kk = k[:, :, :n].repeat_interleave(g, dim=1)
    vv = v[:, :, :n].repeat_interleave(g, dim=1)
    w = torch.matmul(q, kk.transpose(2, 3)) * scaling + add[:, None]
    w = torch.nn.functional.softmax(w, dim=-1, dtype=torch.float32).to(q.dtype)
    return torch.matmul(w, vv).transpose(1, 2).contiguous()


def bound(ref64, pv_abs64, e32, dtype, factor=FACTOR):
    """Per element: half the spacing of `dtype` at the oracle (the one rounding at the store) + 2 u sum_j p_j |v_j| (P is rounded once to
    the type as the P.V operand, relative error u per weight; the second u covers the quotient when the denominator is summed from the
    rounded weights instead) + factor * e32, e32 = max |restated32 - oracle| of the same case: the error of plain fp32 arithmetic on the
    CPU, never the kernel's; the factor is tests/attn_decode_cases.py's (hardware exp2, the extra rounding of s * log2e, another summation
    order)."""
    return halfulp(ref64, dtype) + 2 * U[dtype] * pv_abs64 + factor * e32


def fp32_error(q, k, v, n, scaling, ref64, causal=True, mask=None):
    return (restated32(q, k, v, n, mask, causal, scaling).double() - ref64).abs().max().item()


# ---- exact inputs ------------------------------------------------------------------------------------------------------------------------
SEL_A = 64.0          # the selection inputs' code amplitude: a full match scores 2 A^2, a half match A^2, scaling 1 / 8
SEL_SCALING = 0.125
SEL_GAP_LOG2 = SEL_A * SEL_A * SEL_SCALING * 1.4426950408889634   # 738.7: the winner's lead in the log2 domain (the issue asks for >= 40)


def value_rows(b, hk, L, d, dtype):
    """V [B, Hkv, L, D] of small asymmetric integers (-150 .. 250: exact in fp16 and bf16), V[j][c] = (j + 3 c + shift) mod 401 - 150:
    for L <= 401 and D <= 128 distinct in j at every column and distinct in c within every row; the shift tells batches and heads apart."""
    assert L <= 401 and d <= 128
    j = torch.arange(L)[None, None, :, None]
    c = torch.arange(d)[None, None, None, :]
    shift = 7 * (torch.arange(b)[:, None, None, None] * 3 + torch.arange(hk)[None, :, None, None])
    return ((j + 3 * c + shift) % 401 - 150).to(dtype)


def selection_pi(b, hq, s, q_start):
    """pi [B, Hq, S]: the key row i of head h selects, visible under causality (pi <= q_start + i) and not monotone in i."""
    i = torch.arange(s)[None, None, :]
    h = torch.arange(hq)[None, :, None]
    bb = torch.arange(b)[:, None, None]
    pos = q_start + i
    return ((pos * 2654435761 + h * 40503 + bb * 9973) >> 7) % (pos + 1)     # a multiplicative hash of the position, folded below it


def selection(b, hq, hk, d, s, q_start, dtype, lmax=None):
    """q, k, v, pi, scaling with out[b, i, h, :] == V[b, h / G, pi[b, h, i], :] EXACTLY: key j carries the code A (e_{j % 16} + e_{16 + j // 16}),
    q row i the code of pi(i), so its score is 2 A^2 / 8 at pi(i) and at most A^2 / 8 elsewhere -- 738 below in the log2 domain, weight
    exactly 0 in fp32 and in the type.  n = q_start + s <= 16 * (d - 16) keys."""
    n = q_start + s
    lmax = n if lmax is None else lmax
    assert n <= 16 * (d - 16) and lmax >= n
    j = torch.arange(lmax)
    k1 = torch.zeros(lmax, d, dtype=torch.float64)
    k1[j, j % 16] = SEL_A
    k1[j, 16 + j // 16] = SEL_A
    k = k1[None, None].expand(b, hk, lmax, d).to(dtype).contiguous()
    pi = selection_pi(b, hq, s, q_start)
    q = torch.zeros(b, hq, s, d, dtype=torch.float64)
    q.scatter_(3, (pi % 16)[..., None], SEL_A)
    q.scatter_(3, (16 + pi // 16)[..., None], SEL_A)
    return q.to(dtype), k, value_rows(b, hk, lmax, d, dtype), pi, SEL_SCALING


def selection_expected(v, pi, hk):
    """[B, S, Hq, D]: V[b, h / G, pi[b, h, i], :]"""
    b, hq, s = pi.shape
    g = hq // hk
    vh = v.repeat_interleave(g, dim=1)                                         # [B, Hq, L, D]
    return torch.gather(vh, 2, pi[..., None].expand(b, hq, s, v.shape[3])).transpose(1, 2).contiguous()


def uniform(b, hq, hk, d, s, n, dtype, lmax=None):
    """q = 0, K arbitrary finite, V integers: every visible key has weight exactly 1 / count."""
    lmax = n if lmax is None else lmax
    gen = torch.Generator().manual_seed(17 * s + n)
    q = torch.zeros(b, hq, s, d, dtype=dtype)
    k = torch.randn((b, hk, lmax, d), generator=gen).to(dtype)
    return q, k, value_rows(b, hk, lmax, d, dtype)


def uniform_expected(v, vis, hq):
    """(mean of V over the visible keys [B, S, Hq, D] float64 -- zeros for a row with none --, count [B, S])"""
    b, hk, _, d = v.shape
    n = vis.shape[2]
    cnt = vis.sum(dim=-1)
    tot = torch.einsum("bsn,bknd->bskd", vis.double(), v[:, :, :n].double())
    mean = torch.where(cnt[:, :, None, None] > 0, tot / cnt.clamp(min=1)[:, :, None, None].double(), torch.zeros((), dtype=torch.float64))
    return mean.repeat_interleave(hq // hk, dim=2), cnt


def ulp(ref64, dtype):
    return 2 * halfulp(ref64, dtype)


def left_padded(b, s, q_start, lwidth, pads, kind, dtype):
    """The mask transformers builds for a left-padded batch: [B, 1, S, lwidth], row i sees keys pads[b] <= j <= q_start + i; bool, or
    additive in `dtype` (0 / finfo.min)."""
    j, i = torch.arange(lwidth)[None, None, :], torch.arange(s)[None, :, None]
    vis = (j <= q_start + i) & (j >= torch.tensor(pads)[:, None, None])
    return as_mask(vis[:, None], kind, dtype)


def as_mask(vis, kind, dtype):
    if kind == "bool":
        return vis.clone()
    return torch.where(vis, torch.zeros((), dtype=dtype), torch.full((), torch.finfo(dtype).min, dtype=dtype))
