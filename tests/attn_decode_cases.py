"""What tests/test_attn_decode_cpu.py, tests/test_attn_decode_gpu.py, tests/test_attn_decode_inputs_cpu.py and
tests/test_attn_decode_edges_gpu.py share: the float64 oracle, the eager yardstick, the torch restatement of the op that the CPU module
tests count calls with (and its fp32 result before the last rounding, the yardstick of `bound`), the shapes, the launch geometry and the
value families of the edge tests."""
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


def scores64(q, k, n, scaling, visible=None, bias=None):
    """float64 scores [B, Hkv, G, n] of q [B, Hq, D] against the first n positions of k [B, Hkv, L, D]: scaling * q.k, plus `bias` [B or 1, L]
    (any float type, -inf allowed), -inf where `visible` [B or 1, L] is False."""
    b, hq, d = q.shape
    hk = k.shape[1]
    s = torch.einsum("bkgd,bknd->bkgn", q.double().reshape(b, hk, hq // hk, d), k[:, :, :n].double()) * scaling   # the heads of a group share their kv head
    if bias is not None:
        s = s + bias.double()[:, None, None, :n]
    if visible is not None:
        s = s.masked_fill(~visible[:, None, None, :n], float("-inf"))
    return s


def oracle(q, k, v, n, scaling, visible=None, bias=None):
    """float64 attention of q [B, Hq, D] over the first n positions of k / v [B, Hkv, L, D] (CPU tensors of any type), keys hidden where
    `visible` [B, L] is False, `bias` [B, L] added to the scores: [B, Hq, D] float64."""
    w = torch.softmax(scores64(q, k, n, scaling, visible, bias), dim=-1)
    return torch.einsum("bkgn,bknd->bkgd", w, v[:, :, :n].double()).reshape(q.shape)


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


def restated32(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None):
    """`restated` before its last rounding: [B, Hq, D] float32.  Appends to the caches as `restated` does."""
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
    return torch.einsum("bhn,bhnd->bhd", torch.softmax(s, dim=-1), vv)


def restated(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None, *, out=None, plan=None):
    """ops.attn_decode restated in torch (any device): fp32 softmax over the valid keys, the append included.  Same signature."""
    return restated32(q, k_cache, v_cache, length, k_new, v_new, mask, scaling).to(q.dtype)


# ---- the tolerance of the edge tests -----------------------------------------------------------------------------------------------------------
FACTOR = 8      # of `bound`: the hardware exp2 (1 ulp where libm is below 1), the extra rounding of s * log2e, another summation order


def halfulp(ref64, dtype):
    """Half the spacing of `dtype` (fp16 / bf16) at |ref64|, per element, float64: what ONE rounding of the exact value costs at most.
    Floors: half the subnormal spacing for fp16 (2^-25), half the smallest normal's spacing for bf16 (2^-134)."""
    mant, emin = (10, -14) if dtype == torch.float16 else (7, -126)
    e = torch.frexp(ref64.abs())[1] - 1                                 # |ref| in [2^e, 2^(e + 1))
    e = torch.where(ref64 == 0, torch.full_like(e, emin), e).clamp(min=emin)
    return torch.ldexp(torch.ones_like(ref64), e - mant - 1)


def bound(ref64, e32, dtype, factor=FACTOR):
    """The per-element tolerance of a kernel that computes in fp32 and rounds once: halfulp(ref64, dtype) + factor * e32, where e32 is
    max |restated32 - oracle| of the same case (the error of the fp32 arithmetic on the CPU, never the kernel's)."""
    return halfulp(ref64, dtype) + factor * e32


def fp32_error(q, k, v, n, scaling, ref64, mask=None):
    """e32 of a case: max |restated32 - oracle| over its elements.  q [B, Hq, D]; mask as `restated` takes it."""
    r32 = restated32(q[:, :, None], k, v, n, mask=mask, scaling=scaling)
    return (r32.double() - ref64).abs().max().item(), r32


def geometry(b, hq, hk, d, at=1024, most=2051):
    """(L_max, {tile, splits, chunk, group}) of the accuracy tests: L_max = S * T + 3 of the launch for `at` positions (at most `most`), so
    the last split is ragged; at least 3 splits."""
    from qllm_amd import ops
    g0 = parse_describe(ops.attn_decode_describe(b, hq, hk, d, at))
    lmax = min(g0["splits"] * g0["tile"] + 3, most)
    g = parse_describe(ops.attn_decode_describe(b, hq, hk, d, lmax))
    assert g["splits"] >= 3 and g["chunk"] % g["tile"] == 0 and (g["splits"] - 1) * g["chunk"] < lmax <= g["splits"] * g["chunk"], g
    return lmax, g


def mid_split(g):
    return max(1, g["splits"] // 2)


def reduced_lengths(lmax, g):
    """1, T, the last position of a middle split and the first of the next, L_max - 1, L_max"""
    t, c, mid = g["tile"], g["chunk"], mid_split(g)
    return sorted({n for n in (1, t, mid * c, mid * c + 1, lmax - 1, lmax) if 1 <= n <= lmax})


def family_lengths(lmax, g):
    """T + 1, the first position behind a middle split, L_max"""
    return sorted({n for n in (g["tile"] + 1, mid_split(g) * g["chunk"] + 1, lmax) if 1 <= n <= lmax})


# ---- value families: (b, hq, hk, d, L, dtype, gen) -> q [B, Hq, D], k, v [B, Hkv, L, D] of `dtype`, scaling ------------------------------------
def _randn(shape, gen):
    return torch.randn(shape, generator=gen, dtype=torch.float64)


def _pull(q, hk, scaling):
    """u [B, Hkv, 1, D] float64, the shortest vector with scaling * q_g . u = 1 for EVERY query head g of the kv head's group, and the
    projector [B, Hkv, D, D] onto what is orthogonal to all of the group's q."""
    b, hq, d = q.shape
    qg = q.double().reshape(b, hk, hq // hk, d)
    pinv = torch.linalg.pinv(qg)                                              # [B, Hkv, D, G]
    u = pinv.sum(dim=-1) / scaling
    return u[:, :, None, :], torch.eye(d, dtype=torch.float64) - pinv @ qg


def peaked(b, hq, hk, d, L, dtype, gen):
    """N(0, 1) q and k, q times 8: scores with a standard deviation near 8 -- a few keys carry the weight, none all of it."""
    q, k, v = 8 * _randn((b, hq, d), gen), _randn((b, hk, L, d), gen), _randn((b, hk, L, d), gen)
    return q.to(dtype), k.to(dtype), v.to(dtype), d ** -0.5


SINK_SCORES = (27.0, 29.0, 31.0, 33.0, 35.0)    # of position 0 and of the last four, before their own noise (a quarter of the bulk's)


def sink(b, hq, hk, d, L, dtype, gen):
    """N(0, 1) values; position 0 and the last 4 positions pulled towards q (towards every q of the group alike): their scores sit 20 to
    40 above the bulk's largest, two apart from each other -- an attention sink and a recent window over a bulk that still counts in fp32."""
    q, k, v = _randn((b, hq, d), gen).to(dtype), _randn((b, hk, L, d), gen), _randn((b, hk, L, d), gen)
    u, _ = _pull(q, hk, d ** -0.5)
    for p, t in zip(sorted({0} | set(range(max(0, L - 4), L))), SINK_SCORES):
        k[:, :, p] = 0.25 * k[:, :, p] + t * u[:, :, 0]
    return q, k.to(dtype), v.to(dtype), d ** -0.5


CLIMB = 30.0


def _ramp(b, hq, hk, d, L, dtype, gen, ramp):
    q, k, v = _randn((b, hq, d), gen).to(dtype), _randn((b, hk, L, d), gen), _randn((b, hk, L, d), gen)
    u, perp = _pull(q, hk, d ** -0.5)
    k = k @ perp + CLIMB * ramp[None, None, :, None] * u        # the noise is orthogonal to every q of the group: it fills K, not the scores
    return q, k.to(dtype), v.to(dtype), d ** -0.5


def rising(b, hq, hk, d, L, dtype, gen):
    """k[pos] = noise + (pos / L) * c * q_dir (q_dir: `_pull`; the noise N(0, 1) without its part along the group's q): the scores climb
    by 30 across the cache, every tile raises the running maximum and scales what was accumulated by alpha < 1."""
    return _ramp(b, hq, hk, d, L, dtype, gen, torch.arange(L, dtype=torch.float64) / L)


def falling(b, hq, hk, d, L, dtype, gen):
    """`rising` mirrored: the first tile sets the running maximum, every later weight is smaller, down to e^-30."""
    return _ramp(b, hq, hk, d, L, dtype, gen, torch.arange(L - 1, -1, -1, dtype=torch.float64) / L)


def large_v(b, hq, hk, d, L, dtype, gen):
    """N(0, 1) scores, V uniform in (-1024, 1024): the outputs are convex combinations of V rows, so below 1024 < 65504 by construction."""
    q, k = _randn((b, hq, d), gen).to(dtype), _randn((b, hk, L, d), gen).to(dtype)
    v = (torch.rand((b, hk, L, d), generator=gen, dtype=torch.float64) * 2 - 1) * 1024
    return q, k, v.to(dtype), d ** -0.5


FAMILIES = {"peaked": peaked, "sink": sink, "rising": rising, "falling": falling, "large_v": large_v}
FAMILY_HEADS = ((8, 2), (5, 1))


def family_inputs(name, hq, hk, d, dtype, n):
    """The family's batch-1 inputs over n positions, seeded by the case: the CPU file proves its premises on the very tensors the GPU file runs."""
    return FAMILIES[name](1, hq, hk, d, n, dtype, torch.Generator().manual_seed(1000 * n + 7 * hq + d))
