"""A static, full-attention KV cache layer whose rows are stored as 8-bit or 4-bit codes with one scale (and zero) per 32 elements.

Format (csrc/kv_quant.hpp, include/qllm_mi355x.h): 8 bits symmetric -- s = act(max|x| / 127), code = clamp(rint(x / s), -127, 127), value
s * code; 4 bits asymmetric -- z = act(min x), s = act((max x - min x) / 15), code = clamp(rint((x - z) / s), 0, 15), value fma(code, s,
z); code 0 where s == 0; all in fp32.  `k_codes` / `v_codes`: uint8 [B, Hkv, L, D * bits / 8] (at 4 bits element i in nibble i of its
row, low nibble first); `k_params` / `v_params`: act [B, Hkv, L, P], P = D / 32 scales at 8 bits, D / 16 scales-then-zeros at 4.  At
D = 128 a row takes 136 bytes at 8 bits and 80 at 4, against 256 in fp16.

`ops.attn_decode_quant` (qllm_attn_decode_quant, csrc/attn_decode_quant.hip) reads such a cache in place and quantises and appends the
new row itself; the fused attention modules (q_layers/fused_attention.py, kind "quant_static") use it at decode and then call
`advance(1)`.  A token is quantised once, when it enters the cache, and every step -- the one that appends it included -- attends over
the dequantised row: unlike transformers' `QuantizedLayer` there is no full-precision residual.

Every other route -- prompts, chunks, eager, whatever the kernel refuses -- goes through `update`: it quantises the new rows into the
cache (`ops.kv_quantize` at the device counter) and returns [B, Hkv, max_cache_len, D] act-type tensors holding the valid positions
dequantised (`ops.kv_dequantize`); states that kernel cannot read in place (misaligned, odd strides) are copied contiguous first.  That
is the correctness route, not the fast path.  On CPU tensors both steps are a few lines of
torch with the same formulas.

Not built: a quantized ring / sliding layer, a dynamic quantized cache, per-channel K quantisation (KIVI), fp8 (prompts and chunks
read the codes in place where the install asks for it: csrc/attn_chunk_quant.hip, csrc/attn_prefill_quant.hip; otherwise they go through `update`), a residual full-precision window, torch.compile of the layer (it is not compileable: `update` launches ctypes kernels)."""
from __future__ import annotations

import torch
from transformers.cache_utils import StaticCache, StaticLayer

from .. import ops

GROUP = 32


def quantize_rows(x: torch.Tensor, bits: int):
    """The format's formulas in torch, any device: x [..., D] fp16 / bf16 -> (codes uint8 [..., D * bits / 8], params [..., P] of x's type)."""
    dtype, d = x.dtype, x.shape[-1]
    g = x.float().unflatten(-1, (d // GROUP, GROUP))
    if bits == 8:
        s = (g.abs().amax(-1) / 127.0).to(dtype)
        c = torch.round(g / s.float()[..., None]).clamp(-127, 127)
        c = torch.where(s[..., None] == 0, torch.zeros_like(c), c).to(torch.int8).flatten(-2).view(torch.uint8)
        return c, s
    lo, hi = g.amin(-1), g.amax(-1)
    z, s = lo.to(dtype), ((hi - lo) / 15.0).to(dtype)
    c = torch.round((g - z.float()[..., None]) / s.float()[..., None]).clamp(0, 15)
    c = torch.where(s[..., None] == 0, torch.zeros_like(c), c).to(torch.uint8).flatten(-2)
    return c[..., 0::2] | (c[..., 1::2] << 4), torch.cat((s, z), dim=-1)


def dequantize_rows(codes: torch.Tensor, params: torch.Tensor, bits: int) -> torch.Tensor:
    """The inverse of `quantize_rows`, rounded once to the params' type: [..., D]."""
    if bits == 8:
        c, s, z = codes.view(torch.int8).float(), params.float(), None
    else:
        c = torch.stack((codes & 15, codes >> 4), dim=-1).flatten(-2).float()
        s, z = params.float().chunk(2, dim=-1)
    c = c.unflatten(-1, (s.shape[-1], GROUP))
    v = c * s[..., None] if z is None else torch.addcmul(z[..., None].double(), c.double(), s[..., None].double()).float()
    return v.flatten(-2).to(params.dtype)


def _readable(states: torch.Tensor) -> torch.Tensor:
    """`states` as ops.kv_quantize reads it in place -- 16-byte aligned, a contiguous last dimension, strides that are multiples of 8 (the
    [B, S, H, D] projection view is) -- or a contiguous copy of it."""
    ok = states.data_ptr() % 16 == 0 and states.stride(-1) == 1 and all(st % 8 == 0 and st >= 0 for st in states.stride()[:3])
    return states if ok else states.contiguous()


class QuantStaticLayer(StaticLayer):
    """Four buffers (`k_codes`, `k_params`, `v_codes`, `v_params`) for max_cache_len positions, the device counter `cumulative_length`
    (what the kernels read) and the host counter `cumulative_length_int`.  `keys` / `values` are the scratch pair of the CACHE (`scratch`,
    a dict all layers of one cache share): [B, Hkv, max_cache_len, D] act-type tensors, allocated zero-filled on first use, into which
    `update` dequantises the valid positions.  One pair suffices only because the layers of a model run one after another: what `update`
    returned is consumed by that layer's attention before the next layer's `update` overwrites it."""

    is_compileable = False

    def __init__(self, max_cache_len: int, bits: int = 8, scratch: dict | None = None, **kwargs):
        super().__init__(max_cache_len=max_cache_len)
        if isinstance(bits, bool) or bits not in ops.KV_QUANT_BITS:
            raise ValueError(f"QuantStaticLayer: bits must be 8 or 4 (got {bits!r})")
        self.bits = bits
        self.scratch = {} if scratch is None else scratch
        self.cumulative_length_int = 0
        self.k_codes = self.k_params = self.v_codes = self.v_params = None

    def lazy_initialization(self, key_states: torch.Tensor, value_states: torch.Tensor) -> None:
        self.dtype, self.device = key_states.dtype, key_states.device
        self.batch_size, self.num_heads = key_states.shape[:2]
        self.k_head_dim = self.v_head_dim = d = key_states.shape[-1]
        if d % GROUP or value_states.shape[-1] != d or self.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"QuantStaticLayer needs fp16 / bf16 states of one head_dim that is a multiple of {GROUP} (got {d}, {value_states.shape[-1]}, {self.dtype})")
        nbytes, nparams = ops.kv_quant_shapes(d, self.bits)
        lead = (self.batch_size, self.num_heads, self.max_cache_len)
        self.k_codes, self.v_codes = (torch.zeros(lead + (nbytes,), dtype=torch.uint8, device=self.device) for _ in range(2))
        self.k_params, self.v_params = (torch.zeros(lead + (nparams,), dtype=self.dtype, device=self.device) for _ in range(2))
        self.cumulative_length = self.cumulative_length.to(self.device)
        key = (lead + (d,), self.dtype, self.device)
        if key not in self.scratch:   # zero-filled, once per cache: positions beyond the length are never written
            self.scratch[key] = (torch.zeros(key[0], dtype=self.dtype, device=self.device), torch.zeros(key[0], dtype=self.dtype, device=self.device))
        self.keys, self.values = self.scratch[key]
        self.is_initialized = True

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs) -> tuple[torch.Tensor, torch.Tensor]:
        """Quantise the new rows into positions cumulative_length .. of the cache, bump both counters, and return the scratch pair with
        every valid position dequantised."""
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        new, cur = key_states.shape[-2], self.cumulative_length_int
        if cur + new > self.max_cache_len:
            raise ValueError(f"QuantStaticLayer: {cur} + {new} positions do not fit max_cache_len = {self.max_cache_len}")
        if key_states.is_cuda:
            ops.kv_quantize(_readable(key_states), self.k_codes, self.k_params, self.bits, self.cumulative_length)
            ops.kv_quantize(_readable(value_states), self.v_codes, self.v_params, self.bits, self.cumulative_length)
        else:
            for states, codes, params in ((key_states, self.k_codes, self.k_params), (value_states, self.v_codes, self.v_params)):
                codes[:, :, cur:cur + new], params[:, :, cur:cur + new] = quantize_rows(states, self.bits)
        self.advance(new)
        if key_states.is_cuda:
            ops.kv_dequantize(self.k_codes, self.k_params, self.bits, self.cumulative_length, self.keys)
            ops.kv_dequantize(self.v_codes, self.v_params, self.bits, self.cumulative_length, self.values)
        else:
            n = self.cumulative_length_int
            self.keys[:, :, :n] = dequantize_rows(self.k_codes[:, :, :n], self.k_params[:, :, :n], self.bits)
            self.values[:, :, :n] = dequantize_rows(self.v_codes[:, :, :n], self.v_params[:, :, :n], self.bits)
        return self.keys, self.values

    def advance(self, count: int = 1) -> None:
        """Count `count` tokens whose rows a kernel has already stored (ops.attn_decode_quant's append): both counters, no copy."""
        self.cumulative_length.add_(count)
        self.cumulative_length_int += count

    def reset(self) -> None:
        """Both counters to zero.  The codes stay: positions at or beyond the length are never read."""
        self.cumulative_length.zero_()
        self.cumulative_length_int = 0

    def crop(self, tokens_to_remove: int) -> None:
        """transformers' contract (`DynamicLayer.crop`, what `Cache.crop` hands every layer): a NEGATIVE value removes that many of the
        last tokens (at most all of them), 0 does nothing, a positive value is the deprecated absolute final length (nothing happens if
        the layer holds no more than that).  Both counters; the codes stay, positions at or beyond the length are never read."""
        n, cur = int(tokens_to_remove), self.cumulative_length_int
        keep = max(0, cur + n) if n < 0 else min(cur, n) if n > 0 else cur
        if keep != cur:
            self.cumulative_length.fill_(keep)
            self.cumulative_length_int = keep

    def offload(self):
        raise ValueError("QuantStaticLayer does not serve offloading caches")

    prefetch = offload

    def batch_repeat_interleave(self, repeats: int) -> None:
        raise ValueError("QuantStaticLayer does not serve batch_repeat_interleave / batch_select_indices (its buffers have a static batch)")

    batch_select_indices = batch_repeat_interleave

    def reorder_cache(self, beam_idx: torch.LongTensor) -> None:
        if self.is_initialized:
            idx = beam_idx.to(self.device)
            for name in ("k_codes", "k_params", "v_codes", "v_params"):
                getattr(self, name).copy_(getattr(self, name).index_select(0, idx))


def to_quant(cache, bits: int = 8):
    """Replace every layer of `cache` that is exactly an uninitialised StaticLayer by a QuantStaticLayer of the same size, in place; the new
    layers share one scratch pair.  Sliding layers stay as they are.  Returns `cache`.  ValueError on an offloading cache, on bits other
    than 8 / 4 and on a static layer that already holds its buffers."""
    layers = getattr(cache, "layers", None)
    if not isinstance(layers, list):
        raise ValueError("to_quant needs a cache with a list of layers (a transformers StaticCache)")
    if getattr(cache, "offloading", False):
        raise ValueError("to_quant does not serve offloading caches")
    if isinstance(bits, bool) or bits not in ops.KV_QUANT_BITS:
        raise ValueError(f"to_quant: bits must be 8 or 4 (got {bits!r})")
    full = [i for i, layer in enumerate(layers) if type(layer) is StaticLayer]
    if any(layers[i].is_initialized for i in full):
        raise ValueError("to_quant needs static layers that have not been initialised: convert the cache before its first update")
    scratch: dict = {}
    for i in full:
        layers[i] = QuantStaticLayer(max_cache_len=layers[i].max_cache_len, bits=bits, scratch=scratch)
    return cache


def quant_static_cache(config, max_cache_len: int, bits: int = 8, **kwargs) -> StaticCache:
    """A `StaticCache(config, max_cache_len, **kwargs)` whose full-attention layers store 8- or 4-bit codes: hand it to `generate` / the
    model as `past_key_values`."""
    return to_quant(StaticCache(config, max_cache_len=max_cache_len, **kwargs), bits)
