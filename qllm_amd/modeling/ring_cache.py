"""A sliding-window KV cache layer that keeps its rows as a ring buffer: position j lives in slot j mod C.

transformers' `StaticSlidingWindowLayer` keeps the last C = min(sliding_window, max_cache_len) positions in linear order, so once it is
full every new token rolls the whole K and V buffers by one row (profiles/attn_sliding.md: 68 to 78 % of the fused attention step at
W = 4096), and it switches from `index_copy_` to `roll` on a Python int, so a captured decode step cannot cross the point where it fills.
`RingSlidingWindowLayer` never moves a row: a new row overwrites the slot of the position that has just left the window, and the device
counter `cumulative_length` is the TOTAL number of tokens seen -- maintained on every update, unlike the parent's, which stops at
overflow.  `ops.attn_decode_ring` (qllm_attn_decode_ring, csrc/attn_decode_ring.hip) reads such a cache in place and appends the new row
itself; the fused attention modules (q_layers/fused_attention.py, kind "ring_sliding") use it at decode and then call `advance(1)`.

Every other route goes through `update`, which keeps the parent's contract: it returns, value for value and shape for shape, what
`StaticSlidingWindowLayer.update` returns for the same history -- past the fill a linearised copy, at about the cost of the roll.  That
is the correctness fallback, not the fast path.

Not built: torch.compile (the layer is not compileable: `update` returns fresh tensors past the fill), quantized and offloaded caches,
a ring for full-attention layers, prefill written into the ring by a kernel."""
from __future__ import annotations

import torch
from transformers.cache_utils import StaticCache, StaticSlidingWindowLayer


class RingSlidingWindowLayer(StaticSlidingWindowLayer):
    """Buffers [B, H, C = min(sliding_window, max_cache_len), D] with position j in slot j mod C; constructor, lazy initialisation, static
    addresses, `get_mask_sizes`, `get_seq_length`, `reset` and batch reordering are the parent's."""

    is_compileable = False

    def _slots(self, first: int, count: int) -> torch.Tensor:
        """The slots of positions first .. first + count - 1, from the host counter."""
        return (torch.arange(first, first + count, device=self.device) % self.max_cache_len)

    def update(self, key_states: torch.Tensor, value_states: torch.Tensor, *args, **kwargs) -> tuple[torch.Tensor, torch.Tensor]:
        """Store the new rows (the last C of them if there are more) in their slots, bump both counters, and return what the parent's
        `update` returns for the same history.  Branches on the Python int as the parent does."""
        if not self.is_initialized:
            self.lazy_initialization(key_states, value_states)
        new, cur, size = key_states.shape[-2], self.cumulative_length_int, self.max_cache_len
        # past the fill with several tokens the parent returns what it held in front of the new rows and the new rows: built before any
        # slot is overwritten
        full = None
        if cur >= size and new > 1:          # full: the C - 1 latest positions in front
            idx = self._slots(cur - size + 1, size - 1)
            full = (torch.cat((self.keys.index_select(2, idx), key_states), dim=-2),
                    torch.cat((self.values.index_select(2, idx), value_states), dim=-2))
        elif cur < size < cur + new:         # fills on this update: nothing has wrapped yet (a first prompt: the states themselves)
            full = (key_states, value_states) if cur == 0 else (torch.cat((self.keys[:, :, :cur, :], key_states), dim=-2),
                                                                torch.cat((self.values[:, :, :cur, :], value_states), dim=-2))
        # the rows, by index, with the slot from the device counter (one captured update serves every total)
        kept = min(new, size)
        slots = (torch.arange(kept, device=self.device) + (self.cumulative_length + (new - kept))) % size
        try:
            self.keys.index_copy_(2, slots, key_states[:, :, new - kept:, :])
            self.values.index_copy_(2, slots, value_states[:, :, new - kept:, :])
        except NotImplementedError:
            self.keys[:, :, slots] = key_states[:, :, new - kept:, :]
            self.values[:, :, slots] = value_states[:, :, new - kept:, :]
        self.cumulative_length.add_(new)
        self.cumulative_length_int += new
        if cur + new <= size:                # not past the fill: slot j is position j, as in the parent
            return self.keys, self.values
        if full is None:                     # full, one token: the parent's rolled buffer
            idx = self._slots(cur - size + 1, size)
            return self.keys.index_select(2, idx), self.values.index_select(2, idx)
        return full

    def advance(self, count: int = 1) -> None:
        """Count `count` tokens whose rows a kernel has already stored in their slots (ops.attn_decode_ring's append): both counters, no copy."""
        self.cumulative_length.add_(count)
        self.cumulative_length_int += count


def to_ring(cache):
    """Replace every layer of `cache` that is exactly a StaticSlidingWindowLayer by a RingSlidingWindowLayer of the same size, in place;
    returns `cache`.  ValueError on an offloading cache and on a sliding layer that already holds its buffers."""
    layers = getattr(cache, "layers", None)
    if not isinstance(layers, list):
        raise ValueError("to_ring needs a cache with a list of layers (a transformers StaticCache)")
    if getattr(cache, "offloading", False):
        raise ValueError("to_ring does not serve offloading caches")
    sliding = [i for i, layer in enumerate(layers) if type(layer) is StaticSlidingWindowLayer]
    if any(layers[i].is_initialized for i in sliding):
        raise ValueError("to_ring needs sliding layers that have not been initialised: convert the cache before its first update")
    for i in sliding:
        size = layers[i].max_cache_len   # min(sliding_window, max_cache_len): both arguments of the new layer
        layers[i] = RingSlidingWindowLayer(max_cache_len=size, sliding_window=size)
    return cache


def ring_static_cache(config, max_cache_len: int, **kwargs) -> StaticCache:
    """A `StaticCache(config, max_cache_len, **kwargs)` whose sliding layers are ring layers: hand it to `generate` / the model as
    `past_key_values` to decode past the window without the roll."""
    return to_ring(StaticCache(config, max_cache_len=max_cache_len, **kwargs))
