"""The attention core of a decode step -- one query token against the KV cache -- as one kernel.

Per layer and token transformers runs `past_key_values.update` (torch.cat of the whole K and V on a DynamicCache; arange, add, add_ and two
index_copy_ on a StaticCache) and sdpa or the eager matmul / softmax / matmul over what `update` returned: with a StaticCache all
max_cache_len positions behind a mask.  `ops.attn_decode` (qllm_attn_decode, csrc/attn_decode.hip) reads only the valid keys, each K / V
row once for all query heads of its group, and takes the length from device memory when the cache is static.

`install_fused_attention` gives each whitelisted attention INSTANCE the restated forward of fused_rope.py (one text for both installs: the
class's data flow, no transformers global touched) with `_fused_core` behind the rotary embedding.  The core serves a call when q_len == 1,
q / k / v are device tensors of one fp16 / bf16 type, nothing is being differentiated, the module is not training, the attention
implementation is sdpa or eager, no kwarg changes the mathematics (a `sliding_window` handed in by the caller does), the mask is None or
one of the two forms transformers builds at q_len == 1 ([B, 1, 1, L] bool or additive), the cache layer is EXACTLY a DynamicLayer or an
initialised StaticLayer of a cache that does not offload -- with a sliding window W (config.sliding_window for Mistral, the module's own
for Qwen2) EXACTLY one of the three sliding layers below -- and `ops.attn_decode_plan` serves the shapes:

  DynamicLayer  `update` as before, then the kernel over what it returned with the host length.
  StaticLayer   `update` as before, then the kernel over the layer's buffers with the length read from `layer.cumulative_length` on the
                device: the valid positions, not max_cache_len.  (The append form of the kernel -- two launches instead of update's five
                -- needs a host-side bound on the length that holds across `reset`, `crop` and foreign updates of the layer; it is not
                used here.)

  DynamicSlidingWindowLayer   of that very window W, not recording its past: `update` as before (it returns the W - 1 positions it kept
                and the new ones), then the kernel over what it returned with the host length and `window=W`.
  StaticSlidingWindowLayer    that holds at most W positions: `update` as before, then the kernel with `window=W` over what it returned:
                the layer's buffers with the length from `layer.cumulative_length` on the device while `layer.cumulative_length_int <=
                layer.max_cache_len`; once the layer has overflowed it stops updating that tensor (a 5-token prompt into a window of 4
                leaves it at 0), and everything `update` returns is valid: the host length.  The layer branches on a Python int at the
                point where it fills (index_copy before, roll or cat after), fused or not, so a manually captured step cannot cross that
                point: capture before it or after it.  Past it the layer rolls its whole buffer at every token.  Chunked attention
                and `record_past` are not built.
  RingSlidingWindowLayer      (modeling/ring_cache.py; the caller builds the cache: `ring_static_cache` / `to_ring`) that holds at most W
                positions, position j in slot j mod C: at decode NO `update` -- `ops.attn_decode_ring` over the layer's buffers in
                place with the total from `layer.cumulative_length` on the device and the new rows stored by the kernel, then
                `layer.advance(1)`: no roll, no copy of the cache, no branch on whether the layer is full, so ONE captured step serves
                every length.  Where its plan refuses, `update` (which returns what the static sliding layer's returns) and the
                family's route.  At prefill it is a static sliding layer: `update`, then the same call of `ops.attn_prefill`.
On the full layers the calls carry no `window`.  On the sliding ones a decode call carries it, but it hides nothing there: a dynamic
sliding layer returns at most W positions and a static one holds at most W, so the lowest visible position is 0 and the windowed kernel
reads what the kernel without a window would.  The decode window skips keys only for direct callers of `ops.attn_decode` on a linear
cache longer than the window; through the modules the gain at decode is that sliding layers are served at all (the valid keys, the
length from the device), and the window itself pays at prefill, where `update` returns more than W positions.
QLLM_FUSE_ATTENTION_SLIDING=0 puts every call that a window reaches back on the family's route.

Everything else -- a window on a full layer, a sliding layer without a window or of another window, subclasses of the sliding layers,
quantized and offloaded caches, no cache, CPU and fp32 tensors, training, output_attentions -- runs the family's own route unchanged.
Composes with install_fused_rope and the other installs in any order.
Opt-in: `load_quantized(..., fuse_attention=True)`.

Prefill (q_len >= 2) runs the family's route unless the install is made with `prefill=True` (`load_quantized(...,
fuse_attention_prefill=True)`): then `_fused_core_prefill` hands prompts, continuation chunks and padded batches to `ops.attn_prefill`
(qllm_attn_prefill, csrc/attn_prefill.hip) under the conditions in its docstring, for the (cache layer kind, mask or none, q_len)
combinations of `PREFILL_ROUTES`.  With the flag off nothing changes."""
from __future__ import annotations

import os
from typing import Iterable, Optional

import torch

from ... import ops
from .fused_norm import ATTENTION_TYPES
from .fused_rope import _ACT_DTYPES, _CORE, _known, _patch, _unpatch

# kwargs the decoder layers pass on that do not change what the attention computes; any other one must be None or False
_BENIGN = ("position_ids", "cache_position", "use_cache", "output_hidden_states", "return_dict", "is_causal")


def _on_device(*ts) -> bool:
    return all(t.is_cuda for t in ts)


def _layer_of(past_key_values, layer_idx, uninitialized=False, sliding=None):
    """(the cache layer the core may serve, its kind) or (None, None).  Without a window (`sliding` None): exactly a DynamicLayer
    ("dynamic") or an initialised StaticLayer ("static"; with `uninitialized`: any StaticLayer).  With the window W of the call: exactly a
    DynamicSlidingWindowLayer of that window that does not record its past ("dynamic_sliding"), or exactly a StaticSlidingWindowLayer
    (initialised, or any with `uninitialized`) that holds at most W positions ("static_sliding"), unless QLLM_FUSE_ATTENTION_SLIDING=0.
    Exactly a RingSlidingWindowLayer (modeling/ring_cache.py) under the static sliding layer's conditions: "ring_sliding".
    Always of a cache that does not offload; a window on a full layer, a sliding layer without one and subclasses are not served."""
    from transformers.cache_utils import DynamicLayer, DynamicSlidingWindowLayer, StaticLayer, StaticSlidingWindowLayer
    from ..ring_cache import RingSlidingWindowLayer
    layers = getattr(past_key_values, "layers", None)
    if not isinstance(layers, list) or not isinstance(layer_idx, int) or not 0 <= layer_idx < len(layers) or getattr(past_key_values, "offloading", False):
        return None, None
    layer = layers[layer_idx]
    if sliding is None:
        if type(layer) is DynamicLayer:
            return layer, "dynamic"
        if type(layer) is StaticLayer and (layer.is_initialized or uninitialized):
            return layer, "static"
        return None, None
    if isinstance(sliding, bool) or not isinstance(sliding, int) or sliding < 1 or os.environ.get("QLLM_FUSE_ATTENTION_SLIDING", "1") == "0":
        return None, None
    if type(layer) is DynamicSlidingWindowLayer and layer.sliding_window == sliding and not layer.record_past:
        return layer, "dynamic_sliding"
    if type(layer) is StaticSlidingWindowLayer and layer.max_cache_len <= sliding and (layer.is_initialized or uninitialized):
        return layer, "static_sliding"
    if type(layer) is RingSlidingWindowLayer and layer.max_cache_len <= sliding and (layer.is_initialized or uninitialized):
        return layer, "ring_sliding"
    return None, None


def _length_after_update(layer, kind, keys):
    """The number of valid positions of what `update` returned.  A static layer: its device counter.  A static sliding layer: its device
    counter while the layer has not overflowed (it stops updating the tensor from then on: the tensor is wrong and must not be used), then
    the length of what `update` returned -- all of it is valid.  A dynamic layer of either kind: the length of what `update` returned."""
    if kind == "static" or (kind in ("static_sliding", "ring_sliding") and layer.cumulative_length_int <= layer.max_cache_len):
        return layer.cumulative_length
    return keys.shape[2]


def _gate(self, q, k, v, attention_mask, past_key_values, kwargs, window, rows, uninitialized=False):
    """The conditions both cores share, for a call of `rows` query rows: (the cache layer, its kind, the call's sliding window or None),
    or None for the family's route.  Implementation, training, types, device, autograd, kwargs, the mask's form ([B, 1, rows, L'], bool
    or of the activation type), `_layer_of` (`uninitialized`: a static layer may still be empty) and, on a static layer that holds its
    buffers, their type, batch and head size.  Nothing here touches the cache."""
    if past_key_values is None or self.training or self.config._attn_implementation not in ("sdpa", "eager"):
        return None
    if q.dtype not in _ACT_DTYPES or k.dtype != q.dtype or v.dtype != q.dtype or not _on_device(q, k, v):
        return None
    if torch.is_grad_enabled() and (q.requires_grad or k.requires_grad or v.requires_grad):
        return None
    sliding = getattr(self.config, "sliding_window", None) if window == "config" else getattr(self, "sliding_window", None) if window == "self" else None
    if any(val is not None and val is not False for name, val in kwargs.items() if name not in _BENIGN):
        return None
    if attention_mask is not None and not (isinstance(attention_mask, torch.Tensor) and attention_mask.dim() == 4 and attention_mask.shape[1] == 1
                                           and attention_mask.shape[2] == rows and (attention_mask.dtype == torch.bool or attention_mask.dtype == q.dtype)):
        return None
    layer, kind = _layer_of(past_key_values, self.layer_idx, uninitialized=uninitialized, sliding=sliding)
    if layer is None:
        return None
    if kind in ("static", "static_sliding", "ring_sliding") and layer.is_initialized and (layer.keys.dtype != q.dtype or layer.keys.shape[0] != q.shape[0] or layer.keys.shape[3] != q.shape[3]):
        return None
    return layer, kind, sliding


def _update_and_attend(self, q, k, v, attention_mask, past_key_values, layer, kind, sliding):
    """Behind the last refusal that leaves the cache alone: `update`, once, then ops.attn_decode (one query row) or ops.attn_prefill
    (causal) over what it returned where that op's plan serves it -- with `window=` on a sliding layer only -- else None and the updated
    states for the family's route."""
    keys, values = past_key_values.update(k, v, self.layer_idx)
    length = _length_after_update(layer, kind, keys)
    decode = q.shape[2] == 1
    try:
        plan = (ops.attn_decode_plan if decode else ops.attn_prefill_plan)(q, keys, values, length, mask=attention_mask)
    except ops.QllmUnsupported:
        return None, keys, values, True
    how = {} if decode else {"causal": True}
    if sliding is not None:
        how["window"] = sliding
    with torch.no_grad():
        return (ops.attn_decode if decode else ops.attn_prefill)(q, keys, values, length, mask=attention_mask, scaling=self.scaling, plan=plan, **how), keys, values, True


def _fused_core(self, q, k, v, attention_mask, past_key_values, kwargs, window):
    """(the attention output [B, Hq, D] or None, key states, value states, whether the cache has been updated) of one forward: the kernel
    where the conditions of this file's docstring hold, else None and the states for the family's route."""
    served = _gate(self, q, k, v, attention_mask, past_key_values, kwargs, window, 1) if q.shape[2] == 1 else None
    if served is None:
        return None, k, v, False
    if served[1] == "ring_sliding":
        return _attend_ring(self, q, k, v, attention_mask, past_key_values, served[0])
    return _update_and_attend(self, q, k, v, attention_mask, past_key_values, *served)


def _attend_ring(self, q, k, v, attention_mask, past_key_values, layer):
    """One token on a ring layer: ops.attn_decode_ring over the layer's buffers in place -- the total from `layer.cumulative_length` on the
    device, the new rows stored by the kernel -- then `layer.advance(1)`: no launch touches more than the new rows, and nothing branches
    on whether the layer is full.  The window of the call is the layer's size (min(W, max_cache_len): what a static sliding layer of
    these sizes holds and shows).  Where the plan refuses nothing has touched the cache: `update`, once, and the family's route."""
    try:
        plan = ops.attn_decode_ring_plan(q, layer.keys, layer.values, layer.cumulative_length, layer.max_cache_len, k, v, attention_mask)
    except ops.QllmUnsupported:
        keys, values = past_key_values.update(k, v, self.layer_idx)
        return None, keys, values, True
    with torch.no_grad():
        out = ops.attn_decode_ring(q, layer.keys, layer.values, layer.cumulative_length, layer.max_cache_len, k_new=k, v_new=v, mask=attention_mask,
                                   scaling=self.scaling, plan=plan)
    layer.advance(1)
    return out, layer.keys, layer.values, True


# What `_fused_core_prefill` hands to ops.attn_prefill, by (cache layer kind, whether the call carries a mask): the q_len range (lowest,
# highest; None: no upper end) and whether calls behind already cached tokens are routed too.  Set from profiles/attn_prefill.md, "Module
# routing" (tools/attn_prefill_bench.py; fp16, head_dim 128, S = 16 .. 2048, one MI355X): a combination the kernel loses at a measured
# point stays on the family's route.  Without a mask and on a static layer every measured point wins (1.06 to 13 times).  On a dynamic
# layer with a mask the prompt wins up to 128 rows at all three shapes, is mixed at 512 and 1024 (the 32 / 32 shape loses) and loses at
# 2048, and a chunk of 128 rows behind 1024 cached tokens loses (0.78 to 0.96: B x Hq blocks walk the keys alone, there is no split over
# them), so there only first prompts of at most PREFILL_DYNAMIC_MASKED_MAX_ROWS rows are routed.
PREFILL_DYNAMIC_MASKED_MAX_ROWS = 128


class Windows(float):
    """A q_len bound of PREFILL_ROUTES given in multiples of the call's sliding window."""


PREFILL_ROUTES = {
    ("dynamic", False): (2, None, True),
    ("dynamic", True): (2, PREFILL_DYNAMIC_MASKED_MAX_ROWS, False),
    ("static", False): (2, None, True),
    ("static", True): (2, None, True),
    # The two sliding kinds, by the same rule, from profiles/attn_sliding.md, "Prefill": measured at ONE window, W = 4096
    # (tools/attn_prefill_bench.py --window 4096; fp16, (32, 8, 128) and (32, 32, 128); first prompts of 128 .. 8192 rows and a 128-row
    # chunk behind a full window), so every bound that the window decides is written in windows (`Windows`), not in rows.  An entry may
    # hold several ranges, and an upper end may be the lower of two bounds.  Without a mask (a first prompt shorter than the window on a
    # dynamic sliding layer) every point wins (1.11 to 1.23 times).  With the band mask and the prompt inside half a window -- where the
    # window hides nothing and the call is the masked path of the full layers -- the kernel wins up to 128 rows on a dynamic and up to 2048
    # rows (half the window) on a static sliding layer (1.04 to 9.0 times), and loses at 512 / 2048 rows on the dynamic one.  At one window
    # (4096 rows) it loses on both (0.83 to 0.92: the whole prompt lies inside the window, nothing is skipped and the mask is read byte by
    # byte).  At two windows (8192 rows) it wins (1.48 to 1.63): half the causal triangle lies below the window and is never read; nothing
    # between one and two windows was measured.  The chunk behind a full window loses (0.39 to 0.43: no split over the keys).  A static
    # sliding layer without a mask was not measured (transformers always hands it one): not routed.
    ("dynamic_sliding", False): (2, None, False),
    ("dynamic_sliding", True): ((2, (PREFILL_DYNAMIC_MASKED_MAX_ROWS, Windows(0.5)), False), (Windows(2), None, False)),
    ("static_sliding", False): (1, 0, False),
    ("static_sliding", True): ((2, (2048, Windows(0.5)), False), (Windows(2), None, False)),
}


def _rows(bound, window):
    """A bound of PREFILL_ROUTES in rows: an int, `Windows(x)` (x times the call's window, rounded down), or the lowest of a tuple of these."""
    if isinstance(bound, tuple):
        return min(_rows(b, window) for b in bound)
    return int(bound * window) if isinstance(bound, Windows) else bound


def _prefill_routed(kind: str, masked: bool, q_len: int, behind: bool, window: Optional[int] = None) -> bool:
    """`behind`: the host knows that the layer held tokens before this call (a dynamic layer's length and a static sliding layer's
    Python counter; a static layer's length is on the device).  `window`: the call's sliding window, for the bounds written in windows."""
    entry = PREFILL_ROUTES.get(("static_sliding" if kind == "ring_sliding" else kind, masked), (1, 0, False))
    ranges = entry if isinstance(entry[0], tuple) else (entry,)
    return any(q_len >= _rows(lo, window) and (hi is None or q_len <= _rows(hi, window)) and (chunks or not behind) for lo, hi, chunks in ranges)


def _fused_core_prefill(self, q, k, v, attention_mask, past_key_values, kwargs, window):
    """`_fused_core` for q_len == 1; for q_len >= 2 the same tuple with ops.attn_prefill's [B, S, Hq, D] output: the kernel under
    `_fused_core`'s conditions on types, device, autograd, training, implementation, sliding window, kwargs and cache layer (a StaticLayer
    or StaticSlidingWindowLayer may also be uninitialised: `update` initialises it; on the sliding layers first prompts and continuation
    chunks alike go to the kernel with `window=W`, over what `update` returned), and in addition: the module is causal
    (`self.is_causal`); the mask is None or 4-D [B, 1, S, L'], bool or of the activation type; with mask None the cache layer holds nothing before this call and that is known on the
    host (sdpa's own is_causal rule: a DynamicLayer of length 0, a StaticLayer not yet initialised); `PREFILL_ROUTES` routes the
    combination.  The kernel runs with causal = 1 plus the mask: a hand-made mask that shows a causal model keys above the diagonal is
    not honoured there."""
    if q.shape[2] == 1:
        return _fused_core(self, q, k, v, attention_mask, past_key_values, kwargs, window)
    no = (None, k, v, False)
    s = q.shape[2]
    served = _gate(self, q, k, v, attention_mask, past_key_values, kwargs, window, s, uninitialized=True) if getattr(self, "is_causal", False) else None
    if served is None:
        return no
    layer, kind, sliding = served
    static = kind in ("static", "static_sliding", "ring_sliding")
    held = layer.is_initialized if static else layer.get_seq_length() != 0   # (a static layer: may hold tokens; its length is on the device)
    behind = layer.is_initialized and layer.cumulative_length_int != 0 if kind in ("static_sliding", "ring_sliding") else held and not static
    if not _prefill_routed(kind, attention_mask is not None, s, behind, sliding) or (attention_mask is None and held):
        return no
    return _update_and_attend(self, q, k, v, attention_mask, past_key_values, layer, kind, sliding)


def count_fused_attention_prefill(model: torch.nn.Module) -> int:
    """How many attention modules of `model` carry the prefill core."""
    return sum(1 for mod in model.modules() if _CORE in mod.__dict__ and mod.__dict__[_CORE][3] is _fused_core_prefill)


def install_fused_attention(model: torch.nn.Module, attention_types: Optional[Iterable] = None, prefill: bool = False) -> int:
    """Give every attention module of `model` whose class name is in fused_norm.ATTENTION_TYPES (and in `attention_types`, classes or
    names, when given) and whose forward is the one fused_rope.py restates (`_known`) that restated forward with `_fused_core` in it.  No
    transformers global is touched.  Anything else is left alone and not counted.  Returns the number of modules patched;
    QLLM_FUSE_ATTENTION=0 makes it a no-op that returns 0.  `uninstall_fused_attention` restores exactly what was there, in any order with
    `uninstall_fused_rope`.  `prefill` (opt-in, off by default): the modules get `_fused_core_prefill`, which also serves calls with two
    or more query tokens; QLLM_FUSE_ATTENTION_PREFILL=0 turns the flag into a no-op (the decode core alone is installed)."""
    if os.environ.get("QLLM_FUSE_ATTENTION", "1") == "0":
        return 0
    core = _fused_core_prefill if prefill and os.environ.get("QLLM_FUSE_ATTENTION_PREFILL", "1") != "0" else _fused_core
    names = set(ATTENTION_TYPES)
    if attention_types is not None:
        names &= {t if isinstance(t, str) else t.__name__ for t in attention_types}
    n = 0
    for attn in model.modules():
        if type(attn).__name__ not in names or _CORE in attn.__dict__:
            continue
        known = _known(attn)
        if known is None:
            continue
        _patch(attn, _CORE, known + (core,))
        n += 1
    return n


def uninstall_fused_attention(model: torch.nn.Module) -> int:
    """Undo `install_fused_attention`.  Returns how many modules were restored."""
    n = 0
    for mod in model.modules():
        if _CORE in mod.__dict__:
            _unpatch(mod, _CORE)
            n += 1
    return n
