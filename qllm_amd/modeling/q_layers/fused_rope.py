"""The rotary position embedding of q and k as one kernel.

transformers' `apply_rotary_pos_emb` -- `q * cos + rotate_half(q) * sin`, the same for k -- is neg, cat, mul, mul, add per tensor: ten
elementwise kernels per decoder layer and token.  `ops.rope` (qllm_rope, csrc/rope.hip) is one, bit for bit.  The function is a global of
the model family's module and the attention's forward looks it up there, so there is no module call to wrap, and patching the global
would change every other model in the process.  `install_fused_rope` instead gives each whitelisted attention INSTANCE a forward that
restates the class's data flow -- q/k/v projections, view / transpose, rotary, `past_key_values.update`,
`ALL_ATTENTION_FUNCTIONS.get_interface`, reshape, o_proj; Llama's, Mistral's and Qwen2's differ in the `sliding_window` they hand to the
attention interface only -- with `apply_rotary` in the place of the module's function.  `apply_rotary` runs the kernel where it applies
(device tensors of one fp16 / bf16 type, no autograd graph being recorded, what `ops.rope_plan` serves) and the eager function of the
attention's own module everywhere else: fp32 cos / sin, partial rotary, odd head sizes, CPU tensors, training.  The q/k/v and o_proj
modules are called as modules, so `install_fused_norm`, `install_fused_mlp` and `install_fused_residual` compose in any order.
Opt-in: `load_quantized(..., fuse_rope=True)`."""
from __future__ import annotations

import inspect
import os
import sys
import types
from typing import Iterable, Optional

import torch

from ... import ops
from .fused_norm import ATTENTION_TYPES

_ATTN = "_qllm_unfused_attention_forward"   # on an attention module: (the instance forward it had or None, the eager rotary function, how it finds its sliding window)
_CORE = "_qllm_unfused_attention_core"      # fused_attention.py's record on an attention module: the same three, and its attention core
_KNOWN = ("hidden_states", "position_embeddings", "attention_mask", "past_key_values")
_ACT_DTYPES = (torch.float16, torch.bfloat16)


def _kernel_applies(q, k, cos, sin, unsqueeze_dim: int = 1):
    """What `ops.rope_plan` answers when `ops.rope` computes this call -- device tensors of one activation type, nothing to differentiate,
    a shape and layout the entry serves -- else None."""
    ts = (q, k, cos, sin)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts):
        return None
    return _shape_applies(q, k, cos, sin, unsqueeze_dim)


def _shape_applies(q, k, cos, sin, unsqueeze_dim: int = 1):
    ts = (q, k, cos, sin)
    if q.dtype not in _ACT_DTYPES or any(t.dtype != q.dtype for t in ts):
        return None
    if torch.is_grad_enabled() and any(t.requires_grad for t in ts):
        return None
    try:
        return ops.rope_plan(q, k, cos, sin, unsqueeze_dim)
    except ops.QllmUnsupported:
        return None


def apply_rotary(eager, q, k, cos, sin, unsqueeze_dim: int = 1):
    """`eager(q, k, cos, sin, unsqueeze_dim)` -- the apply_rotary_pos_emb of a model family -- as one kernel where it applies."""
    plan = _kernel_applies(q, k, cos, sin, unsqueeze_dim)
    if plan is None:
        return eager(q, k, cos, sin, unsqueeze_dim)
    with torch.no_grad():
        return ops.rope(q, k, cos, sin, unsqueeze_dim, plan=plan)


def _attention_forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
    """LlamaAttention.forward / MistralAttention.forward / Qwen2Attention.forward of transformers 5 -- the ONE restatement, shared with
    fused_attention.py -- with `apply_rotary` where install_fused_rope put it (`_ATTN`) and the fused attention core where
    install_fused_attention put it (`_CORE`); either may be there without the other."""
    rope, core = self.__dict__.get(_ATTN), self.__dict__.get(_CORE)
    _, eager_rotary, window = (rope or core)[:3]
    family = sys.modules[type(self).__module__]
    input_shape = hidden_states.shape[:-1]
    hidden_shape = (*input_shape, -1, self.head_dim)
    query_states = self.q_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    key_states = self.k_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    value_states = self.v_proj(hidden_states).view(hidden_shape).transpose(1, 2)
    cos, sin = position_embeddings
    if rope is not None:
        query_states, key_states = apply_rotary(eager_rotary, query_states, key_states, cos, sin)
    else:
        query_states, key_states = eager_rotary(query_states, key_states, cos, sin)
    updated = False
    if core is not None:
        # (the core's output [B, Hq, D], or None), and the key / value states after the cache update where the core has made it
        attn_output, key_states, value_states, updated = core[3](self, query_states, key_states, value_states, attention_mask, past_key_values, kwargs, window)
        if attn_output is not None:
            return self.o_proj(attn_output.reshape(*input_shape, -1)), None
    if past_key_values is not None and not updated:
        key_states, value_states = past_key_values.update(key_states, value_states, self.layer_idx)
    attention_interface = family.ALL_ATTENTION_FUNCTIONS.get_interface(self.config._attn_implementation, family.eager_attention_forward)
    if window == "config":      # Mistral
        kwargs = dict(kwargs, sliding_window=getattr(self.config, "sliding_window", None))
    elif window == "self":      # Qwen2
        kwargs = dict(kwargs, sliding_window=self.sliding_window)
    attn_output, attn_weights = attention_interface(self, query_states, key_states, value_states, attention_mask,
                                                    dropout=0.0 if not self.training else self.attention_dropout, scaling=self.scaling, **kwargs)
    attn_output = attn_output.reshape(*input_shape, -1).contiguous()
    return self.o_proj(attn_output), attn_weights


def _patch(attn, key: str, value: tuple) -> None:
    """Record `value` under `key` (`_ATTN` or `_CORE`) on an attention module and give it the restated forward, unless the other install
    has done so already; the instance forward it had before either (or None) is kept with both records."""
    other = attn.__dict__.get(_CORE if key == _ATTN else _ATTN)
    if other is None:
        orig = attn.__dict__.get("forward")
        attn.forward = types.MethodType(_attention_forward, attn)
    else:
        orig = other[0]
    setattr(attn, key, (orig,) + value)


def _unpatch(mod, key: str) -> None:
    """Undo `_patch`: drop the record; when the other install's is gone too, the module gets back the forward it had."""
    orig = mod.__dict__.pop(key)[0]
    if (_CORE if key == _ATTN else _ATTN) in mod.__dict__:
        return
    if orig is None:
        mod.__dict__.pop("forward", None)
    else:
        mod.forward = orig


def _known(attn):
    """(the eager rotary function, where the sliding window comes from) of an attention module this file can restate, else None: a class of
    fused_norm.ATTENTION_TYPES whose forward has the known parameters -- hidden_states, position_embeddings, attention_mask,
    past_key_values, **kwargs -- and nothing else, whose module holds the three globals the forward uses, and which has the attributes."""
    name = type(attn).__name__
    if name not in ATTENTION_TYPES:
        return None
    try:
        params = list(inspect.signature(type(attn).forward).parameters.values())[1:]
    except (TypeError, ValueError):
        return None
    if tuple(p.name for p in params[:-1]) != _KNOWN or params[-1].kind != params[-1].VAR_KEYWORD or any(p.kind != p.POSITIONAL_OR_KEYWORD for p in params[:-1]):
        return None
    family = sys.modules.get(type(attn).__module__)
    eager = getattr(family, "apply_rotary_pos_emb", None)
    if not callable(eager) or not hasattr(family, "ALL_ATTENTION_FUNCTIONS") or not callable(getattr(family, "eager_attention_forward", None)):
        return None
    if not all(isinstance(getattr(attn, n, None), torch.nn.Module) for n in ("q_proj", "k_proj", "v_proj", "o_proj")):
        return None
    if not all(hasattr(attn, n) for n in ("head_dim", "layer_idx", "config", "scaling", "attention_dropout")):
        return None
    window = "config" if name.startswith("Mistral") else "self" if name.startswith("Qwen2") else None
    if window == "self" and not hasattr(attn, "sliding_window"):
        return None
    return eager, window


def install_fused_rope(model: torch.nn.Module, attention_types: Optional[Iterable] = None) -> int:
    """Give every attention module of `model` whose class name is in fused_norm.ATTENTION_TYPES (and in `attention_types`, classes or
    names, when given) and whose forward is the one this file knows (`_known`) an instance forward with `apply_rotary` in the place of
    the family's apply_rotary_pos_emb.  No transformers global is touched.  Anything else is left alone and not counted.  Returns the
    number of modules patched; QLLM_FUSE_ROPE=0 makes it a no-op that returns 0.  `uninstall_fused_rope` restores exactly what was there."""
    if os.environ.get("QLLM_FUSE_ROPE", "1") == "0":
        return 0
    names = set(ATTENTION_TYPES)
    if attention_types is not None:
        names &= {t if isinstance(t, str) else t.__name__ for t in attention_types}
    n = 0
    for attn in model.modules():
        if type(attn).__name__ not in names or _ATTN in attn.__dict__:
            continue
        known = _known(attn)
        if known is None:
            continue
        _patch(attn, _ATTN, known)
        n += 1
    return n


def uninstall_fused_rope(model: torch.nn.Module) -> int:
    """Undo `install_fused_rope`: every patched attention computes through the forward it had.  Returns how many were restored."""
    n = 0
    for mod in model.modules():
        if _ATTN in mod.__dict__:
            _unpatch(mod, _ATTN)
            n += 1
    return n
