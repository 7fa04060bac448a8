"""The two residual adds of a decoder layer, folded into the launches in front of them.

`hidden = residual + self_attn(norm(hidden))` and `hidden = residual + mlp(norm(hidden))`: two elementwise kernels behind o_proj and
down_proj.  At one row the batch-1 kernel's 16 storing threads can add the residual themselves (csrc/strip1_resid.hip,
csrc/strip1_swiglu_resid.hip; `HipForwardMixin.forward_residual` / `forward_swiglu_residual`), bit for bit the eager add.  The add lives in
the decoder layer and the launch two modules below it, so `install_fused_residual` replaces the layer's forward by one with the class's
data flow that ARMS o_proj (down_proj) with the residual around the attention (MLP) call: the q_layer's next forward takes the armed
tensor, returns `forward_residual(x, residual)` -- the fused launch where it is served, else the eager add inside the wrapper -- and the
layer skips its own add.  A residual nobody took (an attention that never calls o_proj, a leading shape that does not match) is added by
the layer as before; it never outlives the layer call.  With `install_fused_mlp` in place the armed down_proj is reached through
`forward_swiglu` and answers `forward_swiglu_residual`.  The norm calls stay module calls, so `install_fused_norm` composes in any order;
nothing is ever written in place into the residual tensor (fused_norm keys its caches on tensor identity and version).  Opt-in:
`load_quantized(..., fuse_residual=True)`."""
from __future__ import annotations

import inspect
import os
import types
from typing import Iterable, Optional

import torch

from .fused_mlp import DEFAULT_MLP_TYPES
from .fused_norm import ATTENTION_TYPES, DEFAULT_LAYER_TYPES

_LAYER = "_qllm_unfused_layer_forward"   # on a decoder layer: (the instance forward it had or None, o_proj's slot, down_proj's slot, {parameter: default})
_ARMED = "_qllm_armed_residual"          # on a q_layer: (its slot, the instance forward it had or None, the instance forward_swiglu it had or None)


class _Slot:
    """The residual one decoder layer hands to one q_layer for the duration of one attention / MLP call."""
    __slots__ = ("residual", "consumed")

    def __init__(self):
        self.residual, self.consumed = None, False

    def arm(self, residual: torch.Tensor):
        self.residual, self.consumed = residual, False

    def disarm(self):
        self.residual = None

    def take(self, x: torch.Tensor, n: int) -> Optional[torch.Tensor]:
        """The armed residual for the q_layer's call on `x`, once; None (and disarmed) when there is none or its shape is not this call's."""
        r, self.residual = self.residual, None
        if r is None or r.shape != x.shape[:-1] + (n,):
            return None
        self.consumed = True
        return r


def _q_forward(self, x):
    slot, orig, _ = self.__dict__[_ARMED]
    r = slot.take(x, self.outfeatures)
    if r is None:
        return (orig if orig is not None else types.MethodType(type(self).forward, self))(x)
    return self.forward_residual(x, r)          # (its fallback, residual + self(x), comes back here with the slot empty)


def _q_forward_swiglu(self, gate, up):
    slot, _, orig = self.__dict__[_ARMED]
    r = slot.take(gate, self.outfeatures)
    if r is None:
        return (orig if orig is not None else types.MethodType(type(self).forward_swiglu, self))(gate, up)
    return self.forward_swiglu_residual(gate, up, r)


def _layer_forward(self, hidden_states, *args, **kwargs):
    _, o_slot, d_slot, defaults = self.__dict__[_LAYER]
    if len(args) > len(defaults):                # (as strict as the class's forward)
        raise TypeError(f"forward() takes from 2 to {len(defaults) + 2} positional arguments but {len(args) + 2} were given")
    given = dict(defaults)                       # (the class hands self_attn every named parameter of its own, defaults included, and **kwargs)
    given.update(zip(defaults, args))
    twice = [k for k in list(defaults)[:len(args)] if k in kwargs]
    if twice:
        raise TypeError(f"forward() got multiple values for argument '{twice[0]}'")
    given.update(kwargs)
    residual = hidden_states
    h = self.input_layernorm(hidden_states)
    o_slot.arm(residual)
    try:
        a = self.self_attn(hidden_states=h, **given)
    finally:
        o_slot.disarm()
    a = a[0] if isinstance(a, tuple) else a
    h = a if o_slot.consumed else residual + a
    residual = h
    n = self.post_attention_layernorm(h)
    d_slot.arm(residual)
    try:
        m = self.mlp(n)
    finally:
        d_slot.disarm()
    return m if d_slot.consumed else residual + m


def _signature_names(cls):
    """{name: default} of `cls.forward`'s parameters behind hidden_states, in order, when it is the decoder-layer contract this module
    knows -- forward(self, hidden_states, <positional-or-keyword parameters with defaults>, **kwargs) -> torch.Tensor -- else None.
    A forward with keyword-only parameters or *args is refused too: positional arguments are mapped onto these names in order."""
    try:
        sig = inspect.signature(cls.forward)
    except (TypeError, ValueError):
        return None
    if sig.return_annotation not in (torch.Tensor, "torch.Tensor", "Tensor"):
        return None
    params = list(sig.parameters.values())
    if len(params) < 2 or params[1].name != "hidden_states":
        return None
    defaults = {}
    for p in params[2:]:
        if p.kind == p.VAR_KEYWORD:
            continue
        if p.kind != p.POSITIONAL_OR_KEYWORD or p.default is p.empty:
            return None
        defaults[p.name] = p.default
    return defaults


def install_fused_residual(model: torch.nn.Module, q_layer_types, layer_types: Optional[Iterable] = None) -> int:
    """Patch the decoder layers of `model` whose class name is in fused_norm.DEFAULT_LAYER_TYPES (and in `layer_types`, classes or names,
    when given), whose self_attn is an attention class of fused_norm.ATTENTION_TYPES and whose mlp is one of fused_mlp.DEFAULT_MLP_TYPES,
    whose self_attn.o_proj and mlp.down_proj are q_layers with `forward_residual`, and whose class's forward takes hidden_states first and
    is annotated to return torch.Tensor (the decoder-layer contract of transformers 5: tuple-returning layers of older releases are not
    guessed at).  Anything else -- tensor-parallel wrappers included: they are no q_layers -- is left alone.  Returns the number of layers
    patched; QLLM_FUSE_RESIDUAL=0 makes it a no-op that returns 0.  `uninstall_fused_residual` restores exactly what was there."""
    if os.environ.get("QLLM_FUSE_RESIDUAL", "1") == "0":
        return 0
    names = set(DEFAULT_LAYER_TYPES)
    if layer_types is not None:
        names &= {t if isinstance(t, str) else t.__name__ for t in layer_types}
    q_types = tuple(q_layer_types)
    n = 0
    for layer in model.modules():
        if type(layer).__name__ not in names or _LAYER in layer.__dict__:
            continue
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if type(attn).__name__ not in ATTENTION_TYPES or type(mlp).__name__ not in DEFAULT_MLP_TYPES:
            continue
        o_proj, down_proj = getattr(attn, "o_proj", None), getattr(mlp, "down_proj", None)
        if not all(isinstance(q, q_types) and hasattr(q, "forward_residual") and _ARMED not in q.__dict__ for q in (o_proj, down_proj)):
            continue
        if o_proj is down_proj or not all(isinstance(getattr(layer, nm, None), torch.nn.Module) for nm in ("input_layernorm", "post_attention_layernorm")):
            continue
        params = _signature_names(type(layer))
        if params is None:
            continue
        slots = (_Slot(), _Slot())
        for q, slot in zip((o_proj, down_proj), slots):
            setattr(q, _ARMED, (slot, q.__dict__.get("forward"), q.__dict__.get("forward_swiglu")))
            q.forward = types.MethodType(_q_forward, q)
            q.forward_swiglu = types.MethodType(_q_forward_swiglu, q)
        setattr(layer, _LAYER, (layer.__dict__.get("forward"),) + slots + (params,))
        layer.forward = types.MethodType(_layer_forward, layer)
        n += 1
    return n


def uninstall_fused_residual(model: torch.nn.Module) -> int:
    """Undo `install_fused_residual`: every patched decoder layer and q_layer computes through the forward it had.  Returns how many
    decoder layers were restored."""
    n = 0
    for mod in model.modules():
        if _ARMED in mod.__dict__:
            _, orig, orig_swiglu = mod.__dict__.pop(_ARMED)
            for name, had in (("forward", orig), ("forward_swiglu", orig_swiglu)):
                if had is None:
                    mod.__dict__.pop(name, None)
                else:
                    setattr(mod, name, had)
        if _LAYER in mod.__dict__:
            orig = mod.__dict__.pop(_LAYER)[0]
            if orig is None:
                mod.__dict__.pop("forward", None)
            else:
                mod.forward = orig
            n += 1
    return n
