"""RMSNorm as one kernel, and folded into the grouped launch of the layers it feeds.

A Llama-style decoder layer runs two RMSNorms, each in front of one sibling group: `input_layernorm` feeds q/k/v, `post_attention_layernorm`
feeds gate/up.  transformers' eager norm is about eight tiny kernels.  `install_fused_norm` makes the norm module the identity and wraps
the forwards of the layers behind it: at one row, when those layers are exactly one `SiblingGroup`, the group's launch forms the norm
while it stages its input (`ops.linear_forward_rmsnorm`, csrc/strip1_norm.hip) and the siblings' outputs are parked as the group parks
them today, keyed on the un-normed tensor; every other call -- more rows, a refusal (remembered), partitioned mixed-precision siblings,
a disabled group, act-order members, CPU tensors, grad mode -- computes the norm once per distinct tensor (`PreNorm.apply`: one
`ops.rmsnorm` kernel, csrc/rmsnorm.hip, or the original module where that kernel does not apply) and hands it to the layer's unwrapped
forward, so today's grouping by tensor identity keeps working.  `make_quant_norm` gives every remaining whitelisted RMSNorm (the final
`model.norm`) a forward on `ops.rmsnorm`.  Opt-in: `load_quantized(..., fuse_norm=True)`.

The fused launch and the standalone kernel sum the squares in different (each fixed) orders: their outputs may differ from each other and
from the eager module in rare last-bit roundings of the normed activation (DESIGN.md has the measured shares).  Once a group has
switched itself off (three launches whose parked outputs nobody collected) the layers go on with the standalone kernel.

The reference's counterpart is its TritonLlamaRMSNorm / make_quant_norm (qllm/modeling/q_layers/triton_norm.py; import commented out in
q_layers/__init__.py next to the fused MLP's)."""
from __future__ import annotations

import os
import types
import weakref
from typing import Iterable, Optional

import torch

from ... import ops
from ._hip_forward import autogptq_compat, tensor_version
from .fused_mlp import DEFAULT_MLP_TYPES

DEFAULT_LAYER_TYPES = ("LlamaDecoderLayer", "MistralDecoderLayer", "Qwen2DecoderLayer")
DEFAULT_NORM_TYPES = ("LlamaRMSNorm", "MistralRMSNorm", "Qwen2RMSNorm")
ATTENTION_TYPES = tuple(f"{fam}{kind}" for fam in ("Llama", "Mistral", "Qwen2") for kind in ("Attention", "SdpaAttention", "FlashAttention2", "FlashAttention"))
_ORIGINAL = "_qllm_unfused_norm_forward"   # on a norm module: the instance forward it had (None: the class's)
_PRENORM = "_qllm_prenorm"                 # on a consumer: (PreNorm, the instance forward it had or None)
_ACT_DTYPES = (torch.float16, torch.bfloat16)


def _original_forward(mod, orig):
    return orig if orig is not None else types.MethodType(type(mod).forward, mod)


def _kernel_applies(x: torch.Tensor, weight: torch.Tensor) -> bool:
    """`ops.rmsnorm` computes this call: device tensors of one activation type, contiguous and 16-byte aligned, nothing to differentiate."""
    return (x.is_cuda and weight.is_cuda and x.dtype in _ACT_DTYPES and weight.dtype == x.dtype and x.dim() >= 1 and x.shape[-1] == weight.shape[0]
            and x.shape[-1] % 8 == 0 and x.shape[-1] <= 65536 and x.is_contiguous() and weight.is_contiguous()
            and x.data_ptr() % 16 == 0 and weight.data_ptr() % 16 == 0
            and not (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)))


class PreNorm:
    """The norm in front of one set of consumers (q/k/v or gate/up): its weight and epsilon, the original module for the calls the kernels
    do not take, the normed tensor of the last input (so that every consumer is handed the SAME tensor object), and whether the fused
    entry refused this group."""
    # the most rows the wrapped forwards send to the fused entry (it serves one); 0: never -- the standalone kernel in front of today's
    # launch.  Measured: profiles/rmsnorm.md; QLLM_FUSE_NORM_MAX_M moves it
    norm_max_m = int(os.environ.get("QLLM_FUSE_NORM_MAX_M", "1"))

    def __init__(self, norm: torch.nn.Module, original, consumers):
        self.norm = norm
        self.original = original          # the norm's instance forward before install (None: its class's forward)
        self.consumers = tuple(consumers)
        self.refused = False              # the fused entry refused this group once: not asked again
        self.fused_launches = 0
        self._x = None                    # weak reference to the tensor `_y` was computed from (never keeps the input alive)
        self._ver = -1
        self._y = None

    @property
    def weight(self):
        return self.norm.weight

    @property
    def eps(self) -> float:
        return float(self.norm.variance_epsilon)

    def apply(self, x: torch.Tensor) -> torch.Tensor:
        """RMSNorm(x): the same tensor object for the same (x, version), so the consumers' sibling group sees one input."""
        held = self._x() if self._x is not None else None
        if held is x and tensor_version(x) == self._ver and self._y is not None:
            return self._y
        w = self.weight
        if _kernel_applies(x, w):
            with torch.no_grad():
                y = ops.rmsnorm(x, w.detach(), self.eps)
        else:
            y = _original_forward(self.norm, self.original)(x)
        self._x, self._ver, self._y = weakref.ref(x), tensor_version(x), y
        return y

    def forget(self):
        self._x, self._ver, self._y = None, -1, None

    def fused(self, layer, x: torch.Tensor) -> Optional[torch.Tensor]:
        """`layer`'s output from the group's fused launch on the un-normed x, or None: the caller norms and runs the layer itself."""
        g = getattr(layer, "_siblings", None)
        if g is None or not g.enabled or self.refused:
            return None
        azb = autogptq_compat() if layer._layout_name() == "GPTQ" else 0
        key = id(layer)
        held = g._x() if g._x is not None else None
        if held is x and tensor_version(x) == g._ver and azb == g._azb and key in g._parked:
            out = g._parked.pop(key)      # (parked by a sibling's fused launch on this very tensor)
            g._misses = 0
            if not g._parked:
                g._x = None
            return out
        w = self.weight
        k = x.shape[-1]
        if (self.norm_max_m < 1 or x.numel() != k or not _kernel_applies(x, w) or len(g.layers) != len(self.consumers)
                or {id(l) for l in g.layers} != {id(l) for l in self.consumers} or not g.compatible()):
            return None
        for l in g.layers:
            resolve = getattr(l, "_resolve_act_order", None)   # (GPTQ detects act-order lazily)
            if resolve is not None:
                resolve()
            if getattr(l, "act_order", None):
                return None
        if g._parked:   # the previous launch's parked outputs were never asked for: the group's own rule (SiblingGroup.forward_for)
            g._misses += 1
            if g._misses >= 3:
                g.enabled = False
        g._x, g._parked = None, {}
        if not g.enabled:
            return None
        try:
            descs = [l.decode_descriptor(None, azb) for l in g.layers]
            with torch.no_grad():
                outs = ops.linear_forward_rmsnorm(descs, x.view(1, k), w.detach(), self.eps)
        except ops.QllmUnsupported:
            self.refused = True
            return None
        g.grouped_launches += 1
        self.fused_launches += 1
        shape = x.shape[:-1]
        mine = None
        for l, o in zip(g.layers, outs):
            o = o.reshape(shape + (l.outfeatures,))
            if l is layer:
                mine = o
            else:
                g._parked[id(l)] = o
        g._x, g._ver, g._azb = weakref.ref(x), tensor_version(x), azb
        return mine


def _identity(self, hidden_states):
    return hidden_states


def _consumer_forward(self, x):
    pre, orig = self.__dict__[_PRENORM]
    y = pre.fused(self, x)
    if y is not None:
        return y
    return _original_forward(self, orig)(pre.apply(x))


def _norm_forward(self, hidden_states):
    if _kernel_applies(hidden_states, self.weight):
        with torch.no_grad():
            return ops.rmsnorm(hidden_states, self.weight.detach(), float(self.variance_epsilon))
    return _original_forward(self, self.__dict__[_ORIGINAL])(hidden_states)


def _norm_ok(norm, names: set, k: int) -> bool:
    w = getattr(norm, "weight", None)
    return (isinstance(norm, torch.nn.Module) and type(norm).__name__ in names and _ORIGINAL not in norm.__dict__
            and isinstance(w, torch.Tensor) and w.dim() == 1 and (k is None or w.shape[0] == k)
            and isinstance(getattr(norm, "variance_epsilon", None), float))


def _pair(norm, consumers, norm_names: set, q_types: tuple):
    """The (norm, consumers) pair is exactly a weight-and-epsilon RMSNorm in front of q_layers of one input width, none patched yet."""
    if not all(isinstance(c, q_types) and hasattr(c, "decode_descriptor") and _PRENORM not in c.__dict__ for c in consumers):
        return False
    k = consumers[0].infeatures
    return all(c.infeatures == k for c in consumers) and _norm_ok(norm, norm_names, k)


def install_fused_norm(model: torch.nn.Module, q_layer_types, layer_types: Optional[Iterable] = None) -> int:
    """Patch the decoder layers of `model` whose class (or class name) is in `layer_types` -- default LlamaDecoderLayer,
    MistralDecoderLayer, Qwen2DecoderLayer -- and whose structure is the one this module knows: input_layernorm feeds
    self_attn.{q,k,v}_proj (an attention class of those families), post_attention_layernorm feeds mlp.{gate,up}_proj (an MLP class of
    fused_mlp.DEFAULT_MLP_TYPES), every consumer a q_layer of the norm's width, the norm a module with a 1-D `weight` and a float
    `variance_epsilon`.  Anything else is not guessed at (Gemma's 1 + w norm: not on the list).  Returns the number of norms folded;
    QLLM_FUSE_NORM=0 makes it a no-op that returns 0.  `uninstall_fused_norm` restores the original forwards."""
    if os.environ.get("QLLM_FUSE_NORM", "1") == "0":
        return 0
    names = {t if isinstance(t, str) else t.__name__ for t in (DEFAULT_LAYER_TYPES if layer_types is None else layer_types)}
    norm_names = set(DEFAULT_NORM_TYPES)
    q_types = tuple(q_layer_types)
    n = 0
    for layer in model.modules():
        if type(layer).__name__ not in names:
            continue
        attn, mlp = getattr(layer, "self_attn", None), getattr(layer, "mlp", None)
        if type(attn).__name__ not in ATTENTION_TYPES or type(mlp).__name__ not in DEFAULT_MLP_TYPES:
            continue
        for norm_name, parent, subs in (("input_layernorm", attn, ("q_proj", "k_proj", "v_proj")), ("post_attention_layernorm", mlp, ("gate_proj", "up_proj"))):
            norm = getattr(layer, norm_name, None)
            consumers = [getattr(parent, s, None) for s in subs]
            if not _pair(norm, consumers, norm_names, q_types):
                continue
            pre = PreNorm(norm, norm.__dict__.get("forward"), consumers)
            setattr(norm, _ORIGINAL, pre.original)
            norm.forward = types.MethodType(_identity, norm)
            for c in consumers:
                setattr(c, _PRENORM, (pre, c.__dict__.get("forward")))
                c.forward = types.MethodType(_consumer_forward, c)
            n += 1
    return n


def make_quant_norm(model: torch.nn.Module, norm_types: Optional[Iterable] = None) -> int:
    """Give every whitelisted RMSNorm of `model` that `install_fused_norm` did not fold (the final `model.norm`; all of them when nothing
    was installed) a forward on `ops.rmsnorm`; calls the kernel does not take (CPU tensors, other dtypes, grad mode) run the original
    forward.  Returns the number of modules patched; QLLM_FUSE_NORM=0: none.  The reference's name (triton_norm.py)."""
    if os.environ.get("QLLM_FUSE_NORM", "1") == "0":
        return 0
    names = {t if isinstance(t, str) else t.__name__ for t in (DEFAULT_NORM_TYPES if norm_types is None else norm_types)}
    n = 0
    for mod in model.modules():
        if not _norm_ok(mod, names, None):
            continue
        setattr(mod, _ORIGINAL, mod.__dict__.get("forward"))
        mod.forward = types.MethodType(_norm_forward, mod)
        n += 1
    return n


def _restore(mod, orig):
    if orig is None:
        mod.__dict__.pop("forward", None)
    else:
        mod.forward = orig


def uninstall_fused_norm(model: torch.nn.Module) -> int:
    """Undo `install_fused_norm` and `make_quant_norm`: every patched norm and consumer computes through the forward it had.  Returns
    how many norm modules were restored."""
    n = 0
    for mod in model.modules():
        if _PRENORM in mod.__dict__:
            pre, orig = mod.__dict__.pop(_PRENORM)
            pre.forget()
            g = getattr(mod, "_siblings", None)
            if g is not None:   # (outputs parked on an un-normed tensor must not meet the plain forward)
                g._x, g._parked = None, {}
            _restore(mod, orig)
        if _ORIGINAL in mod.__dict__:
            _restore(mod, mod.__dict__.pop(_ORIGINAL))
            n += 1
    return n
