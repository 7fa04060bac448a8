"""SwiGLU MLPs with the elementwise product folded into the down-projection's launch.

`act_fn(gate_proj(x)) * up_proj(x)` feeds `down_proj`: a separate elementwise kernel and an [M, K] round trip between two linear launches.
The batch-1 kernel stages every element of its input through registers anyway, so the product can be formed there
(csrc/strip1_swiglu.hip, `HipForwardMixin.forward_swiglu`).  `install_fused_mlp` replaces the `forward` of the MLP modules it recognises
by `down_proj.forward_swiglu(gate_proj(x), up_proj(x))`; gate_proj / up_proj keep going through their sibling group, so a decode step
of the MLP is two launches.  Calls the modules do not send to the fused entry (more than `swiglu_max_m` rows -- one, by measurement: profiles/swiglu.md) or that it
does not serve (other widths, act-order ...) fall back, inside
`forward_swiglu`, to exactly the expression the module computed before.  The reference's counterpart was its fused_mlp /
QuantLlamaMLP (qllm/modeling/q_layers/__init__.py:4, import commented out)."""
from __future__ import annotations

import os
import types
from typing import Iterable, Optional

import torch

DEFAULT_MLP_TYPES = ("LlamaMLP", "MistralMLP", "Qwen2MLP")
_ORIGINAL = "_qllm_unfused_forward"


def _is_silu(fn) -> bool:
    if isinstance(fn, torch.nn.SiLU) or fn is torch.nn.functional.silu:
        return True
    # transformers' ACT2FN["silu"]: torch.nn.SiLU in older releases, in recent ones a module of its own whose forward is
    # torch.nn.functional.silu (transformers.activations.SiLUActivation) -- what a loaded LlamaMLP actually carries
    cls = type(fn)
    return cls.__name__ == "SiLUActivation" and cls.__module__.startswith("transformers.")


def _fused_forward(self, x):
    return self.down_proj.forward_swiglu(self.gate_proj(x), self.up_proj(x))


def _eligible(mod: torch.nn.Module, names: set, q_types: tuple) -> bool:
    if type(mod).__name__ not in names or hasattr(mod, _ORIGINAL):
        return False
    # exactly the structure down_proj(act_fn(gate_proj(x)) * up_proj(x)): three q_layers and a SiLU; anything else is not guessed at
    subs = [getattr(mod, n, None) for n in ("gate_proj", "up_proj", "down_proj")]
    if not all(isinstance(s, q_types) and hasattr(s, "forward_swiglu") for s in subs):
        return False
    if getattr(getattr(mod, "config", None), "mlp_bias", False) or getattr(getattr(mod, "config", None), "pretraining_tp", 1) not in (1, None):
        return False
    return _is_silu(getattr(mod, "act_fn", None))


def install_fused_mlp(model: torch.nn.Module, q_layer_types, mlp_types: Optional[Iterable] = None) -> int:
    """Patch every SwiGLU MLP of `model` whose class (or class name) is in `mlp_types` -- default LlamaMLP, MistralMLP, Qwen2MLP --
    and whose gate_proj / up_proj / down_proj are all q_layers with a SiLU act_fn (torch.nn.SiLU, torch.nn.functional.silu, or transformers' SiLUActivation).  Returns the number of modules patched;
    QLLM_FUSE_MLP=0 makes it a no-op that returns 0.  `uninstall_fused_mlp` restores the original forwards."""
    if os.environ.get("QLLM_FUSE_MLP", "1") == "0":
        return 0
    names = {t if isinstance(t, str) else t.__name__ for t in (DEFAULT_MLP_TYPES if mlp_types is None else mlp_types)}
    q_types = tuple(q_layer_types)
    n = 0
    for mod in model.modules():
        if not _eligible(mod, names, q_types):
            continue
        # (the instance's own forward, if it has one, else the marker None: uninstall puts back exactly what was there)
        setattr(mod, _ORIGINAL, mod.__dict__.get("forward"))
        mod.forward = types.MethodType(_fused_forward, mod)
        n += 1
    return n


def uninstall_fused_mlp(model: torch.nn.Module) -> int:
    """Undo `install_fused_mlp`: every patched module computes through its class's forward again.  Returns how many were restored."""
    n = 0
    for mod in model.modules():
        if _ORIGINAL not in mod.__dict__:
            continue
        orig = mod.__dict__.pop(_ORIGINAL)
        if orig is None:
            mod.__dict__.pop("forward", None)
        else:
            mod.forward = orig
        n += 1
    return n
