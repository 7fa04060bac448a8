"""What the install / uninstall pairs of the opt-in fusions (fused_mlp, fused_norm, fused_residual, fused_rope, fused_attention) share.

An install gives a module INSTANCE a method of its own and records, under a key of its own in the module's `__dict__`, what the instance's
`__dict__` held under that name before: a callable, or None for "nothing: the class's method".  Uninstall puts back exactly that, so a
forward someone else had set on the instance survives a round trip as the same object and a module that had none has none again.  The
None convention is written here and nowhere else."""
from __future__ import annotations

import os
import types
from typing import Iterable, Optional

from torch import nn


def switched_off(env: str) -> bool:
    """QLLM_FUSE_*=0 in the environment: the install is a no-op that returns 0."""
    return os.environ.get(env, "1") == "0"


def class_names(default: Iterable[str], given: Optional[Iterable], intersect: bool) -> set:
    """The class names an install looks for.  `given` (classes or class names; None: not given) replaces the `default` list where the
    install verifies the module's structure itself (`intersect` False), and can only narrow it where the install restates the data flow
    of the classes it knows (`intersect` True)."""
    if given is None:
        return set(default)
    names = {t if isinstance(t, str) else t.__name__ for t in given}
    return names & set(default) if intersect else names


def replace(mod: nn.Module, fn, name: str = "forward"):
    """Give `mod` the instance method `name` = `fn` bound to it.  Returns what the instance's own `__dict__` had there, or None."""
    had = mod.__dict__.get(name)
    setattr(mod, name, types.MethodType(fn, mod))
    return had


def restore(mod: nn.Module, had, name: str = "forward") -> None:
    """Undo `replace`, given what it returned."""
    if had is None:
        mod.__dict__.pop(name, None)
    else:
        setattr(mod, name, had)


def original(mod: nn.Module, had, name: str = "forward"):
    """The method `mod` had before `replace`, given what it returned: the instance's, or the class's bound to it."""
    return had if had is not None else types.MethodType(getattr(type(mod), name), mod)
