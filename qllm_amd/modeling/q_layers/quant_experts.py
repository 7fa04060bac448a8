"""The experts of a sparse mixture-of-experts block (Mixtral's `block_sparse_moe.experts`, Qwen3-MoE's `mlp.experts`) over quantized
per-expert layers, with the family module's call: forward(hidden_states [T, H], top_k_index [T, top_k], top_k_weights [T, top_k]).

transformers (5.x) keeps a family's experts as two 3-D parameters, so a quantized checkpoint's `experts.<e>.<proj>.qweight` tensors had
nowhere to go.  `QuantExperts` holds one q_layer per expert and projection under the names the checkpoints use -- Mixtral
`experts.<e>.w1 / w3 / w2` (gate, up, down), Qwen3-MoE `experts.<e>.gate_proj / up_proj / down_proj` -- so load_state_dict fills them
and state_dict writes them back (a Mixtral under transformers' `mlp`, not the checkpoint's `block_sparse_moe`).

Three routes.  Where `ops.moe_plan` serves the call -- 1..4 tokens, 4-bit layers with 128-wide groups, packed or symmetric zero points,
native copies -- the block is TWO launches (ops.moe_gate_up, ops.moe_down; csrc/moe_decode.hip) that read the expert ids on the device:
nothing goes back to the host, so a decode step captures into a graph.  For that the native copies of each projection are stacked per
expert in one allocation, made once; every layer's native buffers become views of its slice (`_hip_forward.py`'s native-copy policy: the
layer regenerates its reference buffers from them, and `release_reference` keeps working), so nothing is stored twice.  Everything else
-- more tokens (unless `fuse_moe_prefill` is on: then ops.moe_route / moe_prefill_gate_up / moe_prefill_down, csrc/moe_prefill.hip, serve
the same layers for any number of tokens as four launches, equally captured), other bit widths or group sizes, HQQ's fp16 zero points, act-order layers, a CPU device, grad mode, QLLM_FUSE_MOE=0 -- is
the family's own loop restated over the per-expert q_layers (one_hot, nonzero, per hit expert three layer calls, index_add_)."""
from __future__ import annotations

import os

import torch
from torch import nn

from ... import ops
from ._hip_forward import _act_tensors_ok

SPARSE_BLOCKS = {  # class name of the sparse block -> the experts' projection names (gate, up, down)
    "MixtralSparseMoeBlock": ("w1", "w3", "w2"),
    "Qwen3MoeSparseMoeBlock": ("gate_proj", "up_proj", "down_proj"),
}


class QuantExperts(nn.ModuleList):
    """One nn.Module per expert ("<e>"), each holding its three q_layers under `names`."""

    def __init__(self, names, layers, act_fn):
        super().__init__()
        self.names = tuple(names)
        for trio in layers:
            expert = nn.Module()
            for name, layer in zip(self.names, trio):
                expert.add_module(name, layer)
            self.append(expert)
        self.num_experts = len(layers)
        self.__dict__["act_fn"] = act_fn   # (not a child: the list's children are the experts, and the state dict holds only their buffers)
        self._stacks = None   # ((qweight, scales, qzeros) x gate, up, down, add_zero_bias), False (not stackable) or None (not built)
        self._installed, self._refused, self._revalidate = None, set(), False   # the slices given to the layers; refused forms
        self.fuse_moe_prefill = False   # opt-in (install_quant_experts): more than ops.MOE_MAX_TOKENS tokens as the routed launches

    @classmethod
    def from_experts(cls, experts, names, make_layer):
        """In the place of the family's `experts` (its sizes and its activation): `make_layer(in_features, out_features, expert,
        name)` builds each q_layer."""
        h, i = experts.hidden_dim, experts.intermediate_dim
        layers = [[make_layer(h, i, e, names[0]), make_layer(h, i, e, names[1]), make_layer(i, h, e, names[2])] for e in range(experts.num_experts)]
        return cls(names, layers, experts.act_fn)

    def trio(self, e: int):
        expert = self[e]
        return tuple(getattr(expert, n) for n in self.names)

    # the stacks point into the layers' buffers: whatever moves or reloads those drops them (the layers' own hooks rebuild their copies)
    def _apply(self, fn, *args, **kwargs):
        self._stacks = None
        return super()._apply(fn, *args, **kwargs)

    def _load_from_state_dict(self, *args, **kwargs):
        self._stacks = None
        return super()._load_from_state_dict(*args, **kwargs)

    def _save_to_state_dict(self, *args, **kwargs):
        self._revalidate = True    # (the layers are about to materialise their reference buffers: `_check_stacks` releases them again)
        return super()._save_to_state_dict(*args, **kwargs)

    def __getstate__(self):
        state = super().__getstate__()
        state.update(_stacks=None, _installed=None, _refused=set(), _revalidate=False)
        return state

    def _build_stacks(self):
        """The three stacks, or False: every layer 4 bits, 128-wide groups, no act-order, no bias, with a native copy of packed or no zero
        points.  Each layer's native buffers are copied into its slice once and replaced by views of it."""
        layers = [self.trio(e) for e in range(self.num_experts)]
        azb = {l._add_zero_bias() for t in layers for l in t}
        if len(azb) != 1 or (self.act_fn is not nn.functional.silu and type(self.act_fn).__name__ not in ("SiLU", "SiLUActivation")):
            return False   # (the kernels compute SiLU)
        azb = azb.pop()
        natives = []
        for trio in layers:
            for l in trio:
                if l.bits != 4 or l.groupsize != 128 or l.bias is not None or l._act_order_resolved():
                    return False
                w = l.native_descriptor(azb)
                if w is None or w.layout != ops.LAYOUTS["NATIVE"]:
                    return False
            natives.append([l._native for l in trio])
        stacks = []
        for kind in range(3):
            keeps = [n[kind][1] for n in natives]       # (nq, ns, nz, None, bias) per expert
            if len({k[2] is None for k in keeps}) != 1:
                return False
            w0 = natives[0][kind][0]
            shapes = ((w0.N // 16, w0.K // 8, 16), (w0.N // 16, w0.K // 128, 16), (w0.N // 16, w0.K // 128, 2))
            parts = []
            for j, shape in enumerate(shapes):
                if keeps[0][j] is None:
                    parts.append(None)
                    continue
                stack = torch.empty((self.num_experts,) + shape, dtype=keeps[0][j].dtype, device=keeps[0][j].device)
                for e, k in enumerate(keeps):
                    if k[j].numel() != stack[e].numel():
                        return False
                    stack[e].view(-1).copy_(k[j].view(-1))
                parts.append(stack)
            stacks.append(tuple(parts))
            for e, trio in enumerate(layers):           # the layer's native copy becomes its slice of the stack
                w, keep = natives[e][kind]
                views = tuple(p[e].view(-1) if p is not None else None for p in parts)
                nw = ops.QllmWeight(views[0].data_ptr(), views[1].data_ptr(), views[2].data_ptr() if views[2] is not None else None, None, None,
                                    w.K, w.N, w.group_size, w.bits, w.layout, w.add_zero_bias)
                trio[kind]._native = (nw, views + (None, None))
        self._installed, self._refused = [l._native for trio in layers for l in trio], set()
        return tuple(stacks) + (azb,)

    def _fused_plan(self, hidden_states, top_k_index, top_k_weights):
        """(plan, stacks) where fused launches serve this call -- 1..4 tokens: the decode pair (`ops.moe_plan`, 5 sizes); more, with
        `fuse_moe_prefill` on: the routed launches (`ops.moe_prefill_plan`, 6 sizes, for the first chunk of rows) -- else None."""
        many = hidden_states.dim() == 2 and hidden_states.shape[0] > ops.MOE_MAX_TOKENS
        if (os.environ.get("QLLM_FUSE_MOE", "1") == "0" or hidden_states.dim() != 2 or hidden_states.shape[0] < 1
                or (many and (not self.fuse_moe_prefill or os.environ.get("QLLM_FUSE_MOE_PREFILL", "1") == "0"))
                or not _act_tensors_ok(hidden_states) or not top_k_index.is_cuda or not top_k_weights.is_cuda
                or (torch.is_grad_enabled() and top_k_weights.requires_grad)):
            return None
        if os.environ.get("QLLM_NATIVE_LAYOUT", "1") == "0":      # (the layers hold no native copies then: nothing to stack, nothing cached)
            return None
        if self._stacks and (self._revalidate or self.trio(0)[0]._native is not self._installed[0]):
            self._check_stacks()
        if self._stacks is None:
            self._stacks = self._build_stacks()
        key = (hidden_states.shape, top_k_index.shape, hidden_states.dtype, top_k_weights.dtype)
        if not self._stacks or key in self._refused:
            return None
        try:
            if many:
                rows = self._chunk_rows(top_k_index)
                return ops.moe_prefill_plan(hidden_states[:rows], top_k_index[:rows], top_k_weights[:rows], *self._stacks[:3]), self._stacks
            return ops.moe_plan(hidden_states, top_k_index, top_k_weights, *self._stacks[:3]), self._stacks
        except ops.QllmUnsupported:
            self._refused.add(key)   # (a form is refused for its sizes and types: not asked again, the loop runs on every step of it)
            return None

    @staticmethod
    def _chunk_rows(top_k_index):
        return max(1, ops.MOE_PREFILL_MAX_SLOTS // max(1, top_k_index.shape[-1]))   # rows of one routed call

    def _check_stacks(self):
        """After a state_dict() (the layers materialised their reference buffers) and whenever the first layer's native copy is no longer
        the slice put there: ask every layer for its native copy again -- that re-releases the reference buffers under `release_reference`
        and rebuilds a copy whose buffers changed -- and drop the stacks if any layer's copy is not its slice any more.  An in-place
        edit of the buffers of a layer other than the first is seen only at the next state_dict / load_state_dict / .to()."""
        self._revalidate = False
        azb = self._stacks[3]
        layers = [l for e in range(self.num_experts) for l in self.trio(e)]
        if any(l.native_descriptor(azb) is None or l._native is not n for l, n in zip(layers, self._installed)):
            self._stacks = None

    def forward(self, hidden_states: torch.Tensor, top_k_index: torch.Tensor, top_k_weights: torch.Tensor) -> torch.Tensor:
        x = hidden_states if hidden_states.is_contiguous() else hidden_states.contiguous()
        ids = top_k_index if top_k_index.is_contiguous() else top_k_index.contiguous()
        wts = top_k_weights if top_k_weights.is_contiguous() else top_k_weights.contiguous()
        served = self._fused_plan(x, ids, wts)
        if served is None:
            return self.forward_loop(hidden_states, top_k_index, top_k_weights)
        plan, (gate, up, down, azb) = served
        if len(plan) == 6:      # the routed launches; rows are independent, so calls of more slots than one call serves go in row chunks
            out, rows = torch.empty_like(x), self._chunk_rows(ids)
            for r in range(0, x.shape[0], rows):
                xs, ic, wc = x[r:r + rows], ids[r:r + rows], wts[r:r + rows]
                nbytes = ops.moe_prefill_workspace_bytes(xs.shape[0], ic.shape[1], self.num_experts, xs.shape[1], gate[0].shape[1] * 16)
                route = ops.moe_route(ic, self.num_experts, workspace=torch.empty(nbytes, dtype=torch.uint8, device=x.device))
                h = ops.moe_prefill_gate_up(xs, ic, route, gate, up, add_zero_bias=azb)
                ops.moe_prefill_down(h, ic, wc, route, down, add_zero_bias=azb, out=out[r:r + rows])
            return out
        h = ops.moe_gate_up(x, ids, gate, up, add_zero_bias=azb)
        return ops.moe_down(h, ids, wts, down, add_zero_bias=azb)

    def forward_loop(self, hidden_states, top_k_index, top_k_weights):
        """The family's loop over the hit experts (transformers' MixtralExperts.forward), each projection a q_layer call."""
        final = torch.zeros_like(hidden_states)
        with torch.no_grad():
            mask = torch.nn.functional.one_hot(top_k_index, num_classes=self.num_experts + 1).permute(2, 1, 0)
            hit = torch.greater(mask.sum(dim=(-1, -2)), 0).nonzero()
        for idx in hit:
            e = int(idx[0])
            if e == self.num_experts:     # the masked-expert sentinel
                continue
            gate_l, up_l, down_l = self.trio(e)
            top_k_pos, token_idx = torch.where(mask[e])
            cur = hidden_states[token_idx]
            cur = down_l(self.act_fn(gate_l(cur)) * up_l(cur))
            cur = cur * top_k_weights[token_idx, top_k_pos, None]
            final.index_add_(0, token_idx, cur.to(final.dtype))
        return final


def install_quant_experts(model: nn.Module, keys, make_layer, fuse_moe_prefill: bool = False) -> int:
    """Put a `QuantExperts` in the place of the experts of every sparse block of `model` (`SPARSE_BLOCKS`) whose per-expert `.qweight`
    tensors `keys` names; the router (`gate`) stays the family's.  `make_layer(in_features, out_features, name)` builds the q_layer of
    the module called `name`.  `fuse_moe_prefill`: the modules' opt-in of the same name.  Returns how many blocks were given one."""
    n = 0
    for name, block in list(model.named_modules()):
        names = SPARSE_BLOCKS.get(type(block).__name__)
        experts = getattr(block, "experts", None)
        if names is None or experts is None or isinstance(experts, QuantExperts) or f"{name}.experts.0.{names[0]}.qweight" not in keys:
            continue
        prefix = f"{name}.experts"
        block.experts = QuantExperts.from_experts(experts, names, lambda k, o, e, proj: make_layer(k, o, f"{prefix}.{e}.{proj}"))
        block.experts.fuse_moe_prefill = bool(fuse_moe_prefill)
        n += 1
    return n
