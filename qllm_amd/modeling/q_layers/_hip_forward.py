"""Shared forward plumbing of the three q_layers: build (and cache) the C descriptor of the module's buffers,
call the fused HIP path, fall back to the library's dequant kernel + a plain GEMM only for configurations the fused
kernels do not cover (the reference's own branch (B), quant_linear_gptq.py:81-85).  Never computes on the CPU."""
from __future__ import annotations

import os

import torch

from ... import ops


def tensor_version(t) -> int:
    """`t._version`, or 0 for inference tensors (created under torch.inference_mode(): they do not track a version counter and
    reading it raises; they are also immutable outside inference mode, so identity alone is a sound key for them)."""
    return 0 if t.is_inference() else t._version


def _tkey(t):
    """Cache key of one buffer: storage address AND in-place version (load_state_dict / .copy_ bump `_version`)."""
    return (0, 0) if t is None else (t.data_ptr(), tensor_version(t))


def bit_family_entry(layout: int, dtype, rows: int):
    """Which of the bit family's own entries module code sends a call of `rows` rows to, under the current knobs: "bitpanel"
    (ops.linear_forward_bitpanel, csrc/bitpanel.hip: 17 .. ops.bitpanel_max_m() rows), "bitgemm" (ops.linear_forward_bitgemm,
    csrc/bitgemm.hip: from ops.bitgemm_min_m() rows -- 0: never -- and above ops.bitpanel_max_m()) or None.  Both read GPTQ / HQQ buffers in
    place and fp16 / bf16 activations; a descriptor with g_idx is not theirs (the callers ask with the row-sorted copy, or not at all).
    The ONE place this rule is written: `_hip_linear` asks it for plain layers, `QuantLinearGPTQ.forward` for act-order ones."""
    if layout not in (ops.LAYOUTS["GPTQ"], ops.LAYOUTS["HQQ"]) or dtype not in (torch.float16, torch.bfloat16):
        return None
    if 17 <= rows <= ops.bitpanel_max_m():
        return "bitpanel"
    if 0 < ops.bitgemm_min_m() <= rows and rows > ops.bitpanel_max_m():
        return "bitgemm"
    return None


def bitgroup_serves(bits: int, n_layers: int, act_order: bool, rows: int) -> bool:
    """Whether a sibling group's launch goes to ops.linear_forward_bitgroup (csrc/bitgemv_group.hip: 2 / 5 / 6 / 7 / 8 bits, up to four
    members, no act-order member, 1 .. ops.bitgroup_max_m() rows -- profiles/bitgemv_group.md) or to ops.linear_forward_grouped, the
    planner's entry, which refuses these widths (the layers then run on their own).  Asked by `SiblingGroup.forward_for` (fused.py)."""
    return bits in (2, 5, 6, 7, 8) and n_layers <= 4 and not act_order and 1 <= rows <= ops.bitgroup_max_m()


def _fused_tensors_ok(*tensors) -> bool:
    """What the fused residual entries ask of the tensors of one call: device tensors of one activation type, nothing to differentiate."""
    t0 = tensors[0]
    return (t0.dtype in (torch.float16, torch.bfloat16) and all(t.is_cuda and t.dtype == t0.dtype and t.device == t0.device for t in tensors)
            and not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors)))


# derived, pointer-holding state (ctypes descriptors, shadows, sibling groups): rebuilt on demand, never copied or pickled
_DERIVED = ("_desc", "_desc_key", "_desc_keep", "_native", "_native_key", "_ao", "_ao_key", "_ao_panel_refused", "_ao_gemm_refused", "_perm", "_swiglu_refused_from", "_residual_refused", "_swiglu_residual_refused", "_siblings")
# (a released module is materialised before it is pickled / deep-copied: see __getstate__)


class HipForwardMixin:
    _desc = None
    _desc_key = None
    _desc_keep = None
    _siblings = None  # SiblingGroup (fused.py) when the layer shares its input with q/k/v or gate/up siblings

    def __getstate__(self):
        # nn.Module pickles / deep-copies its __dict__: drop the caches that hold raw device pointers into THIS module's
        # buffers (a copy must build its own), like the reference's modules, which carry no such state.  nn.Module defines
        # __getstate__ itself and comes first in the q_layers' MRO, so each q_layer class re-exports this one explicitly.
        self.materialize_reference()
        state = torch.nn.Module.__getstate__(self)
        for k in _DERIVED:
            state.pop(k, None)
        return state

    def _invalidate(self):
        for k in _DERIVED[:-1]:
            self.__dict__.pop(k, None)

    def _layout_name(self) -> str:
        raise NotImplementedError

    def _f16(self, t):
        # bf16 modules: the kernels take fp16 scales/zeros/bias (the reference casts per call, ort_ops.cc:79-90);
        # cast once and cache alongside the descriptor.
        if t is None or t.dtype == torch.float16:
            return t
        return t.to(torch.float16)

    def _descriptor(self, act_order_g_idx, add_zero_bias: int):
        self.materialize_reference()
        qzeros = self.qzeros
        bias = self.bias
        key = (_tkey(self.qweight), _tkey(self.scales), _tkey(qzeros), _tkey(bias), _tkey(act_order_g_idx), add_zero_bias)
        if self._desc is None or key != self._desc_key:
            lay = self._layout_name()
            scales = self._f16(self.scales).contiguous()
            if lay == "HQQ":
                qzeros = self._f16(qzeros).contiguous()
            elif qzeros is not None:
                qzeros = qzeros.contiguous()
            g = act_order_g_idx
            if g is not None:
                g = g.to(device=self.qweight.device, dtype=torch.int32).contiguous()
            b = self._f16(bias).contiguous() if bias is not None else None
            self._desc, self._desc_keep = ops.make_weight(
                lay, self.qweight.contiguous(), scales, qzeros, g, b, self.infeatures, self.outfeatures,
                self.groupsize, self.bits, add_zero_bias)
            self._desc_key = key
        return self._desc

    # ---- the library's native (strip-major) layout of this layer --------------------------------------------------------
    _native = None
    _native_key = None
    # Memory policy.  The native copy holds exactly the information of qweight / qzeros / scales (pure permutations), so once it
    # exists the reference buffers are redundant on the device: with `release_reference` set they are replaced by empty
    # placeholders (the layer then costs 1.0x its packed bytes of HBM, not 2.0x) and regenerated bit-exactly on demand --
    # state_dict() / save_pretrained, load_state_dict, .to(), unpack(), or a call no native kernel serves.  The loader
    # (modeling/base.load_quantized) and bench.py switch it on; QLLM_RELEASE_REFERENCE=1 makes it the default for every module.
    release_reference = os.environ.get("QLLM_RELEASE_REFERENCE", "0") == "1"
    _released = None         # dict(name -> (shape, dtype)) of the buffers currently released, or None
    _needs_reference = False  # a call had to fall back to the reference buffers: never release this layer again
    _RELEASABLE = ("qweight", "qzeros", "scales")

    def native_descriptor(self, add_zero_bias: int = 0):
        """This layer in the library's strip-major native layout (include/qllm_mi355x.h): built once on the device from the
        module's own buffers by qllm_repack_native -- a pure integer permutation, the state dict is untouched -- and cached on the
        buffers' identity and version.  The kernels stream it 15-25 % faster at decode sizes than the reference layouts (every
        workgroup reads ONE contiguous region).  None when the layer cannot be held in that layout (bits not 3 / 4, odd shapes,
        act-order: see QuantLinearGPTQ) or QLLM_NATIVE_LAYOUT=0: callers then stream the reference buffers in place."""
        if os.environ.get("QLLM_NATIVE_LAYOUT", "1") == "0":
            self.materialize_reference()
            return None
        if self._released is None:
            key = (_tkey(self.qweight), _tkey(self.scales), _tkey(getattr(self, "qzeros", None)), _tkey(self.bias))
            if self._native_key != key:
                self._native, self._native_key = None, key
                src = self._native_source()
                if src is not None:
                    try:
                        self._native = ops.repack_native(*src)
                    except ops.QllmUnsupported:
                        self._native = None
            if self._native and self.release_reference and not self._needs_reference:
                self._release_reference()
        if not self._native:
            return None
        w = self._native[0]
        if w.add_zero_bias != add_zero_bias:  # (the AutoGPTQ offset is a field of the descriptor, not of the stored zero points)
            w = ops.QllmWeight(w.qweight, w.scales, w.qzeros, w.g_idx, w.bias, w.K, w.N, w.group_size, w.bits, w.layout, int(add_zero_bias))
        return w

    def _native_source(self):
        """(descriptor, keepalive) of the reference-layout buffers the native copy is made from; None = no native copy."""
        self._descriptor(None, 0)
        return self._desc, self._desc_keep

    def _release_reference(self):
        """Replace the buffers the native copy duplicates by empty placeholders (same dtype / device).  fp16 modules only: a bf16
        module's scales were rounded to fp16 for the kernels and could not be regenerated."""
        if self.scales.dtype != torch.float16 or (self._layout_name() == "HQQ" and self.qzeros.dtype != torch.float16):
            return
        rel = {}
        for name in self._RELEASABLE:
            t = getattr(self, name, None)
            if t is None or not t.is_cuda:
                return
            rel[name] = (tuple(t.shape), t.dtype)
        if not rel:   # nothing to release (QuantLinearORT keeps its blob): stay keyed on the buffers
            return
        self._desc = self._desc_key = self._desc_keep = None   # they point into the buffers that go away
        for name in rel:
            setattr(self, name, torch.empty(0, dtype=rel[name][1], device=self.qweight.device))
        self._released = rel

    def _regenerate_reference(self):
        """(qweight, scales, qzeros) of the reference layout, bit-exact, from the native copy."""
        return ops.unpack_native(self._native[0], self._native[1], self._layout_name())

    def materialize_reference(self):
        """Make qweight / qzeros / scales real again (no-op unless they are released).  Afterwards the native copy is still
        valid and keyed on the regenerated tensors; the next decode releases them again unless `_needs_reference` was set."""
        if self._released is None:
            return
        rel, self._released = self._released, None
        qweight, scales, qzeros = self._regenerate_reference()
        for name, t in (("qweight", qweight), ("scales", scales), ("qzeros", qzeros)):
            if name in rel and t is not None:
                setattr(self, name, t.reshape(rel[name][0]).to(rel[name][1]))
        self._native_key = (_tkey(self.qweight), _tkey(self.scales), _tkey(getattr(self, "qzeros", None)), _tkey(self.bias))

    # nn.Module comes first in the q_layers' MRO, so each q_layer class re-exports these three explicitly (like __getstate__)
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        self.materialize_reference()
        return torch.nn.Module._save_to_state_dict(self, destination, prefix, keep_vars)

    def _load_from_state_dict(self, *args, **kwargs):
        self.materialize_reference()   # the incoming tensors are copied INTO the buffers: they must have their shapes
        return torch.nn.Module._load_from_state_dict(self, *args, **kwargs)

    def _apply(self, fn, *args, **kwargs):
        self.materialize_reference()   # .to() / .cuda() / .half(): move real data, the derived copies are rebuilt where it lands
        return torch.nn.Module._apply(self, fn, *args, **kwargs)

    def decode_descriptor(self, act_order_g_idx=None, add_zero_bias: int = 0):
        """Descriptor the fused kernels should stream: the native copy when there is one, else the module's own buffers in place."""
        if act_order_g_idx is None:
            w = self.native_descriptor(add_zero_bias)
            if w is not None:
                return w
        return self._descriptor(act_order_g_idx, add_zero_bias)

    def forward_into(self, x: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
        """y = forward(x) written into the caller's contiguous [M, out_features] tensor `out` (no allocation; used by the
        tensor-parallel wrappers, whose shard kernels write straight into their slice of the gathered output).  Layers without a
        plain fused path for the call (act-order, unsupported shapes) compute normally and copy."""
        x2d = x.reshape(-1, x.shape[-1])
        resolve = getattr(self, "_resolve_act_order", None)   # (GPTQ detects act-order lazily: do it before branching on it)
        if resolve is not None:
            resolve()
        if getattr(self, "act_order", None) or not x2d.is_contiguous() or not out.is_contiguous():
            out.copy_(self(x).reshape(out.shape))
            return out
        azb = autogptq_compat() if self._layout_name() == "GPTQ" else 0
        try:
            ops.linear_forward(self.decode_descriptor(None, azb), x2d, out=out.view(x2d.shape[0], self.outfeatures))
        except ops.QllmUnsupported:
            out.copy_(self(x).reshape(out.shape))
        return out

    def forward_allreduce_into(self, x: torch.Tensor, out: torch.Tensor, reducer) -> bool:
        """Row-parallel shard at batch 1: y = sum over ranks of forward(x_rank), in ONE launch per rank (the batch-1 kernel pushes its
        partial outputs straight into the peers' staging buffers of `reducer`, a qllm_amd.comm.OneShotAllReduce; csrc/strip1_kernel.hpp,
        AR).  False when the call is not served (rows, layout, shape, act-order): the caller then runs forward_into + the collective."""
        x2d = x.reshape(-1, x.shape[-1])
        resolve = getattr(self, "_resolve_act_order", None)
        if resolve is not None:
            resolve()
        if (x2d.shape[0] != 1 or getattr(self, "act_order", None) or not x2d.is_contiguous() or not out.is_contiguous()
                or not hasattr(reducer, "linear_all_reduce")):
            return False
        azb = autogptq_compat() if self._layout_name() == "GPTQ" else 0
        w = self.native_descriptor(azb)
        return w is not None and reducer.linear_all_reduce(w, x2d, out.view(1, self.outfeatures))

    # smallest row count the fused SwiGLU entry refused for this layer (what it serves is monotone in the row count: 1, or up to 4 rows)
    _swiglu_refused_from = 1 << 30
    # the most rows forward_swiglu sends to the fused entry: measured (profiles/swiglu.md), the fused MLP wins at one row and loses at
    # four (the prologue computes silu for every batch row in every block) -- the entry itself serves up to four; QLLM_FUSE_MLP_MAX_M moves it
    swiglu_max_m = int(os.environ.get("QLLM_FUSE_MLP_MAX_M", "1"))

    def forward_swiglu(self, gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
        """forward(silu(gate) * up) -- the down_proj of a SwiGLU MLP.  Where the batch-1 kernel serves the call on the layer's native
        copy, ONE launch forms the product while it stages its input (ops.linear_forward_swiglu, csrc/strip1_swiglu.hip); everything
        else -- more rows than `swiglu_max_m`, a refusal (remembered as "nothing from this many rows up", so a refused shape costs one
        call once), no native copy, an act-order layer, non-contiguous inputs, dtypes or shapes that disagree -- is the elementwise kernel and the layer's own forward."""
        g2d = gate.reshape(-1, gate.shape[-1])
        u2d = up.reshape(-1, up.shape[-1])
        m = g2d.shape[0]
        resolve = getattr(self, "_resolve_act_order", None)   # (GPTQ detects act-order lazily: do it before branching on it)
        if resolve is not None:
            resolve()
        if (1 <= m <= self.swiglu_max_m and m < self._swiglu_refused_from and gate.shape == up.shape and gate.dtype == up.dtype
                and gate.dtype in (torch.float16, torch.bfloat16) and g2d.is_contiguous() and u2d.is_contiguous()
                and not getattr(self, "act_order", None)):
            azb = autogptq_compat() if self._layout_name() == "GPTQ" else 0
            w = self.native_descriptor(azb)
            if w is not None:
                try:
                    return ops.linear_forward_swiglu(w, g2d, u2d).reshape(gate.shape[:-1] + (self.outfeatures,))
                except ops.QllmUnsupported:
                    self._swiglu_refused_from = m
        return self(torch.nn.functional.silu(gate) * up)

    # the fused residual entries refused this layer once (they serve one row of it or nothing): not asked again until `_invalidate()`
    _residual_refused = False
    _swiglu_residual_refused = False
    # the most rows forward_residual / forward_swiglu_residual send to the fused entry (it serves one); 0: never.  Measured:
    # profiles/residual.md; QLLM_FUSE_RESIDUAL_MAX_M moves it
    residual_max_m = int(os.environ.get("QLLM_FUSE_RESIDUAL_MAX_M", "1"))

    def _residual_descriptor(self, inputs, residual: torch.Tensor, refused: bool):
        """The native descriptor for a fused residual call on `inputs` ([..., K] each) and `residual` ([..., N]), or None: the call is not
        one the modules send to the entry -- more rows than `residual_max_m`, a remembered refusal, shapes / dtypes that disagree,
        non-contiguous tensors, CPU tensors, grad mode, an act-order layer, no native copy."""
        x = inputs[0]
        m = x.numel() // x.shape[-1] if x.shape[-1] else 0
        resolve = getattr(self, "_resolve_act_order", None)   # (GPTQ detects act-order lazily: do it before branching on it)
        if resolve is not None:
            resolve()
        if (refused or not 1 <= m <= self.residual_max_m or any(t.shape != x.shape for t in inputs)
                or residual.shape != x.shape[:-1] + (self.outfeatures,) or not _fused_tensors_ok(*inputs, residual)
                or not all(t.reshape(-1, t.shape[-1]).is_contiguous() for t in (*inputs, residual)) or getattr(self, "act_order", None)):
            return None
        return self.native_descriptor(autogptq_compat() if self._layout_name() == "GPTQ" else 0)

    def forward_residual(self, x: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        """residual + forward(x) -- the o_proj (or down_proj) of a decoder layer with its residual add.  Where the batch-1 kernel serves
        the call on the layer's native copy, ONE launch adds the residual as it stores its output (ops.linear_forward_residual,
        csrc/strip1_resid.hip), bit for bit the eager add; everything else (`_residual_descriptor`; a refusal is remembered) is the
        layer's own forward and the elementwise add.  Never writes into `residual`."""
        w = self._residual_descriptor((x,), residual, self._residual_refused)
        if w is not None:
            try:
                return ops.linear_forward_residual(w, x.reshape(-1, x.shape[-1]), residual.reshape(-1, self.outfeatures)).reshape(residual.shape)
            except ops.QllmUnsupported:
                self._residual_refused = True
        return residual + self(x)

    def forward_swiglu_residual(self, gate: torch.Tensor, up: torch.Tensor, residual: torch.Tensor) -> torch.Tensor:
        """residual + forward_swiglu(gate, up) -- the down_proj of a SwiGLU MLP with neither elementwise kernel around it
        (ops.linear_forward_swiglu_residual, csrc/strip1_swiglu_resid.hip), under the rules of `forward_residual`; everything else is
        `forward_swiglu` and the elementwise add."""
        w = self._residual_descriptor((gate, up), residual, self._swiglu_residual_refused) if gate.shape == up.shape else None
        if w is not None:
            try:
                return ops.linear_forward_swiglu_residual(w, gate.reshape(-1, gate.shape[-1]), up.reshape(-1, up.shape[-1]),
                                                          residual.reshape(-1, self.outfeatures)).reshape(residual.shape)
            except ops.QllmUnsupported:
                self._swiglu_residual_refused = True
        return residual + self.forward_swiglu(gate, up)

    def _hip_linear(self, x: torch.Tensor, act_order_g_idx=None, add_zero_bias: int = 0) -> torch.Tensor:
        if not x.is_cuda or not self.qweight.is_cuda:
            raise RuntimeError(
                f"{type(self).__name__}.forward needs HIP tensors on an MI355X: qllm_amd ships no CPU / eager fallback "
                f"(x on {x.device}, qweight on {self.qweight.device})")
        if self._siblings is not None and act_order_g_idx is None:
            y = self._siblings.forward_for(self, x, add_zero_bias)  # q/k/v, gate/up: one grouped launch for the group (fused.py)
            if y is not None:
                return y
        x2d = x.reshape(-1, x.shape[-1])
        if not x2d.is_contiguous():
            x2d = x2d.contiguous()
        w = self.decode_descriptor(act_order_g_idx, add_zero_bias)
        try:
            try:
                # (bf16 prefill: x is converted to fp16 ONCE per distinct tensor -- siblings share it -- instead of once per call)
                y = ops.linear_forward_shared(w, x2d, key=x) if act_order_g_idx is None else ops.linear_forward(w, x2d)
            except ops.QllmUnsupported:
                if w.layout not in (ops.LAYOUTS["NATIVE"], ops.LAYOUTS["NATIVE_F16Z"]):
                    raise
                # a shape the native layout is not served at (e.g. M > 64 with N % 64 != 0, or 3 bits with N % 128 != 0; since
                # round 7 N % 128 == 64 -- Falcon-7B -- is served): the reference buffers in place, and they stay on the device from now on
                self._needs_reference = True
                w = self._descriptor(act_order_g_idx, add_zero_bias)
                y = ops.linear_forward(w, x2d)
        except ops.QllmUnsupported:
            # 2/5/6/7/8-bit layers (and in-place 3/4-bit ones of ragged width) at 17 .. QLLM_BITPANEL_MAX_M rows: the fused mid-batch
            # kernel (bias included); the same layers above those rows, from QLLM_BITGEMM_MIN_M on: the fused 2..8-bit prefill kernel
            y = self._bit_family_linear(w, x2d, act_order_g_idx, key=x)
            if y is None:
                # e.g. 3/5/6/7/8-bit at prefill sizes: dequantise with the library kernel, then a plain library GEMM
                wt = ops.dequant(w, x.device, torch.float16)
                y = torch.matmul(x2d, wt.to(x2d.dtype))
                if self.bias is not None:
                    y = y + self.bias.to(y.dtype)
        return y.reshape(x.shape[:-1] + (self.outfeatures,))

    @staticmethod
    def _bit_family_linear(w, x2d, act_order_g_idx=None, key=None):
        """The bit family's entry for a call no planner route serves (`bit_family_entry`: the mid-batch kernel, above its rows the
        2..8-bit prefill kernel), or None: act-order descriptors, other layouts, other row counts, other activation types and the
        kernel's own refusal all leave the call to dequant + GEMM.  `key`: see ops.linear_forward_bitgemm."""
        entry = None if act_order_g_idx is not None else bit_family_entry(w.layout, x2d.dtype, x2d.shape[0])
        try:
            if entry == "bitpanel":
                return ops.linear_forward_bitpanel(w, x2d)
            if entry == "bitgemm":
                return ops.linear_forward_bitgemm(w, x2d, key=key)
        except ops.QllmUnsupported:
            pass
        return None


def export_module_hooks(cls):
    """Class decorator for the q_layers: nn.Module precedes HipForwardMixin in their MRO, so the mixin's overrides of nn.Module
    methods have to be re-exported on the class itself."""
    for name in ("__getstate__", "_save_to_state_dict", "_load_from_state_dict", "_apply"):
        setattr(cls, name, getattr(HipForwardMixin, name))
    return cls


def autogptq_compat() -> int:
    return int(os.environ.get("COMPATIBLE_WITH_AUTOGPTQ", "0"))
