"""GPTQ quantization on the device: fp16 model + calibration token ids in -> QuantLinearGPTQ layers out.

The reference's path is GPTQQuant.do_quantize (qllm/quantization/gptq/quant_gptq.py:89-157, default non-true_sequential form) over
GPTQ.add_batch / GPTQ.fasterquant (gptq.py:75-102, 129-258) followed by QuantLinearGPTQ.pack.  Here the Hessian, its factorisation and the
packing are torch / library plumbing, and the column walk -- the reference's six tiny launches per column -- is ONE library call per layer
(qllm_gptq_quantize, csrc/gptq_quant.hip).  There is no CPU quantizer.

static_groups=True (gptq.py:157-165, 207-211, 230-233) is a second library call (qllm_gptq_quantize_static, csrc/gptq_static.hip): every
group's scale / zero is fixed from the original weights before the walk, the columns are still walked in act-order, and the layer keeps
the trivial g_idx -- act-order's accuracy in a checkpoint whose layers take the plain decode route (no column gather, no second weight
copy, grouped launches like any plain layer).

Out of scope (the reference's other switches): mse, the allow_mix_bits search, true_sequential, Conv layers.  The AWQ quantizer is
awq.py."""
from __future__ import annotations

import math
import warnings
from typing import Dict, Optional

import torch

from .. import ops
from ._common import bits_for, capture_first_block_inputs, decoder_blocks, first, layer_dtype, need_device


def accumulate_hessian(H: Optional[torch.Tensor], nsamples: int, x: torch.Tensor):
    """GPTQ.add_batch (gptq.py:75-102): the running mean H = 2/n sum X^T X over calibration batches, in H's dtype (fp32 when H is None).
    x: [tokens, K] (one batch) or [batch, tokens, K].  Returns (H, nsamples)."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    batch = x.shape[0]
    x = x.reshape(-1, x.shape[-1])
    if H is None:
        H = torch.zeros((x.shape[1], x.shape[1]), dtype=torch.float32, device=x.device)
    H *= nsamples / (nsamples + batch)
    nsamples += batch
    xs = math.sqrt(2 / nsamples) * x.to(H.dtype)
    H += xs.t().matmul(xs)
    return H, nsamples


def _factor(H: torch.Tensor):
    """(the upper Cholesky factor of H^-1 (gptq.py:179-181), "device" or "host").  The host is used only where this build of torch has
    no device Cholesky, and a warning says so; every other error of the device run (not positive-definite, out of memory, a HIP error)
    is the caller's."""
    def run(h):
        return torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(h)), upper=True)
    try:
        return run(H).contiguous(), "device"
    except RuntimeError as e:
        msg = str(e).lower()
        missing = isinstance(e, NotImplementedError) or any(t in msg for t in ("not implemented", "not compiled", "requires compiling",
                                                                               "without magma", "no lapack"))
        if not missing:
            raise
        warnings.warn(f"torch has no device Cholesky here ({e}): factorising the [{H.shape[0]}, {H.shape[0]}] Hessian on the host")
    return run(H.cpu()).to(H.device).contiguous(), "host"


def _pack(codes_kn: torch.Tensor, zeros_gn: torch.Tensor, bits: int, group_size: int, layer=None):
    """codes [K, N] and integer zero points [K/g, N] on the device -> (qweight, qzeros) on the device, through QuantLinearGPTQ's own
    pack path (compress_weight.py: pack_on_device / pack_qzeros, the COMPATIBLE_WITH_AUTOGPTQ offset included)."""
    from ..modeling.q_layers import QuantLinearGPTQ
    k, n = codes_kn.shape
    if k % 32 or n % 32:
        raise ValueError(f"QuantLinearGPTQ packs whole 32-value words along K and (for the zero points) along N: K={k} N={n}")
    if layer is None:
        layer = QuantLinearGPTQ(bits, group_size, k, n, False)
    layer.pack_on_device(codes_kn, zeros_gn)
    return layer.qweight.to(codes_kn.device), layer.qzeros.to(codes_kn.device)


def _solve(weight, H, bits, g, act_order, sym, damp_percent, debug, static_groups=False):
    """gptq_quantize_weight before packing: (codes i32 [K, N], scale / zero f32 [N, K/g], wq [N, K], all in the original column order,
    g_idx i32 [K], the summed loss, the debug extras or None).  static_groups: the solver gets w in the original order next to perm
    and returns everything in the original order itself."""
    need_device(weight, "gptq_quantize_weight")
    if weight.dim() != 2:
        raise RuntimeError(f"weight must be [out_features, in_features], got {tuple(weight.shape)}")
    n, k = weight.shape
    dev = weight.device
    w = weight.detach().clone()
    perm = u = hd = where = None
    if H is not None:
        if tuple(H.shape) != (k, k):
            raise RuntimeError(f"H must be [{k}, {k}], got {tuple(H.shape)}")
        h = H.to(device=dev, dtype=torch.float32).clone()
        dead = torch.diag(h) == 0
        idx = torch.arange(k, device=dev)
        h[idx[dead], idx[dead]] = 1
        w[:, dead] = 0
        if act_order:
            perm = torch.argsort(torch.diag(h), descending=True)
            if not static_groups:
                w = w[:, perm]
            h = h[perm][:, perm]
        h[idx, idx] += damp_percent * torch.mean(torch.diag(h))
        hd = h.clone() if debug else None
        u, where = _factor(h)
        del h
    w = w.contiguous()
    if static_groups:
        codes, scale, zero, wq, loss_n = ops.gptq_quantize_static(w, u, perm, bits, g, sym, check_perm=False)   # (an argsort)
    else:
        codes, scale, zero, wq, loss_n = ops.gptq_quantize(w, u, bits, g, sym)
    extras = None
    if debug:
        extras = dict(U=u, factorization=where)
        if hd is not None:
            wq_rtn = ops.gptq_quantize(w, None, bits, g, sym)[3]
            for key, q in (("rtn_loss", wq_rtn), ("loss_hd", wq)):
                d = w.float() - q.float()
                if static_groups and perm is not None:
                    d = d[:, perm]      # hd is in processing order
                extras[key] = 0.5 * (d.matmul(hd) * d).sum()
    if perm is not None and not static_groups:
        inv = torch.argsort(perm)
        codes, wq = codes[inv].contiguous(), wq[:, inv].contiguous()
        g_idx = (torch.arange(k, device=dev) // g)[inv].to(torch.int32)
    else:
        g_idx = (torch.arange(k, device=dev) // g).to(torch.int32)
    if debug:
        extras.update(codes=codes.t().contiguous().to(torch.uint8), scale=scale, zero=zero, wq=wq,
                      perm=perm if perm is not None else torch.arange(k, device=dev))
    return codes, scale, zero, wq, g_idx, loss_n.sum(), extras


def gptq_quantize_weight(weight: torch.Tensor, H: Optional[torch.Tensor], bits: int, group_size: int = 128, act_order: bool = False,
                         sym: bool = False, damp_percent: float = 0.01, debug: bool = False, pack: bool = True,
                         static_groups: bool = False):
    """weight [N, K] (fp16 / bf16 / fp32 on a HIP device) and its input Hessian H [K, K] (accumulate_hessian; None: round-to-nearest)
    -> (qweight i32 [K*bits/32, N], qzeros i32 [K/g, N*bits/32], scales [K/g, N] in weight's dtype (fp16 for fp32 weights), g_idx i32 [K],
    loss): QuantLinearGPTQ's buffers and the reference's summed loss (a 0-d device tensor).  GPTQ.fasterquant's order: dead columns
    (diag(H) == 0: H = 1, W = 0), act-order permutation by descending diag(H), damping by damp_percent x mean(diag(H)), cholesky ->
    cholesky_inverse -> upper cholesky, the column solver, un-permutation, packing.  `debug` appends a dict: codes u8 [N, K] / scale /
    zero f32 [N, K/g] / wq [N, K] in the original column order, perm, U, factorization ("device" / "host"), and rtn_loss / loss_hd =
    1/2 tr(D Hd D^T) of round-to-nearest and of the result on the damped Hessian Hd (a second solver call and two [N,K]x[K,K] products:
    only with debug).  pack=False leaves qweight / qzeros None (layers QuantLinearGPTQ cannot hold).  static_groups: every group's scale /
    zero from the original weights, before the walk (the reference's static_groups=True): g_idx is arange(K) // group_size also with
    act_order, which then only orders the walk."""
    g = weight.shape[-1] if group_size == -1 else int(group_size)
    codes, scale, zero, _, g_idx, loss, extras = _solve(weight, H, bits, g, act_order, sym, damp_percent, debug, static_groups)
    sdtype = layer_dtype(weight)
    qweight, qzeros = _pack(codes, zero.t().contiguous(), bits, g) if pack else (None, None)
    ret = (qweight, qzeros, scale.t().contiguous().to(sdtype), g_idx, loss)
    return ret + (extras,) if debug else ret


def quantize_linear(linear: torch.nn.Linear, H: Optional[torch.Tensor], bits: int, group_size: int = 128, act_order: bool = False,
                    sym: bool = False, damp_percent: float = 0.01, device=None, debug: bool = False, static_groups: bool = False):
    """nn.Linear + its input Hessian -> QuantLinearGPTQ on the device, bias carried over.  linear.weight is replaced by the dequantized
    weights (gptq.py:243: what follows the layer sees the quantization error).  The layer carries `gptq_loss` (and, with debug,
    `gptq_rtn_loss` / `gptq_loss_hd`, see gptq_quantize_weight)."""
    from ..modeling.q_layers import QuantLinearGPTQ
    w = linear.weight.data
    dev = torch.device(device) if device is not None else (w.device if w.is_cuda else torch.device("cuda:0"))
    n, k = w.shape
    g = k if group_size == -1 else int(group_size)
    codes, scale, zero, wq, g_idx, loss, extras = _solve(w.to(dev), H, bits, g, act_order, sym, damp_percent, debug, static_groups)
    dtype = layer_dtype(w)
    layer = QuantLinearGPTQ(bits, g, k, n, linear.bias is not None, dtype=dtype)
    layer.qweight, layer.qzeros = _pack(codes, zero.t().contiguous(), bits, g, layer)
    layer.scales, layer.g_idx = scale.t().contiguous().to(dtype), g_idx
    if linear.bias is not None:
        layer.bias = linear.bias.data.to(device=dev, dtype=dtype)
    layer = layer.to(dev)
    layer.gptq_loss = float(loss)
    if debug and "rtn_loss" in extras:
        layer.gptq_rtn_loss, layer.gptq_loss_hd = float(extras["rtn_loss"]), float(extras["loss_hd"])
    linear.weight.data = wq.to(device=w.device, dtype=w.dtype)
    return layer


def quantize_model(model, calibration_input_ids, bits: int, group_size: int = 128, act_order: bool = False, sym: bool = False,
                   bits_by_layer: Optional[Dict[str, int]] = None, device="cuda:0", damp_percent: float = 0.01, debug: bool = False,
                   static_groups: bool = False):
    """Every nn.Linear inside the decoder blocks -> QuantLinearGPTQ, GPTQQuant.do_quantize's default form: the first block's inputs
    and keyword arguments are captured from a forward over `calibration_input_ids` ([rows, tokens] token ids, one calibration batch per
    row); then, block by block: every linear's input Hessian is accumulated by forward hooks over the calibration batches, each linear
    is quantized, and the block is run again ON its quantized layers to produce the next block's inputs.  Only one block's fp16
    weights are resident next to the quantized model.  `bits_by_layer` maps a module kind ("q_proj") or a full module name to its
    width.  `static_groups` (see gptq_quantize_weight) leaves every layer with the trivial g_idx; the saved desc_act still follows
    act_order, as in the reference.  lm_head and the embeddings stay as they are.  The model is left on `device` with `quant_config`
    (version GPTQ, desc_act, sym, static_groups, per-layer widths) for modeling.base.save_quantized / load_quantized, sibling groups installed, and `gptq_losses`
    {module name: loss} (with debug also `gptq_rtn_losses` and `gptq_losses_hd`)."""
    from ..modeling import base
    from ..modeling.q_layers import QuantLinearGPTQ, install_sibling_groups
    from ..utils import modelutils
    dev = torch.device(device)
    bits_by_layer = dict(bits_by_layer or {})
    prefix, blocks = decoder_blocks(model)
    cfg = base.QuantConfig(bits=bits, group_size=group_size, version="GPTQ", quant_method="gptq", desc_act=bool(act_order), sym=bool(sym),
                           static_groups=bool(static_groups))
    ids = torch.as_tensor(calibration_input_ids)
    if ids.dim() == 1:
        ids = ids.unsqueeze(0)
    losses, rtn_losses, losses_hd = {}, {}, {}
    with torch.no_grad():
        inps, args, kwargs = capture_first_block_inputs(model, blocks, ids, dev)
        for i in range(len(blocks)):
            block = blocks[i].to(dev)
            linears = modelutils.find_layers(block, [torch.nn.Linear])
            stats = {name: [None, 0] for name in linears}

            def hook(name):
                def add(_, inp, out):
                    stats[name][0], stats[name][1] = accumulate_hessian(stats[name][0], stats[name][1], inp[0].data)
                return add
            handles = [m.register_forward_hook(hook(name)) for name, m in linears.items()]
            try:
                for x in inps:
                    block(x, *args, **kwargs)
            finally:
                for h in handles:
                    h.remove()
            for name, lin in linears.items():
                full = f"{prefix}.{i}.{name}"
                b = bits_for(bits_by_layer, full, name, bits)
                layer = quantize_linear(lin, stats[name][0], b, group_size, act_order, sym, damp_percent, device=dev, debug=debug,
                                        static_groups=static_groups)
                lin.weight.data = torch.empty(0, dtype=lin.weight.dtype, device=lin.weight.device)   # the block runs on the q_layer
                modelutils.set_op_by_name(block, name, layer)
                cfg.by_layer[full] = {"wbits": b, "groupsize": layer.groupsize}
                losses[full] = layer.gptq_loss
                if debug:
                    rtn_losses[full], losses_hd[full] = layer.gptq_rtn_loss, layer.gptq_loss_hd
                stats[name][0] = None
            inps = [first(block(x, *args, **kwargs)) for x in inps]
    model.to(dev)
    model.sibling_groups = install_sibling_groups(model, [QuantLinearGPTQ])
    model.quant_config = cfg
    model.gptq_losses = losses
    if debug:
        model.gptq_rtn_losses, model.gptq_losses_hd = rtn_losses, losses_hd
    return model
