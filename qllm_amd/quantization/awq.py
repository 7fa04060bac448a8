"""AWQ quantization on the device: fp16 model + calibration token ids in -> WQLinear_GEMM layers out.

The reference's path is AWQQuant.do_quantize (qllm/quantization/awq/quant_awq.py:107-134) over InternalAWQuantizer.fast_quant_layer
(_awq_quantizer.py:381-399): per decoder block the scale search (auto_scale_block / _search_module_scale), apply_scale, the clip search
(auto_clip_block / auto_clip_layer), apply_clip, pseudo_quantize_tensor, and WQLinear_GEMM.pack.  Here the two device steps are library
calls: the scale search's inner step (scale, pseudo-quantize, unscale) and the final quantization are qllm_awq_quantize, and the whole
clip search of a layer -- ten candidates over [rows, tokens, groups, g] tensors in the reference -- is ONE qllm_awq_clip_search over
per-group Gram matrices of the layer's input (csrc/awq_quant.hip).  The statistics, the Gram matrices, folding the scales into the
previous op and packing are torch plumbing.  All arithmetic of the two kernels and the losses is fp32 whatever the model's dtype (the
reference works in the model's fp16); the activation and weight statistics are accumulated in fp32.  There is no CPU quantizer.

Not built (the reference's other switches and families): symmetric grids (zero_point=False), group_size = -1, the model families of
sequential_layes_awq_config.py other than the Llama-shaped block (Llama, Mistral, Qwen2, Yi) and their ScaledActivation, Mixtral,
USE_ACCUMULATE_BATCH; packed layers are 4-bit (WQLinear_GEMM holds nothing else)."""
from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .. import ops
from ._common import capture_first_block_inputs, decoder_blocks, first, layer_dtype, need_device

N_GRID = 20               # ratios of the scale search and the grid of the clip search (_awq_quantizer.py:320, :184)
MAX_SHRINK = 0.5
N_SAMPLE_TOKEN = 512
NO_CLIP = ("q_", "k_", "query", "key", "Wqkv")       # auto_clip_block: "due to qk bmm, it is hard to clip precisely"


def sample_tokens(x: torch.Tensor, n_sample_token: int = N_SAMPLE_TOKEN) -> torch.Tensor:
    """auto_clip_layer's token sample of x [tokens, K]: every (tokens // n_sample_token)-th token; below n_sample_token tokens (where
    the reference divides by zero) every token."""
    x = x.reshape(-1, x.shape[-1])
    return x[0::max(1, x.shape[0] // n_sample_token)]


def gram_matrices(x: torch.Tensor, g: int, n_sample_token: int = N_SAMPLE_TOKEN) -> torch.Tensor:
    """The clip search's input statistics: x [.., K] -> f32 [K/g, g, g], per group X^T X / tokens over the sampled tokens."""
    xs = sample_tokens(x, n_sample_token).float()
    xs = xs.reshape(xs.shape[0], -1, g)
    return (torch.einsum("tjg,tjh->jgh", xs, xs) / xs.shape[0]).contiguous()


def clip_linear(linear: torch.nn.Linear, x: torch.Tensor, bits: int, g: int, n_sample_token: int = N_SAMPLE_TOKEN):
    """auto_clip_layer for one linear and its input x [.., K]: (best_max f32 [N, K/g], best_idx i32 [N, K/g], err f32 [N, K/g, 2]:
    the unclipped and the chosen output error of every (row, group)).  The weight is left as it is."""
    w = linear.weight.data
    need_device(w, "clip_linear")
    return ops.awq_clip_search(w.contiguous(), gram_matrices(x.to(w.device), g, n_sample_token), bits, g, N_GRID, MAX_SHRINK)


def fold_scales(block, prev_op, layers, s: torch.Tensor):
    """apply_scale for one group (_awq_quantizer.py:101-127): the layers' input channels are multiplied by s and the op that feeds them
    is divided by it -- a norm's weight (and bias), or the last len(s) output rows of a previous linear and its bias.  Any other
    previous op raises (the reference's ScaledActivation is not built)."""
    layers = list(layers)
    if isinstance(prev_op, torch.nn.Linear):
        if len(layers) != 1:
            raise ValueError("a previous linear feeds exactly one layer")
        w = prev_op.weight.data
        sv = s.to(device=w.device, dtype=w.dtype)
        w[-sv.numel():].div_(sv.view(-1, 1))
        if prev_op.bias is not None:
            prev_op.bias.data.div_(sv.view(-1))
    elif isinstance(prev_op, torch.nn.LayerNorm) or "rmsnorm" in str(prev_op.__class__).lower():
        w = prev_op.weight.data
        w.div_(s.to(device=w.device, dtype=w.dtype))
        if getattr(prev_op, "bias", None) is not None:
            prev_op.bias.data.div_(s.to(device=w.device, dtype=w.dtype))
    else:
        raise NotImplementedError(f"prev_op {type(prev_op)} not supported yet!")
    for fc in layers:
        fc.weight.data.mul_(s.to(device=fc.weight.device, dtype=fc.weight.dtype).view(1, -1))
    for m in [prev_op] + layers:
        for p in m.parameters():
            if not torch.isfinite(p).all():
                raise RuntimeError(f"folding the scales left non-finite values in {type(m).__name__}")


def _run(module, x: torch.Tensor, kwargs):
    """module over x [batch, tokens, K] one calibration row at a time (the captured keyword arguments are those of one row)."""
    if x.dim() < 3:
        return first(module(x, **kwargs))
    return torch.cat([first(module(x[b:b + 1], **kwargs)) for b in range(x.shape[0])], dim=0)


def search_scales(module2inspect, linears, x: torch.Tensor, kwargs: Optional[dict], bits: int, g: int):
    """_search_module_scale (_awq_quantizer.py:292-361) for the linears that read x [.., K]: (best_s f32 [K], best_ratio,
    history: the N_GRID losses).  x_mean = mean |x| per channel, w_mean = mean over the rows of |w| / (max |w| of its group + 1e-6); for
    ratio r = i / N_GRID: s = (x_mean^r / (w_mean^(1-r) + 1e-4)).clamp(1e-4), normalised by sqrt(max s * min s); every linear's weight
    becomes pseudo_quantize(W * s) / s (ops.awq_quantize with col_scale=s), module2inspect runs, and the loss is the mean squared
    difference to its output on the original weights, in fp32.  The first strictly smallest loss wins.  The weights are the originals
    again afterwards (they are never written: the candidates are separate device tensors)."""
    linears = list(linears)
    kwargs = dict(kwargs or {})
    kwargs.pop("use_cache", None)
    orig = [fc.weight.data for fc in linears]
    need_device(orig[0], "search_scales")
    dev = orig[0].device
    x = x.to(dev)
    weight = torch.cat([w.float() for w in orig], dim=0)
    wg = weight.abs().view(-1, g)
    w_mean = (wg / (wg.amax(dim=1, keepdim=True) + 1e-6)).view(weight.shape).mean(0)
    del weight, wg
    x_mean = x.reshape(-1, x.shape[-1]).float().abs().mean(0)
    losses, scales = [], []
    with torch.no_grad():
        org_out = _run(module2inspect, x, kwargs)
        try:
            for i in range(N_GRID):
                ratio = i / N_GRID
                s = (x_mean.pow(ratio) / (w_mean.pow(1 - ratio) + 1e-4)).clamp(min=1e-4).view(-1)
                s = (s / (s.max() * s.min()).sqrt()).contiguous()
                for fc, w in zip(linears, orig):
                    fc.weight.data = ops.awq_quantize(w.contiguous(), bits, g, col_scale=s, want=("wq",))[3]
                out = _run(module2inspect, x, kwargs)
                losses.append((org_out - out).float().pow(2).mean())
                scales.append(s)
        finally:
            for fc, w in zip(linears, orig):
                fc.weight.data = w
    history = torch.stack(losses).cpu().tolist()       # the one host synchronisation of the search
    best = -1
    for i, loss in enumerate(history):
        if loss < (float("inf") if best < 0 else history[best]):
            best = i
    if best < 0:
        raise RuntimeError(f"the scale search found no finite loss: {history}")
    if not torch.isfinite(scales[best]).all():
        raise RuntimeError("the scale search's best scales are not finite")
    return scales[best], best / N_GRID, history


def _llama_groups(block, feat: Dict[str, torch.Tensor], kwargs):
    """get_llama_layers (sequential_layes_awq_config.py:545-581): (prev_op, layer names, input, module2inspect, kwargs)."""
    att, mlp = block.self_attn, block.mlp
    groups = [(block.input_layernorm, ["self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"], feat["self_attn.q_proj"], att, kwargs)]
    if att.v_proj.weight.shape == att.o_proj.weight.shape:
        groups.append((att.v_proj, ["self_attn.o_proj"], feat["self_attn.o_proj"], att.o_proj, {}))
    groups.append((block.post_attention_layernorm, ["mlp.gate_proj", "mlp.up_proj"], feat["mlp.gate_proj"], mlp, {}))
    groups.append((mlp.up_proj, ["mlp.down_proj"], feat["mlp.down_proj"], mlp.down_proj, {}))
    return groups


def _is_llama_block(block) -> bool:
    att, mlp = getattr(block, "self_attn", None), getattr(block, "mlp", None)
    return (all(hasattr(att, n) for n in ("q_proj", "k_proj", "v_proj", "o_proj")) and
            all(hasattr(mlp, n) for n in ("gate_proj", "up_proj", "down_proj")) and
            hasattr(block, "input_layernorm") and hasattr(block, "post_attention_layernorm") and
            "mixtral" not in block.__class__.__name__.lower())


def quantize_block(block, inps: List[torch.Tensor], args, kwargs, bits: int = 4, group_size: int = 128, auto_scale: bool = True,
                   auto_clip: bool = True, prefix: str = ""):
    """One Llama-shaped decoder block on the device, fast_quant_layer + _apply_quant + pack: every nn.Linear becomes a WQLinear_GEMM.
    `inps`: the block's inputs, one [1, tokens, hidden] tensor per calibration row; args / kwargs: what the model hands the block.
    Returns (the block's outputs on its quantized layers, {prefix + linear name: {"ratio", "history", "clip_err"}})."""
    from ..modeling.q_layers import WQLinear_GEMM
    from ..utils import modelutils
    if not _is_llama_block(block):
        raise NotImplementedError(f"the AWQ quantizer knows the Llama-shaped decoder block only, not {type(block).__name__}")
    if group_size not in (32, 64, 128):
        raise NotImplementedError(f"group_size must be 32, 64 or 128 (got {group_size}); -1 is not built")
    linears = modelutils.find_layers(block, [torch.nn.Linear])
    for lin in linears.values():
        need_device(lin.weight.data, "quantize_block")
    report = {f"{prefix}{name}": {"ratio": None, "history": None, "clip_err": None} for name in linears}
    kwargs = {k: v for k, v in kwargs.items() if k != "use_cache"}
    with torch.no_grad():
        # every linear's input, on the device
        feat = {name: [] for name in linears}
        handles = [m.register_forward_hook(lambda _, inp, out, name=name: feat[name].append(inp[0].detach())) for name, m in linears.items()]
        try:
            for x in inps:
                block(x, *args, **kwargs)
        finally:
            for h in handles:
                h.remove()
        feat = {name: torch.cat(v, dim=0) for name, v in feat.items()}
        if auto_scale:
            found = []
            for prev_op, names, x, inspect, kw in _llama_groups(block, feat, kwargs):
                s, ratio, history = search_scales(inspect, [linears[n] for n in names], x, kw, bits, group_size)
                found.append((prev_op, names, s))
                for n in names:
                    report[f"{prefix}{n}"].update(ratio=ratio, history=history)
            for prev_op, names, s in found:       # all four searches see the unscaled block, as auto_scale_block's do
                fold_scales(block, prev_op, [linears[n] for n in names], s)
                for n in names:
                    feat[n] = feat[n] / s.to(feat[n].dtype).view(1, -1)
        for name, lin in linears.items():
            w = lin.weight.data.contiguous()
            clip = None
            if auto_clip and not any(t in name for t in NO_CLIP):
                clip, _, err = clip_linear(lin, feat[name], bits, group_size)
                report[f"{prefix}{name}"]["clip_err"] = err.sum(dim=(0, 1))
            codes, scales, zeros, _ = ops.awq_quantize(w, bits, group_size, clip=clip, want=("codes", "scales", "zeros"))
            n, k = w.shape
            dtype = layer_dtype(w)
            layer = WQLinear_GEMM(bits, group_size, k, n, lin.bias is not None, dtype=dtype)
            layer.pack_on_device(codes, zeros.t().contiguous().to(torch.int32))
            layer.scales = scales.t().contiguous().to(dtype)
            if lin.bias is not None:
                layer.bias = lin.bias.data.to(dtype)
            lin.weight.data = torch.empty(0, dtype=w.dtype, device=w.device)     # the block runs on the q_layer
            modelutils.set_op_by_name(block, name, layer.to(w.device))
            feat[name] = None
        for r in report.values():
            if r["clip_err"] is not None:
                r["clip_err"] = [float(v) for v in r["clip_err"].cpu()]
        outs = [first(block(x, *args, **kwargs)) for x in inps]
    return outs, report


def quantize_model(model, calibration_input_ids, bits: int = 4, group_size: int = 128, auto_scale: bool = True, auto_clip: bool = True,
                   device="cuda:0"):
    """Every nn.Linear inside the decoder blocks -> WQLinear_GEMM, AWQQuant.do_quantize: the first block's inputs and keyword arguments
    are captured from a forward over `calibration_input_ids` ([rows, tokens] token ids); then block by block quantize_block, whose
    outputs on the quantized layers are the next block's inputs.  The model's weights must be on `device` already (there is no CPU
    quantizer).  lm_head and the embeddings stay as they are.  The model is left with `quant_config` (version GEMM, method awq) for
    modeling.base.save_quantized / load_quantized, sibling groups installed, and `awq_report` {module name: {"ratio": the group's best
    ratio, "history": its 20 losses, "clip_err": [unclipped, chosen] output error summed over the layer, None for q / k}}."""
    from ..modeling import base
    from ..modeling.q_layers import WQLinear_GEMM, install_sibling_groups
    dev = torch.device(device)
    prefix, blocks = decoder_blocks(model)
    for p in model.parameters():
        need_device(p, "quantize_model")
    if bits != 4:
        raise NotImplementedError("WQLinear_GEMM packs 4-bit layers only")
    cfg = base.QuantConfig(bits=bits, group_size=group_size, version="GEMM", quant_method="awq")
    ids = torch.as_tensor(calibration_input_ids)
    if ids.dim() == 1:
        ids = ids.unsqueeze(0)
    report = {}
    with torch.no_grad():
        inps, args, kwargs = capture_first_block_inputs(model, blocks, ids, dev)
        for i in range(len(blocks)):
            block = blocks[i].to(dev)
            inps, rep = quantize_block(block, inps, args, kwargs, bits, group_size, auto_scale, auto_clip, prefix=f"{prefix}.{i}.")
            report.update(rep)
            for name in rep:
                cfg.by_layer[name] = {"wbits": bits, "groupsize": group_size}
    model.sibling_groups = install_sibling_groups(model, [WQLinear_GEMM])
    model.quant_config = cfg
    model.awq_report = report
    return model
