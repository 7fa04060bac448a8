"""HQQ quantization on the device: fp16 model in -> QuantLinearHQQ layers out.

The reference's path is HQQQuant.do_quantize (qllm/quantization/hqq/quant_hqq.py:17-48) over InternalHQQQuantizer.quantize
(_hqq_quantizer.py:66-121, proximal solver :29-64) followed by QuantLinearHQQ.pack; here solver, rounding and bit packing are ONE
library call (qllm_hqq_quantize, csrc/hqq_quant.hip) per layer.  HQQ needs no calibration data.  There is no CPU fallback: weights that
are not on a HIP device are moved to one."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from .. import ops
from ._common import bits_for, decoder_blocks, layer_dtype, need_device

HQQ_DEFAULTS = dict(iters=20, lp_norm=0.7, beta=10.0, kappa=1.01)   # _hqq_quantizer.py:30


def hqq_quantize_weight(weight: torch.Tensor, bits: int, group_size: int = 64, **opt):
    """weight [N, K] (out_features x in_features; fp16 / bf16 / fp32 on a HIP device) -> (qweight i32 [K*bits/32, N], scales f16
    [K/g, N], zeros f16 [K/g, N]): QuantLinearHQQ's buffers.  `opt`: iters, lp_norm, beta, kappa (the reference's defaults)."""
    unknown = set(opt) - set(HQQ_DEFAULTS)
    if unknown:
        raise TypeError(f"unknown solver options {sorted(unknown)}; known: {sorted(HQQ_DEFAULTS)}")
    need_device(weight, "hqq_quantize_weight")
    return ops.hqq_quantize(weight.contiguous(), bits, group_size, **{**HQQ_DEFAULTS, **opt})[:3]


def quantize_linear(linear: torch.nn.Linear, bits: int, group_size: int = 64, device=None, **opt):
    """nn.Linear -> QuantLinearHQQ on the device (`device`, default: the linear's own if it is a HIP device, else cuda:0).  The bias is
    carried over; the linear's fp16 weight is released (its storage is replaced by an empty tensor)."""
    from ..modeling.q_layers import QuantLinearHQQ
    w = linear.weight.data
    dev = torch.device(device) if device is not None else (w.device if w.is_cuda else torch.device("cuda:0"))
    n, k = w.shape
    g = k if group_size == -1 else group_size
    qweight, scales, zeros = hqq_quantize_weight(w.to(dev), bits, g, **opt)
    dtype = layer_dtype(w)
    layer = QuantLinearHQQ(bits, g, k, n, linear.bias is not None, dtype=dtype)
    layer.qweight, layer.scales, layer.qzeros = qweight, scales.to(dtype), zeros.to(dtype)
    if linear.bias is not None:
        layer.bias = linear.bias.data.to(device=dev, dtype=dtype)
    linear.weight.data = torch.empty(0, dtype=w.dtype, device=w.device)
    del w
    return layer


def quantize_model(model, bits: int, group_size: int = 64, bits_by_layer: Optional[Dict[str, int]] = None, device="cuda:0", **opt):
    """Every nn.Linear inside the decoder blocks -> QuantLinearHQQ, one block at a time on the device (quant_hqq.py:23-46: only one
    block's fp16 weights are ever resident next to the quantized model).  `bits_by_layer` maps a module kind ("q_proj") or a full
    module name ("model.layers.0.mlp.up_proj") to its width; everything else gets `bits`.  lm_head and the embeddings stay as they are.
    The model is left on `device` with `quant_config` set (version HQQ, per-layer widths), ready for modeling.base.save_quantized /
    load_quantized."""
    from ..modeling import base
    from ..modeling.q_layers import QuantLinearHQQ, install_sibling_groups
    from ..utils import modelutils
    dev = torch.device(device)
    bits_by_layer = dict(bits_by_layer or {})
    prefix, blocks = decoder_blocks(model)
    cfg = base.QuantConfig(bits=bits, group_size=group_size, version="HQQ", quant_method="hqq")
    with torch.no_grad():
        for i in range(len(blocks)):
            block = blocks[i].to(dev)
            for name in list(modelutils.find_layers(block, [torch.nn.Linear])):
                full = f"{prefix}.{i}.{name}"
                b = bits_for(bits_by_layer, full, name, bits)
                layer = quantize_linear(modelutils.get_op_by_name(block, name), b, group_size, device=dev, **opt)
                modelutils.set_op_by_name(block, name, layer)
                cfg.by_layer[full] = {"wbits": b, "groupsize": layer.groupsize}
    model.to(dev)
    model.sibling_groups = install_sibling_groups(model, [QuantLinearHQQ])
    model.quant_config = cfg
    return model
