"""What the HQQ, GPTQ and AWQ quantizers share: finding the decoder blocks, capturing what the model hands the first one, and the
small per-layer rules (the layer's dtype, its width, "the weight must be on the device")."""
from __future__ import annotations

from typing import Dict

import torch


def decoder_blocks(model):
    """(prefix, ModuleList) of the decoder blocks: the longest nn.ModuleList of the model (model.layers, transformer.h, ...)."""
    best = None
    for name, m in model.named_modules():
        if isinstance(m, torch.nn.ModuleList) and (best is None or len(m) > len(best[1])):
            best = (name, m)
    if best is None:
        raise ValueError("no nn.ModuleList of decoder blocks found in the model")
    return best


class Stop(Exception):
    pass


class Catcher(torch.nn.Module):
    """Stands in for the first decoder block: records what the model hands it, then ends the forward."""

    def __init__(self):
        super().__init__()
        self.inputs, self.args, self.kwargs = [], (), {}

    def forward(self, hidden, *args, **kwargs):
        self.inputs.append(hidden)
        self.args, self.kwargs = args, kwargs
        raise Stop()


def first(out):
    return out[0] if isinstance(out, (tuple, list)) else out


def capture_first_block_inputs(model, blocks, ids: torch.Tensor, dev):
    """(inps, args, kwargs): the first decoder block's input for every row of `ids` ([rows, tokens] token ids, one calibration batch per
    row) and the positional / keyword arguments the model hands its blocks.  Everything but the blocks goes to `dev`, a catcher stands
    where block 0 was while the rows run; the block list is the original one again afterwards, whatever the forward raises."""
    saved = [blocks[i] for i in range(len(blocks))]
    catcher = Catcher()
    del blocks[:]
    blocks.append(catcher)
    try:
        model.to(dev)
        for j in range(ids.shape[0]):
            try:
                model(ids[j:j + 1].to(dev), use_cache=False)
            except Stop:
                pass
    finally:
        del blocks[:]
        blocks.extend(saved)
    if len(catcher.inputs) != ids.shape[0]:
        raise RuntimeError("the decoder blocks were not reached by the model's forward")
    return catcher.inputs, catcher.args, catcher.kwargs


def layer_dtype(w: torch.Tensor) -> torch.dtype:
    """The quantized layer's dtype: the weight's if it is a 16-bit float, else fp16."""
    return w.dtype if w.dtype in (torch.float16, torch.bfloat16) else torch.float16


def bits_for(bits_by_layer: Dict[str, int], full_name: str, name: str, default: int) -> int:
    """The width of one linear: by its full module name, else by its kind (the last component of `name`), else `default`."""
    return bits_by_layer.get(full_name, bits_by_layer.get(name.rsplit(".", 1)[-1], default))


def need_device(t: torch.Tensor, what: str):
    if not t.is_cuda:
        raise RuntimeError(f"{what} needs the weight on an MI355X: qllm_amd ships no CPU quantizer")
