"""Quantizers that run on the MI355X: HQQ (data-free; hqq.py over the library's fused proximal solver), GPTQ (calibrated; gptq.py over
the library's fused column solver) and AWQ (calibrated; awq.py over the library's clip search and pseudo-quantizer).  `quantize_linear` /
`quantize_model` are HQQ's; GPTQ's live in `qllm_amd.quantization.gptq`, AWQ's in `qllm_amd.quantization.awq`."""
from .hqq import hqq_quantize_weight, quantize_linear, quantize_model  # noqa: F401
from . import gptq  # noqa: F401
from .gptq import accumulate_hessian, gptq_quantize_weight  # noqa: F401
from .gptq import quantize_linear as gptq_quantize_linear, quantize_model as gptq_quantize_model  # noqa: F401
from . import awq  # noqa: F401
from .awq import clip_linear, fold_scales, search_scales  # noqa: F401
from .awq import quantize_block as awq_quantize_block, quantize_model as awq_quantize_model  # noqa: F401
