"""Quantizers that run on the MI355X: HQQ (data-free; hqq.py over the library's fused proximal solver) and GPTQ (calibrated; gptq.py over
the library's fused column solver).  `quantize_linear` / `quantize_model` are HQQ's; GPTQ's live in `qllm_amd.quantization.gptq`."""
from .hqq import hqq_quantize_weight, quantize_linear, quantize_model  # noqa: F401
from . import gptq  # noqa: F401
from .gptq import accumulate_hessian, gptq_quantize_weight  # noqa: F401
from .gptq import quantize_linear as gptq_quantize_linear, quantize_model as gptq_quantize_model  # noqa: F401
