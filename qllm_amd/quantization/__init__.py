"""Quantizers that run on the MI355X: HQQ (data-free; hqq.py over the library's fused proximal solver)."""
from .hqq import hqq_quantize_weight, quantize_linear, quantize_model  # noqa: F401
