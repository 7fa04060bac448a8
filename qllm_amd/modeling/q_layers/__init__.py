"""Quantized linear layers with the reference's module contract (qllm/modeling/q_layers/*.py), forward on MI355X."""
from .quant_linear_gptq import QuantLinearGPTQ  # noqa: F401
from .quant_linear_awq import WQLinear_GEMM  # noqa: F401
from .quant_linear_hqq import QuantLinearHQQ  # noqa: F401
from .quant_linear_onnxruntime import QuantLinearORT  # noqa: F401
from .fused import SiblingGroup, fuse_siblings, install_sibling_groups  # noqa: F401
from .fused_mlp import install_fused_mlp, uninstall_fused_mlp  # noqa: F401
from .fused_norm import install_fused_norm, make_quant_norm, uninstall_fused_norm  # noqa: F401
from .fused_residual import install_fused_residual, uninstall_fused_residual  # noqa: F401
from .fused_rope import install_fused_rope, uninstall_fused_rope  # noqa: F401
from .fused_attention import install_fused_attention, uninstall_fused_attention  # noqa: F401
