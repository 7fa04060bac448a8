// The RESID forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp) around act(gate) * up: y = residual +
// linear(w, silu(gate) * up) -- the down_proj launch of a SwiGLU MLP with neither the elementwise kernel in front of it nor the one behind.
// One instantiation per batch-1 (MR = 1) form strip1.hip's launch_e builds without AR / DBG, with the same caps on the round length per
// form (strip1_resid_forms.inc); strip1.hip, strip1_swiglu.hip and what they build are untouched.  qllm_linear_forward_residual (capi.hip) is the only caller.
#include "strip1_kernel.hpp"

#define QLLM_RESID_KERNEL strip1_swiglu_resid_kernel
#define QLLM_RESID_LAUNCH launch_strip1_swiglu_resid
#include "strip1_resid_forms.inc"
