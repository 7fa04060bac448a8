// The RESID forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp): y = residual + linear(w, x) with the add formed by the
// threads that store the output -- the o_proj launch of a decoder layer without the elementwise kernel behind it.
// One instantiation per batch-1 (MR = 1) form strip1.hip's launch_e builds without AR / DBG, with the same caps on the round length per
// form (strip1_resid_forms.inc); strip1.hip and what it builds are untouched.  qllm_linear_forward_residual (capi.hip) is the only caller.
#include "strip1_kernel.hpp"

#define QLLM_RESID_KERNEL strip1_resid_kernel
#define QLLM_RESID_LAUNCH launch_strip1_resid
#include "strip1_resid_forms.inc"
