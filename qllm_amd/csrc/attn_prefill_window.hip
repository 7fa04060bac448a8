// The sliding-window variants of the prefill attention kernel (attn_prefill.hip has the text, attn_prefill_kernel.hpp the code): a unit of
// their own: the unit without a window holds only kernels without window code.
#include "attn_prefill_kernel.hpp"

namespace qllm {

int launch_attn_prefill_window(const AttnPrefillParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  return launch_attn_prefill_variant<true>(p, head_dim, act_bf16, stream);
}

}  // namespace qllm
