// The sliding-window variants of the decode attention kernel (attn_decode.hip has the text, attn_decode_kernel.hpp the code): a unit of
// their own: the unit without a window holds only kernels without window code.
#include "attn_decode_kernel.hpp"

namespace qllm {

int launch_attn_decode_window(const AttnDecodeParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  return launch_attn_decode_variant<true>(p, head_dim, act_bf16, stream);
}

}  // namespace qllm
