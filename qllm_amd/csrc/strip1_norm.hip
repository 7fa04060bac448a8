// The NORM forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp): y_i = linear(w_i, RMSNorm(x)) for the siblings that share
// x (q/k/v, gate/up) with the norm formed while the activations are staged -- the grouped launch behind input_layernorm /
// post_attention_layernorm without the norm's kernels in front of it.  One instantiation per batch-1 (MR = 1) form of the plain family
// (strip1.hip): the family below is all this unit adds to strip1_forms.hpp's table.  M = 1 only: the four-row forms (M = 2..4) are out
// of scope -- they would double the instantiations, and the modules send one row.  The norm weight's chunks are 4 XL more live
// registers across the load batch; the forms next to their bound park them in LDS (strip1_body.inc, NORM / PARK).
// qllm_linear_forward_rmsnorm (capi.hip) is the only caller.
#include "strip1_forms.hpp"
#include "strip1_kernel.hpp"

namespace qllm {

struct Strip1Norm {
  static constexpr const char *kWhat = "fused RMSNorm";
  static constexpr int kLdsExtra = kStrip1NormLdsBytes, kMaxRound = 64;   // (+ the waves' partial sums of squares)
  static constexpr bool kRows4 = false, kG64B3 = true;
  template <int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3>
  static Strip1Kernel kernel() { return strip1_norm_kernel<NW, MAXS, EXACT, G64, MR, B3, strip1_min_waves(MAXS, G64, MR, B3)>; }
};

int launch_strip1_norm(const Strip1Params &p, int nw, int maxs, int n_prob, int max_strips, hipStream_t stream) {
  if (p.M != 1) return set_error(QLLM_ERR_UNSUPPORTED, "internal: the fused RMSNorm forms take one row");
  return strip1_launch<Strip1Norm>(p, nw, maxs, dim3(max_strips, n_prob), stream);
}

}  // namespace qllm
