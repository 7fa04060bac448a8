// The SWIGLU forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp): y = linear(w, silu(gate) * up) with the product
// formed while the activations are staged -- the down_proj launch of a SwiGLU MLP without the elementwise kernel in front of it.
// One instantiation per form of the plain family (strip1.hip), four-row forms included: the family below is all this unit adds to
// strip1_forms.hpp's table.  The up vector's chunks are 4 XL more live registers per batch row across the load batch; the forms next
// to their bound park them in LDS once they have arrived (strip1_body.inc, PARK).  qllm_linear_forward_swiglu (capi.hip) is the only caller.
#include "strip1_forms.hpp"
#include "strip1_kernel.hpp"

namespace qllm {

struct Strip1Swiglu {
  static constexpr const char *kWhat = "fused SwiGLU";
  static constexpr int kLdsExtra = 0, kMaxRound = 64;
  static constexpr bool kRows4 = true, kG64B3 = true;
  template <int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3>
  static Strip1Kernel kernel() { return strip1_swiglu_kernel<NW, MAXS, EXACT, G64, MR, B3, strip1_min_waves(MAXS, G64, MR, B3)>; }
};

int launch_strip1_swiglu(const Strip1Params &p, int nw, int maxs, int n_strips, hipStream_t stream) {
  return strip1_launch<Strip1Swiglu>(p, nw, maxs, dim3(n_strips, 1), stream);
}

}  // namespace qllm
