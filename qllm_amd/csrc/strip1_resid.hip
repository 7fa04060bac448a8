// The RESID forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp): y = residual + linear(w, x) with the add formed by the
// threads that store the output -- the o_proj launch of a decoder layer without the elementwise kernel behind it.
// One instantiation per batch-1 (MR = 1) form of the plain family (strip1.hip): the family below is all this unit adds to
// strip1_forms.hpp's table.  The residual element is ONE more live register from the load batch to the epilogue.
// qllm_linear_forward_residual (capi.hip) is the only caller.
#include "strip1_forms.hpp"
#include "strip1_kernel.hpp"

namespace qllm {

struct Strip1Resid {
  static constexpr const char *kWhat = "fused residual";
  static constexpr int kLdsExtra = 0, kMaxRound = 64;
  static constexpr bool kRows4 = false, kG64B3 = true;
  template <int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3>
  static Strip1Kernel kernel() { return strip1_resid_kernel<NW, MAXS, EXACT, G64, B3, strip1_min_waves(MAXS, G64, MR, B3)>; }
};

int launch_strip1_resid(const Strip1Params &p, int nw, int maxs, int n_strips, hipStream_t stream) {
  if (p.M != 1) return set_error(QLLM_ERR_UNSUPPORTED, "internal: the fused residual forms take one row");
  return strip1_launch<Strip1Resid>(p, nw, maxs, dim3(n_strips, 1), stream);
}

}  // namespace qllm
