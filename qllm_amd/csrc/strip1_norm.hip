// The NORM forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp): y_i = linear(w_i, RMSNorm(x)) for the siblings that share
// x (q/k/v, gate/up) with the norm formed while the activations are staged -- the grouped launch behind input_layernorm /
// post_attention_layernorm without the norm's kernels in front of it.  One instantiation per batch-1 (MR = 1) form strip1.hip's launch_e
// builds without AR / DBG, with the same caps on the round length per form; strip1.hip and what it builds are untouched.  M = 1 only:
// the four-row forms (M = 2..4) are out of scope -- they would double the instantiations, and the modules send one row.
// qllm_linear_forward_rmsnorm (capi.hip) is the only caller.
#include "strip1_kernel.hpp"

namespace qllm {

// Second launch bound (minimum waves per SIMD) per form, from the compiler's report (-Rpass-analysis=kernel-resource-usage).  The norm
// weight's chunks are 4 XL more live registers across the load batch, as the up vector's are in the SWIGLU forms; with the forms next to
// their bound parking them in LDS once they have arrived (strip1_body.inc, NORM / PARK) every form fits its twin's bound without scratch:
// 64 registers (8 waves per SIMD) for the plain forms up to rounds of 24 k-steps, 128 (4: what a 16-wave block needs anyway) for the rest.
template <int MAXS, bool G64, bool B3>
constexpr int norm_waves() {
  return (MAXS <= 24 && !G64 && !B3) ? 8 : 4;
}

template <int NW, int MAXS, bool EXACT, bool G64 = false, bool B3 = false>
static int launch_t(const Strip1Params &p, dim3 grid, hipStream_t stream) {
  constexpr int lds_bytes = strip1_lds_bytes<NW, MAXS, 1>() + kStrip1NormLdsBytes;   // (+ the waves' partial sums of squares)
  static_assert(lds_bytes <= 160 * 1024, "LDS of one CU");
  constexpr int waves = norm_waves<MAXS, G64, B3>();
  if constexpr (lds_bytes > 64 * 1024) {
    static DeviceLatch attr_done;
    if (int rc = lds_optin(attr_done, (const void *)strip1_norm_kernel<NW, MAXS, EXACT, G64, 1, B3, waves>)) return rc;
  }
  hipLaunchKernelGGL((strip1_norm_kernel<NW, MAXS, EXACT, G64, 1, B3, waves>), grid, dim3(NW * 64), lds_bytes, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// the batch-1 forms of one (NW, MAXS) pair, as launch_e of strip1.hip picks them
template <int NW, int MAXS>
struct NormForms {
  static int launch(const Strip1Params &p, dim3 grid, hipStream_t stream) {
    const bool exact = NW * MAXS == p.T;
    if (p.bits3) {  // 3-bit layers: 64- and 128-wide groups, rounds of up to 32 k-steps
      if constexpr (MAXS <= 32) {
        if (p.group64) return exact ? launch_t<NW, MAXS, true, true, true>(p, grid, stream) : launch_t<NW, MAXS, false, true, true>(p, grid, stream);
        return exact ? launch_t<NW, MAXS, true, false, true>(p, grid, stream) : launch_t<NW, MAXS, false, false, true>(p, grid, stream);
      } else {
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: 3-bit layers on the batch-1 kernel stop at K = 16384");
      }
    }
    if (p.group64) {  // 64-wide groups: rounds of up to 48 k-steps
      if constexpr (MAXS <= 48)
        return exact ? launch_t<NW, MAXS, true, true>(p, grid, stream) : launch_t<NW, MAXS, false, true>(p, grid, stream);
      else
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: 64-wide groups on the batch-1 kernel stop at K = 24576");
    }
    return exact ? launch_t<NW, MAXS, true>(p, grid, stream) : launch_t<NW, MAXS, false>(p, grid, stream);
  }
};

// every (NW, MAXS) pair of launch_strip1's table (strip1.hip)
#define QLLM_NORM_PAIRS(X) \
  X(4, 8) X(4, 16) X(4, 32) X(8, 16) X(7, 16) X(8, 24) X(8, 32) X(16, 16) X(16, 24) X(15, 24) X(16, 32) X(16, 40) X(16, 48) X(16, 56) X(16, 64)

int launch_strip1_norm(const Strip1Params &p, int nw, int maxs, int n_prob, int max_strips, hipStream_t stream) {
  if (p.M != 1) return set_error(QLLM_ERR_UNSUPPORTED, "internal: the fused RMSNorm forms take one row");
  const dim3 grid(max_strips, n_prob);
#define X(NW, MAXS) \
  if (nw == NW && maxs == MAXS) return NormForms<NW, MAXS>::launch(p, grid, stream);
  QLLM_NORM_PAIRS(X)
#undef X
  return set_error(QLLM_ERR_UNSUPPORTED, "fused RMSNorm: no batch-1 instantiation for nw=%d round=%d", nw, maxs);
}

}  // namespace qllm
