// The SWIGLU forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp): y = linear(w, silu(gate) * up) with the product
// formed while the activations are staged -- the down_proj launch of a SwiGLU MLP without the elementwise kernel in front of it.
// One instantiation per form strip1.hip's launch_e builds without AR / DBG, with the same caps on the round length per form; strip1.hip
// and what it builds are untouched.  qllm_linear_forward_swiglu (capi.hip) is the only caller.
#include "strip1_kernel.hpp"

namespace qllm {

// Second launch bound (minimum waves per SIMD) per form, from the compiler's report (-Rpass-analysis=kernel-resource-usage; DESIGN 3.10
// has the table).  The up vector's chunks are 4 XL more live registers per batch row across the load batch; with the forms next to their
// bound parking them in LDS once they have arrived (strip1_body.inc, PARK) every form fits its twin's bound without scratch: 64 registers
// (8 waves per SIMD) for the plain forms up to rounds of 24 k-steps, 128 (4: what a 16-wave block needs anyway) for the rest.
template <int MAXS, bool G64, int MR, bool B3>
constexpr int swiglu_waves() {
  return (MAXS <= 24 && !G64 && MR == 1 && !B3) ? 8 : 4;
}

template <int NW, int MAXS, bool EXACT, bool G64 = false, int MR = 1, bool B3 = false>
static int launch_t(const Strip1Params &p, int n_strips, hipStream_t stream) {
  constexpr int lds_bytes = strip1_lds_bytes<NW, MAXS, MR>();
  static_assert(lds_bytes <= 160 * 1024, "LDS of one CU");
  constexpr int waves = swiglu_waves<MAXS, G64, MR, B3>();
  if constexpr (lds_bytes > 64 * 1024) {
    static DeviceLatch attr_done;
    if (int rc = lds_optin(attr_done, (const void *)strip1_swiglu_kernel<NW, MAXS, EXACT, G64, MR, B3, waves>)) return rc;
  }
  hipLaunchKernelGGL((strip1_swiglu_kernel<NW, MAXS, EXACT, G64, MR, B3, waves>), dim3(n_strips, 1), dim3(NW * 64), lds_bytes, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// the forms of one (NW, MAXS) pair, as launch_e of strip1.hip picks them
template <int NW, int MAXS>
struct SwigluForms {
  static int launch(const Strip1Params &p, int n_strips, hipStream_t stream) {
    const bool exact = NW * MAXS == p.T;
    if (p.bits3) {  // 3-bit layers: batch 1, 64- and 128-wide groups, rounds of up to 32 k-steps
      if constexpr (MAXS <= 32) {
        if (p.group64) return exact ? launch_t<NW, MAXS, true, true, 1, true>(p, n_strips, stream) : launch_t<NW, MAXS, false, true, 1, true>(p, n_strips, stream);
        return exact ? launch_t<NW, MAXS, true, false, 1, true>(p, n_strips, stream) : launch_t<NW, MAXS, false, false, 1, true>(p, n_strips, stream);
      } else {
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: 3-bit layers on the batch-1 kernel stop at K = 16384");
      }
    }
    if (p.M > 1) {  // batches 2..4: the four-row forms, 128-wide groups, rounds of up to 32 k-steps
      if constexpr (MAXS <= 32)
        return exact ? launch_t<NW, MAXS, true, false, 4>(p, n_strips, stream) : launch_t<NW, MAXS, false, false, 4>(p, n_strips, stream);
      else
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: four batch rows on the batch-1 kernel stop at K = 16384");
    }
    if (p.group64) {  // 64-wide groups: rounds of up to 48 k-steps
      if constexpr (MAXS <= 48)
        return exact ? launch_t<NW, MAXS, true, true>(p, n_strips, stream) : launch_t<NW, MAXS, false, true>(p, n_strips, stream);
      else
        return set_error(QLLM_ERR_UNSUPPORTED, "internal: 64-wide groups on the batch-1 kernel stop at K = 24576");
    }
    return exact ? launch_t<NW, MAXS, true>(p, n_strips, stream) : launch_t<NW, MAXS, false>(p, n_strips, stream);
  }
};

// every (NW, MAXS) pair of launch_strip1's table (strip1.hip)
#define QLLM_SWIGLU_PAIRS(X) \
  X(4, 8) X(4, 16) X(4, 32) X(8, 16) X(7, 16) X(8, 24) X(8, 32) X(16, 16) X(16, 24) X(15, 24) X(16, 32) X(16, 40) X(16, 48) X(16, 56) X(16, 64)

int launch_strip1_swiglu(const Strip1Params &p, int nw, int maxs, int n_strips, hipStream_t stream) {
#define X(NW, MAXS) \
  if (nw == NW && maxs == MAXS) return SwigluForms<NW, MAXS>::launch(p, n_strips, stream);
  QLLM_SWIGLU_PAIRS(X)
#undef X
  return set_error(QLLM_ERR_UNSUPPORTED, "fused SwiGLU: no batch-1 instantiation for nw=%d round=%d", nw, maxs);
}

}  // namespace qllm
