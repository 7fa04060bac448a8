// bitgemv_ao: the bit-stream matvec (bitgemv.hip) with the act-order gather inside its staging pass -- y = x[:, perm] . dequant(w) for a
// PLAIN row-stream layer w and a permutation of its K rows.  An act-order GPTQ layer is such a pair: sorting its rows by group
// (perm = argsort(g_idx)) leaves contiguous groups, and the activations have to follow.  The 3- and 4-bit
// kernels get them from a separate qllm_gather_columns launch; at these widths a whole decode matvec runs 10-18 us and a launch costs
// 2.4-3, and the kernel stages x through LDS itself anyway -- so the gather lives in that pass: a thread's 16 perm entries are four
// 16-byte loads, its activations 16 two-byte loads from an x that sits in L2 (<= 16 K 2 bytes).  Everything after the staging pass is
// bitgemv_kernel's (bitgemv_kernel.hpp, GATHER): the result is bit-identical to the plain kernel on a gathered copy of x.
#include "bitgemv_kernel.hpp"

namespace qllm {
namespace bg {

template <int BITS, int MT>
__global__ __launch_bounds__(kNW * 64) void bitgemv_ao_kernel(const BitGemvParams p, const int32_t *__restrict__ perm) {
  bitgemv_body<BITS, MT, true>(p, perm, blockIdx.x);
}

template <int BITS>
static int launch_ao(const BitGemvParams &p, const int32_t *perm, int mt, int grid, size_t lds, hipStream_t stream) {
#define QLLM_BG(MT_)                                                                                              \
  {                                                                                                               \
    static DeviceLatch attr_done; /* per (kernel, device): the LDS opt-in is a per-device attribute */              \
    if (int rc = lds_optin(attr_done, (const void *)bitgemv_ao_kernel<BITS, MT_>)) return rc;                      \
    hipLaunchKernelGGL((bitgemv_ao_kernel<BITS, MT_>), dim3(grid), dim3(kNW * 64), lds, stream, p, perm);         \
  }                                                                                                               \
  break
  switch (mt) {
    case 1: QLLM_BG(1);
    case 2: QLLM_BG(2);
    case 4: QLLM_BG(4);
    case 8: QLLM_BG(8);
    default: QLLM_BG(16);
  }
#undef QLLM_BG
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace bg

int launch_bitgemv_permuted(const BitGemvParams &p_in, const int32_t *perm, int bits, hipStream_t stream) {
  BitGemvParams p = p_in;
  const bg::Geometry g = bg::geometry(p);
  switch (bits) {
    case 2: return bg::launch_ao<2>(p, perm, g.mt, g.grid, g.lds, stream);
    case 3: return bg::launch_ao<3>(p, perm, g.mt, g.grid, g.lds, stream);
    case 4: return bg::launch_ao<4>(p, perm, g.mt, g.grid, g.lds, stream);
    case 5: return bg::launch_ao<5>(p, perm, g.mt, g.grid, g.lds, stream);
    case 6: return bg::launch_ao<6>(p, perm, g.mt, g.grid, g.lds, stream);
    case 7: return bg::launch_ao<7>(p, perm, g.mt, g.grid, g.lds, stream);
    case 8: return bg::launch_ao<8>(p, perm, g.mt, g.grid, g.lds, stream);
  }
  return set_error(QLLM_ERR_UNSUPPORTED, "bitgemv: bits must be 2..8 (got %d)", bits);
}

}  // namespace qllm
