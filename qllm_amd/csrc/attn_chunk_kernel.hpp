// The kernel of attn_chunk.hip (the text there says what it computes) and its launcher.  The MFMA frame is attn_prefill_kernel.hpp's
// (its helpers ap_mfma / ap_round / ap_pack2 and its constants are used as they stand); the rows a block holds, the split over the keys
// and the hand-off are this kernel's own.  The body is attn_chunk_body.inc, the text attn_chunk_quant.hip builds its kernel from too.
#pragma once
#include "attn_prefill_kernel.hpp"

namespace qllm {

namespace {

// the quantized form of the body's tile staging (attn_chunk_quant.hip defines and uses it; here the body only names it, in a branch that
// is discarded)
template <bool BF16, int D, int QB, class P, int NCH>
__device__ void chunk_quant_load(const P &p, int b, int kvh, int tid, int t, int64_t len, uint32_t (&kq)[NCH][QB / 4], uint32_t (&vq)[NCH][QB / 4],
                                 uint32_t (&pq)[NCH]);
template <bool BF16, int D, int QB, int NCH>
__device__ void chunk_quant_store(int tid, const uint32_t (&kq)[NCH][QB / 4], const uint32_t (&vq)[NCH][QB / 4], const uint32_t (&pq)[NCH], uint16_t *sK,
                                  uint16_t *sV);

// Two blocks per compute unit wherever attn_prefill_kernel has them (everywhere but head_dim 128 with an additive mask).
template <bool BF16, int D, int MK>  // MK: the mask kind
__global__ __launch_bounds__(256, (D == 128 && MK == 2) ? 1 : 2) void attn_chunk_kernel(const AttnChunkParams p) {
  constexpr int QBITS = 0;  // act rows
#include "attn_chunk_body.inc"
}

// shapes, strides and alignment checked by the entry (capi.hip); p.splits / p.chunk from attn_chunk_geom
int launch_attn_chunk_kernels(const AttnChunkParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  const dim3 grid((unsigned)p.splits, (unsigned)p.kv_heads, (unsigned)p.batch);
#define QLLM_AC_LAUNCH(BF, DD)                                                                                  \
  switch (p.mask_kind) {                                                                                      \
    case 0: hipLaunchKernelGGL((attn_chunk_kernel<BF, DD, 0>), grid, dim3(256), 0, stream, p); break;         \
    case 1: hipLaunchKernelGGL((attn_chunk_kernel<BF, DD, 1>), grid, dim3(256), 0, stream, p); break;         \
    default: hipLaunchKernelGGL((attn_chunk_kernel<BF, DD, 2>), grid, dim3(256), 0, stream, p); break;        \
  }
  if (head_dim == 128) {
    if (act_bf16) { QLLM_AC_LAUNCH(true, 128) } else { QLLM_AC_LAUNCH(false, 128) }
  } else {
    if (act_bf16) { QLLM_AC_LAUNCH(true, 64) } else { QLLM_AC_LAUNCH(false, 64) }
  }
#undef QLLM_AC_LAUNCH
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace

}  // namespace qllm
