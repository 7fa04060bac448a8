// How a 64-key tile of a QUANTIZED cache (kv_quant.hpp has the format) reaches LDS as [key][D + 8] act rows: the staging of
// attn_chunk_quant.hip and attn_prefill_quant.hip, written once.  attn_chunk_quant.hip's head says why it has this form (ownership, one
// param load per run and the quad_perm DPP, what is in flight, the arithmetic of the store).
#pragma once
#include "attn_prefill_kernel.hpp"
#include "kv_quant.hpp"

namespace qllm {

namespace {

// codes and one param per run of tile t into registers; a run at a position >= len: zeros, nothing loaded.  P: launch parameters with
// k_cache / v_cache (the codes; c_batch / c_head / c_pos in bytes) and k_params / v_params (p_batch / p_head / p_pos in elements)
template <bool BF16, int D, int QB, class P, int NCH>
__device__ __forceinline__ void chunk_quant_load(const P &p, int b, int kvh, int tid, int t, int64_t len, uint32_t (&kq)[NCH][QB / 4],
                                                 uint32_t (&vq)[NCH][QB / 4], uint32_t (&pq)[NCH]) {
  constexpr int CPR = D / 8, CW = QB / 4;
  const int role = tid & 3;  // the lane's place in its quad (256 and D / 8 are multiples of 4: the same for all its runs)
  const bool of_v = QB == 4 ? role >= 2 : (role & 1) != 0, zero = QB == 4 && (role & 1) != 0;
  const uint8_t *kc = (const uint8_t *)p.k_cache + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head;
  const uint8_t *vc = (const uint8_t *)p.v_cache + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head;
  const uint16_t *pr = (const uint16_t *)(of_v ? p.v_params : p.k_params) + (int64_t)b * p.p_batch + (int64_t)kvh * p.p_head + (zero ? D / 32 : 0);
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int c = tid + 256 * u, row = c / CPR, ch = c % CPR;
    const int64_t pos = (int64_t)t * kAttnChunkKvTile + row;
#pragma unroll
    for (int i = 0; i < CW; ++i) kq[u][i] = vq[u][i] = 0u;
    pq[u] = 0u;
    if (pos < len) {
      if constexpr (QB == 8) {
        const uint2_t k2 = *(const uint2_t *)(kc + pos * p.c_pos + 8 * ch), v2 = *(const uint2_t *)(vc + pos * p.c_pos + 8 * ch);
        kq[u][0] = k2.x, kq[u][1] = k2.y, vq[u][0] = v2.x, vq[u][1] = v2.y;
      } else {
        kq[u][0] = *(const uint32_t *)(kc + pos * p.c_pos + 4 * ch);
        vq[u][0] = *(const uint32_t *)(vc + pos * p.c_pos + 4 * ch);
      }
      pq[u] = pr[pos * p.p_pos + ch / 4];
    }
  }
}

// the runs in registers, dequantised, as the [key][D + 8] act rows of sK and sV.  Every thread of the block calls it (the quads are whole).
template <bool BF16, int D, int QB, int NCH>
__device__ __forceinline__ void chunk_quant_store(int tid, const uint32_t (&kq)[NCH][QB / 4], const uint32_t (&vq)[NCH][QB / 4], const uint32_t (&pq)[NCH],
                                                  uint16_t *sK, uint16_t *sV) {
  constexpr int CPR = D / 8, LROW = D + 8, kVs = QB == 4 ? 2 : 1;
#pragma unroll
  for (int u = 0; u < NCH; ++u) {
    const int c = tid + 256 * u, row = c / CPR, ch = c % CPR;
    const uint32_t ks = kvq_quad_lane<0>(pq[u]), vs = kvq_quad_lane<kVs>(pq[u]);
    const uint32_t kz = QB == 4 ? kvq_quad_lane<1>(pq[u]) : 0u, vz = QB == 4 ? kvq_quad_lane<3>(pq[u]) : 0u;
    *(uint4_t *)(sK + row * LROW + 8 * ch) = kvq_decode<BF16, QB>(kq[u], ks, kz);
    *(uint4_t *)(sV + row * LROW + 8 * ch) = kvq_decode<BF16, QB>(vq[u], vs, vz);
  }
}

}  // namespace

}  // namespace qllm
