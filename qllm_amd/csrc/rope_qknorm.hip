// q_out = rope(q_norm(q)), k_out = rope(k_norm(k)): the per-head RMSNorm of Qwen3's attention (a Qwen3RMSNorm over head_dim between the
// projection and the rotary embedding, for q and for k) and the rotary embedding of both tensors as ONE kernel -- eager runs about eight
// elementwise kernels per norm and ten for the rotary expression.  Per (token, head), over the D elements of the head:
//   rstd = rsqrt(mean(x^2) + eps)   squares, sum and rstd in fp32 (an fp16 / bf16 square is exact in fp32)
//   h = round(x * rstd),  y = round(w * h)                              rmsnorm.hip's two roundings (norm_chunk)
//   out = round(round(y * c) + round(r * s)),  r = -y2 | y1             rope.hip's three (rope_chunk)
// every rounding in the activation type, none skipped: the result is bit for bit ops.rope(ops.rmsnorm(q), ops.rmsnorm(k)).
//
// Work split.  A work item is one (token, head) of q or of k, numbered as rope.hip numbers them (q's heads, then k's, token by token); its
// T = D / 16 lanes are consecutive and aligned in a wave (8 lanes at D = 128, 4 at D = 64: 8 or 16 heads per wave).  Lane t owns the 16-byte
// chunk t of the head's first half and the chunk T + t -- the pairing the rotary needs -- of x, of the weight, of cos and of sin: two
// 16-byte loads of each, all eight issued before the first use, nothing read twice; both outputs are formed and stored from registers, so
// an output may BE its input (no other lane reads what this one writes, and the head's sum of squares is complete in every lane before the
// first store).  No LDS, no workspace, no scratch.
//
// Reduction order: rmsnorm_kernel<256, 1>'s on a row of D elements.  That kernel sums each chunk's eight squares in element order
// (sumsq_chunk) and runs an xor butterfly over the wave whose lanes >= 2 T hold zeros: a balanced binary tree over the chunk sums
// c_0 .. c_{2T-1} in index order, then zeros added to a non-negative sum, which changes nothing.  Here lane t holds c_t and c_{T+t}; the
// first-half sums and the second-half sums are reduced separately over the head's T lanes -- xor 1 and xor 2 as quad_perm, xor 4 as
// row_half_mirror (behind the first two steps the four lanes of a quad hold one value, so lane 7 - t holds what lane t ^ 4 holds) -- and
// the two halves are added last: the same tree, its two subtrees side by side in one lane.  DPP moves only, no ds_bpermute; every lane of
// the head ends with the same bits (fp32 addition commutes).
//
// The T lanes of a head enter and leave the grid-stride loop together: the work index advances by gridDim.x * 256, a multiple of T, and
// `total` is a multiple of T, so i < total holds for all lanes of a head or for none -- the DPP moves never read a lane that has left.
//
// Resources (gfx950, hipcc -O3): profiles/rope_qknorm.md.
#include "rope_kernel.hpp"
#include "strip1_kernel.hpp"

namespace qllm {

// the sum of v over the T (4 or 8) consecutive, aligned lanes of a head, in butterfly order, in every one of them
template <int T>
__device__ __forceinline__ float head_sum(float v) {
  static_assert(T == 4 || T == 8, "a head is a quad or a half row of lanes");
  v = dpp_add1<0xB1>(v);   // quad_perm [1,0,3,2]
  v = dpp_add1<0x4E>(v);   // quad_perm [2,3,0,1]
  if constexpr (T == 8) v = dpp_add1<0x141>(v);  // row_half_mirror
  return v;
}

// strides in 16-byte chunks; total = rows * (q_heads + k_heads) * T threads' worth of work
template <bool BF16, int D>
__global__ __launch_bounds__(256) void rope_qknorm_kernel(const uint4_t *q, const uint4_t *k, const uint4_t *cos, const uint4_t *sin, uint4_t *q_out,
                                                          uint4_t *k_out, const uint4_t *q_weight, const uint4_t *k_weight, float eps, uint32_t q_heads,
                                                          uint32_t k_heads, int64_t q_row, int64_t q_head, int64_t k_row, int64_t k_head, uint32_t cos_rows,
                                                          uint64_t total) {
  constexpr uint32_t T = D / 16;
  static_assert(256 % T == 0, "a head's lanes share a block, a wave and the loop's trip count");
  const uint32_t heads = q_heads + k_heads;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t item = i / T, row = item / heads;
    const uint32_t t = (uint32_t)(i % T), h = (uint32_t)(item - row * heads);
    const bool is_q = h < q_heads;
    const uint32_t hh = is_q ? h : h - q_heads;
    const uint4_t *in = is_q ? q + (int64_t)row * q_row + (int64_t)hh * q_head : k + (int64_t)row * k_row + (int64_t)hh * k_head;
    const uint4_t *w = is_q ? q_weight : k_weight;
    uint4_t *out = (is_q ? q_out + (row * q_heads + hh) * (2 * (uint64_t)T) : k_out + (row * k_heads + hh) * (2 * (uint64_t)T));
    const uint64_t cs = (row % cos_rows) * (2 * (uint64_t)T);
    const uint4_t x1 = in[t], x2 = in[T + t];
    const uint4_t w1 = w[t], w2 = w[T + t];
    const uint4_t c1 = cos[cs + t], c2 = cos[cs + T + t], s1 = sin[cs + t], s2 = sin[cs + T + t];
    const float lo = head_sum<T>(sumsq_chunk<BF16>(x1)), hi = head_sum<T>(sumsq_chunk<BF16>(x2));
    const float rstd = rms_rstd(lo + hi, D, eps);
    const uint4_t y1 = norm_chunk<BF16>(x1, w1, rstd), y2 = norm_chunk<BF16>(x2, w2, rstd);
    out[t] = rope_chunk<BF16, true>(y1, y2, c1, s1);
    out[T + t] = rope_chunk<BF16, false>(y2, y1, c2, s2);
  }
}

// strides in elements (multiples of 8), head_dim 64 or 128: checked by the entry (capi.hip)
int launch_rope_qknorm(const void *q, const void *k, const void *cos, const void *sin, void *q_out, void *k_out, const void *q_weight, const void *k_weight,
                       float eps, int rows, int q_heads, int k_heads, int head_dim, int64_t q_row_stride, int64_t q_head_stride, int64_t k_row_stride,
                       int64_t k_head_stride, int cos_rows, int act_bf16, hipStream_t stream) {
  const uint64_t total = (uint64_t)rows * (uint64_t)(q_heads + k_heads) * (uint64_t)(head_dim / 16);
  const uint64_t want = (total + 255) / 256, cap = (uint64_t)compute_units() * 8;
  const dim3 grid((unsigned)(want < cap ? want : cap));
  auto kernel = head_dim == 128 ? (act_bf16 ? rope_qknorm_kernel<true, 128> : rope_qknorm_kernel<false, 128>)
                                : (act_bf16 ? rope_qknorm_kernel<true, 64> : rope_qknorm_kernel<false, 64>);
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (const uint4_t *)q, (const uint4_t *)k, (const uint4_t *)cos, (const uint4_t *)sin, (uint4_t *)q_out,
                     (uint4_t *)k_out, (const uint4_t *)q_weight, (const uint4_t *)k_weight, eps, (uint32_t)q_heads, (uint32_t)k_heads, q_row_stride / 8,
                     q_head_stride / 8, k_row_stride / 8, k_head_stride / 8, (uint32_t)cos_rows, total);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
