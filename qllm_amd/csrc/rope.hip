// q_out = q * cos + rotate_half(q) * sin, k_out likewise: the rotary position embedding of the Llama family (rotate_half(x) =
// cat(-x2, x1) of the two halves of a head) for BOTH tensors as ONE kernel -- the eager expression is neg, cat, mul, mul, add per tensor,
// ten kernels.  The arithmetic is the eager expression's, rounding for rounding, in the activation type:
//   a = round(x * c), b = round(r * s), out = round(float(a) + float(b)),  r = -x2 for the first half of a head and x1 for the second
// (three roundings, no FMA: the library is built with -ffp-contract=off; the negation is applied to the element, as eager does, so signed
// zeros come out as eager's).
//
// A work item is one (row, head) of q or of k; a thread owns one 16-byte chunk (eight elements) of the head's first half and the chunk
// D/2 further on: two loads of the input, two of cos, two of sin, two stores.  It forms both outputs from registers, so an output may BE
// its input (same strides): no other thread reads what it writes.  Threads are numbered chunk by chunk, head by head (q's heads, then
// k's), row by row: neighbouring threads read neighbouring 16 bytes.  The grid is sized from the thread count and capped at eight blocks
// per compute unit, with a grid-stride loop behind it; every offset is 64 bits wide.  No LDS.
#include "kernels.hpp"

namespace qllm {

template <bool BF16>
__device__ __forceinline__ float rope_f32(uint32_t bits16) {
  static_assert(BF16, "fp16 elements are multiplied and added as halves");
  return __builtin_bit_cast(float, bits16 << 16);
}
// one element: round(round(x * c) + round(r * s)) with r = -other (NEG: the first half of the head) or other.  fp16: native half
// arithmetic -- a half product is the fp32 product rounded once, and a half sum of two halves is their fp32 sum rounded once (24 >= 2 * 11 +
// 2 bits: the double rounding is innocuous).  Spelled through float, hipcc forms round(r * s) as v_fma_mix(r, s, +0), which turns a
// product of -0 into +0: the sign of a zero result then is not eager's.  The negation flips the sign bit of the element itself.
template <bool BF16, bool NEG>
__device__ __forceinline__ uint32_t rope_elem(uint32_t x, uint32_t other, uint32_t c, uint32_t s) {
  const uint32_t r = NEG ? other ^ 0x8000u : other;
  if constexpr (BF16) {
    const float a = rope_f32<true>(f32_to_bf16(rope_f32<true>(x) * rope_f32<true>(c)));
    const float b = rope_f32<true>(f32_to_bf16(rope_f32<true>(r) * rope_f32<true>(s)));
    return f32_to_bf16(a + b);
  } else {
    const half_t a = __builtin_bit_cast(half_t, (uint16_t)x) * __builtin_bit_cast(half_t, (uint16_t)c);
    const half_t b = __builtin_bit_cast(half_t, (uint16_t)r) * __builtin_bit_cast(half_t, (uint16_t)s);
    return __builtin_bit_cast(uint16_t, (half_t)(a + b));
  }
}
template <bool BF16, bool NEG>
__device__ __forceinline__ uint32_t rope_pair(uint32_t x, uint32_t other, uint32_t c, uint32_t s) {
  return rope_elem<BF16, NEG>(x & 0xffffu, other & 0xffffu, c & 0xffffu, s & 0xffffu) |
         (rope_elem<BF16, NEG>(x >> 16, other >> 16, c >> 16, s >> 16) << 16);
}
template <bool BF16, bool NEG>
__device__ __forceinline__ uint4_t rope_chunk(uint4_t x, uint4_t other, uint4_t c, uint4_t s) {
  return uint4_t{rope_pair<BF16, NEG>(x.x, other.x, c.x, s.x), rope_pair<BF16, NEG>(x.y, other.y, c.y, s.y),
                 rope_pair<BF16, NEG>(x.z, other.z, c.z, s.z), rope_pair<BF16, NEG>(x.w, other.w, c.w, s.w)};
}

// strides in 16-byte chunks; T = head_dim / 16 chunks per half head; total = rows * (q_heads + k_heads) * T threads' worth of work
template <bool BF16>
__global__ __launch_bounds__(256) void rope_kernel(const uint4_t *q, const uint4_t *k, const uint4_t *cos, const uint4_t *sin, uint4_t *q_out, uint4_t *k_out,
                                                   uint32_t q_heads, uint32_t k_heads, uint32_t T, int64_t q_row, int64_t q_head, int64_t k_row, int64_t k_head,
                                                   uint32_t cos_rows, uint64_t total) {
  const uint32_t heads = q_heads + k_heads;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
    const uint64_t item = i / T, row = item / heads;
    const uint32_t t = (uint32_t)(i - item * T), h = (uint32_t)(item - row * heads);
    const bool is_q = h < q_heads;
    const uint32_t hh = is_q ? h : h - q_heads;
    const uint4_t *in = is_q ? q + (int64_t)row * q_row + (int64_t)hh * q_head : k + (int64_t)row * k_row + (int64_t)hh * k_head;
    uint4_t *out = (is_q ? q_out + (row * q_heads + hh) * (2 * (uint64_t)T) : k_out + (row * k_heads + hh) * (2 * (uint64_t)T));
    const uint64_t cs = (row % cos_rows) * (2 * (uint64_t)T);
    const uint4_t x1 = in[t], x2 = in[T + t];
    const uint4_t c1 = cos[cs + t], c2 = cos[cs + T + t], s1 = sin[cs + t], s2 = sin[cs + T + t];
    out[t] = rope_chunk<BF16, true>(x1, x2, c1, s1);
    out[T + t] = rope_chunk<BF16, false>(x2, x1, c2, s2);
  }
}

// strides in elements (multiples of 8), head_dim a multiple of 16: checked by the entry (capi.hip)
int launch_rope(const void *q, const void *k, const void *cos, const void *sin, void *q_out, void *k_out, int rows, int q_heads, int k_heads, int head_dim,
                int64_t q_row_stride, int64_t q_head_stride, int64_t k_row_stride, int64_t k_head_stride, int cos_rows, int act_bf16, hipStream_t stream) {
  const uint32_t T = head_dim / 16;
  const uint64_t total = (uint64_t)rows * (uint64_t)(q_heads + k_heads) * T;
  const uint64_t want = (total + 255) / 256, cap = (uint64_t)compute_units() * 8;
  const dim3 grid((unsigned)(want < cap ? want : cap));
  auto kernel = act_bf16 ? rope_kernel<true> : rope_kernel<false>;
  hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, (const uint4_t *)q, (const uint4_t *)k, (const uint4_t *)cos, (const uint4_t *)sin, (uint4_t *)q_out,
                     (uint4_t *)k_out, (uint32_t)q_heads, (uint32_t)k_heads, T, q_row_stride / 8, q_head_stride / 8, k_row_stride / 8, k_head_stride / 8,
                     (uint32_t)cos_rows, total);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
