// The rotary embedding's element arithmetic, shared by rope.hip and rope_qknorm.hip: one 16-byte chunk of a head against the chunk half a
// head away, with the eager expression's three roundings in the activation type.
#pragma once
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

}  // namespace qllm
