// What the quantizer translation units (hqq_quant.hip, gptq_quant.hip, gptq_static.hip, awq_quant.hip) share: the weight's storage types and their
// conversions, the host-side dispatch on the weight's dtype, the 16-lane min / max butterfly and the way codes leave a row tile.
// Grids differ per quantizer (find_params, grid_of / code_of) and stay with their kernels; so do HQQ's DPP reductions: a sum in another
// order changes bits, another cross-lane instruction changes speed.
#pragma once
#include "kernels.hpp"

namespace qllm {

namespace {   // (internal to each translation unit, like the kernels' other helpers: bf16_t is part of the kernels' mangled names)

// ---- storage types of W: half_t, bf16_t, float -------------------------------------------------------------------------------------------
struct bf16_t { uint16_t bits; };
__device__ __forceinline__ float to_f32(half_t v) { return (float)v; }
__device__ __forceinline__ float to_f32(bf16_t v) { return __builtin_bit_cast(float, (uint32_t)v.bits << 16); }
__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ void from_f32(half_t *d, float v) { *d = (half_t)v; }
__device__ __forceinline__ void from_f32(float *d, float v) { *d = v; }
__device__ __forceinline__ void from_f32(bf16_t *d, float v) {  // round to nearest even (v is finite)
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  d->bits = (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
// v rounded to the storage type T and back: what an in-place product leaves in a 16-bit tensor
template <typename T> __device__ __forceinline__ float round_to(float v) { T t; from_f32(&t, v); return to_f32(t); }

// f(T{}) with T the storage type behind w_dtype (the entry points have checked it): with_w_type(w_dtype, [&](auto tag) { using T = decltype(tag); ... })
template <typename F> void with_w_type(int w_dtype, F &&f) {
  if (w_dtype == QLLM_F16) f(half_t{});
  else if (w_dtype == QLLM_BF16) f(bf16_t{});
  else f(float{});
}

inline float maxq_of(int bits) { return (float)((1 << bits) - 1); }   // the largest code of a `bits`-wide grid

// ---- a row tile: 16 rows per 256-thread block, 16 lanes per row -----------------------------------------------------------------------------
// one step of the row's min / max butterfly: both against the lane m away (xor; m = 1, 2, 4, 8 leaves every lane of the row with the
// row's extremes).  A step by value with the loop at the call site: clang schedules the kernels exactly as it did the written-out loops,
// which a function around the whole loop, or one taking references, does not (profiles/quant_refactor.md).
struct MinMax { float mn, mx; };
__device__ __forceinline__ MinMax minmax_xor(MinMax v, int m) {
  return {fminf(v.mn, __shfl_xor(v.mn, m, 16)), fmaxf(v.mx, __shfl_xor(v.mx, m, 16))};
}

// the idx-th of a tile's codes, staged in LDS as s_q[column][16 rows], to codes[K][N]: the tile's columns start at k0, its rows at n0;
// 16 consecutive idx are 16 consecutive int32 along N.  The loop over idx stays with the kernel (same reason as above).
__device__ __forceinline__ void store_code(int32_t *codes, const int *s_q, int idx, int k0, int n0, int N) {
  const int c = idx >> 4, nn = n0 + (idx & 15);
  if (nn < N) codes[(size_t)(k0 + c) * N + nn] = s_q[idx];
}

}  // namespace

}  // namespace qllm
