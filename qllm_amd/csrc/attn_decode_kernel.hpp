// The kernel of attn_decode.hip (the text there says what it computes) and its launcher.  Three units instantiate it: attn_decode.hip
// without the sliding window (WIN = false: that instantiation contains no window code and never reads p.window), attn_decode_window.hip
// with it, attn_decode_ring.hip over a ring-buffer cache (RING: a kernel name of its own, attn_decode_ring_kernel; the text is there).
// The body is one text, attn_decode_body.inc, included into both kernels (the idiom of strip1_body.inc); what only the ring does sits
// behind `if constexpr (RING)`, so the other two units' kernels are the instruction streams they were before the ring existed.  (A
// __device__ function template called from both kernels would read better and was tried first: inlined into attn_decode_kernel it
// changed all 64 existing streams, the block's 64-bit division moving from the scalar to the vector unit.  profiles/attn_ring.md.)
#pragma once
#include "kernels.hpp"

namespace qllm {

namespace {

constexpr int kU = 4;          // wave loads of K (and of V) per block step
constexpr int kCombine = 8;    // splits whose partial results the combining block loads at a time
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kNoMax = -1e30f;  // the running maximum before any visible key: finite, so that exp2(m - m) never sees inf - inf

template <int CTRL>
__device__ __forceinline__ float ad_dpp_add(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// sum over the LPP (8 or 16) lanes that share a position; every one of them gets it
template <int LPP>
__device__ __forceinline__ float ad_group_sum(float v) {
  v = ad_dpp_add<0xB1>(v);   // quad_perm [1,0,3,2]
  v = ad_dpp_add<0x4E>(v);   // quad_perm [2,3,0,1]
  v = ad_dpp_add<0x141>(v);  // row_half_mirror
  if constexpr (LPP == 16) v = ad_dpp_add<0x140>(v);  // row_mirror
  return v;
}
template <bool BF16>
__device__ __forceinline__ void ad_unpack(uint4_t v, float (&f)[8]) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if constexpr (BF16) {
      f[2 * i] = __builtin_bit_cast(float, w[i] << 16);
      f[2 * i + 1] = __builtin_bit_cast(float, w[i] & 0xffff0000u);
    } else {
      const half2_t h = __builtin_bit_cast(half2_t, w[i]);
      f[2 * i] = (float)h.x;
      f[2 * i + 1] = (float)h.y;
    }
  }
}
template <bool BF16>
__device__ __forceinline__ uint32_t ad_round(float f) {
  if constexpr (BF16) return f32_to_bf16(f);
  else return __builtin_bit_cast(uint16_t, (half_t)f);
}
template <bool BF16>
__device__ __forceinline__ uint4_t ad_pack(const float (&f)[8]) {
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) w[i] = ad_round<BF16>(f[2 * i]) | (ad_round<BF16>(f[2 * i + 1]) << 16);
  return uint4_t{w[0], w[1], w[2], w[3]};
}
__device__ __forceinline__ float ad_exp2(float x) { return __builtin_amdgcn_exp2f(x); }

// (m, l, a[8]) <- the softmax state of both key sets; symmetric in its two arguments, bit for bit
__device__ __forceinline__ void ad_merge(float &m, float &l, float (&a)[8], float m2, float l2, const float (&a2)[8]) {
  const float mx = fmaxf(m, m2), f = ad_exp2(m - mx), f2 = ad_exp2(m2 - mx);
  l = l * f + l2 * f2;
#pragma unroll
  for (int e = 0; e < 8; ++e) a[e] = a[e] * f + a2[e] * f2;
  m = mx;
}

template <bool BF16, int D, int G, bool WIN>
__global__ __launch_bounds__(256) void attn_decode_kernel(const AttnDecodeParams p) {
  constexpr bool RING = false;
#include "attn_decode_body.inc"
}
// the ring's kernels: a name of their own (attn_decode_kernel's template list is what the other units' symbols are made of)
template <bool BF16, int D, int G>
__global__ __launch_bounds__(256) void attn_decode_ring_kernel(const AttnDecodeParams p) {
  constexpr bool WIN = false, RING = true;
#include "attn_decode_body.inc"
}

template <bool BF16, int D, bool WIN, bool RING = false>
int launch_d(const AttnDecodeParams &p, int G, dim3 grid, hipStream_t stream) {
  switch (G) {
#define QLLM_AD_CASE(GG)                                                                          \
  case GG:                                                                                        \
    if constexpr (RING) hipLaunchKernelGGL((attn_decode_ring_kernel<BF16, D, GG>), grid, dim3(256), 0, stream, p); \
    else hipLaunchKernelGGL((attn_decode_kernel<BF16, D, GG, WIN>), grid, dim3(256), 0, stream, p);  \
    break;
    QLLM_AD_CASE(1) QLLM_AD_CASE(2) QLLM_AD_CASE(3) QLLM_AD_CASE(4) QLLM_AD_CASE(5) QLLM_AD_CASE(6) QLLM_AD_CASE(7) QLLM_AD_CASE(8)
#undef QLLM_AD_CASE
    default:
      return set_error(QLLM_ERR_UNSUPPORTED, "attn_decode serves 1..%d query heads per kv head (got %d)", kAttnDecodeMaxGroup, G);
  }
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// shapes, strides and alignment checked by the entry (capi.hip); p.splits / p.chunk from attn_decode_geom
template <bool WIN, bool RING = false>
int launch_attn_decode_variant(const AttnDecodeParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  const dim3 grid((unsigned)p.splits, (unsigned)p.kv_heads, (unsigned)p.batch);
  const int G = p.q_heads / p.kv_heads;
  if (head_dim == 128) return act_bf16 ? launch_d<true, 128, WIN, RING>(p, G, grid, stream) : launch_d<false, 128, WIN, RING>(p, G, grid, stream);
  return act_bf16 ? launch_d<true, 64, WIN, RING>(p, G, grid, stream) : launch_d<false, 64, WIN, RING>(p, G, grid, stream);
}

}  // namespace

}  // namespace qllm
