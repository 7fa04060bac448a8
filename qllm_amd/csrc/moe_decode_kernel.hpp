// The routed experts of a mixture-of-experts block at decode (Mixtral, Qwen3-MoE): what the two kernels of moe_decode.hip share.
//
// Format: 4-bit layers with 128-wide groups in the native strip-major layout (native.hip), the layers of one kind (gate, up, down)
// stacked per expert in ONE allocation each: expert e of a [K -> N] kind lies at
//     qweight + e * (N/16) * (K/8) * 16 words,   scales + e * (N/16) * (K/128) * 16 halves,   qzeros + e * (N/16) * (K/128) * 2 words
// (qzeros NULL: the symmetric grid, zero point 8).  The expert of a slot is read from `ids` ON THE DEVICE -- int64, as torch.topk leaves
// them -- so no pointer table, no host knowledge of the routing, and a captured launch serves every routing.
//
// One group of one strip is 16 word rows x 16 columns = 1024 contiguous bytes: ONE 16-byte load per lane of a wave.  Lane (r, c) =
// (lane >> 2, lane & 3) holds word row r -- k = 8 r .. 8 r + 7 of the group -- of columns 4 c .. 4 c + 3, next to its four scales (one
// 8-byte load) and the word with its four zero points.  A word's nibbles become exact fp16 pairs (1024 + q_k, 1024 + q_{k+4}) by the
// layout's raw 0x6400 | nibble patterns; one packed add of -(1024 + z) makes them q - z, exact; v_dot2_f32_f16 multiplies the pair with
// the matching pair of x and adds in fp32.  So a lane accumulates  sum_k x_k (q_k - z)  of its 8 k for 4 columns in fp32 and folds the
// group in with one fma by the scale:  y += s * acc  -- the library's contract x . s (q - z) on the unrounded W, with NO 1024-sized
// term in any sum (the matrix-instruction kernels carry one and subtract it per group; here the vector ALU has the spare add).
//
// Why dot products on the vector ALU and not MFMA: at T <= 4 rows a block's 16 x 16 x 16 tile would hold one real row of A; what the
// batch-1 kernel gains from it is instruction count, and it pays with the LDS round trip of A fragments per k-step and with the
// 1024-offset in its sums.  These kernels run 2.6 vector instructions per weight byte pair -- 84 per lane and 1 KB group -- which at 8
// (16) waves per block stays under the time the group's bytes take to arrive ("Routed experts at decode", has the count); the
// MFMA form was not built, so this is a choice by count, not by a measured A/B.
#pragma once
#include "strip1_kernel.hpp"

namespace qllm {

// one lane's share of one group: 4 columns x 8 k, their scales, the word with their zero points
struct MoeGroup {
  uint4_t w;
  uint2_t s;
  uint32_t z;
};

// group g of strip `strip` of expert e of a [K -> N] kind; G = K / 128 groups, NS = N / 16 strips
__device__ __forceinline__ MoeGroup moe_load_group(const uint32_t *qw, const half_t *sc, const uint32_t *qz, int64_t e, int NS, int strip, int G, int g,
                                                   int lane) {
  const int64_t sg = (e * NS + strip) * (int64_t)G + g;   // (strip, group) counted over the whole stack
  MoeGroup m;
  m.w = *(const uint4_t *)(qw + sg * 256 + lane * 4);
  m.s = *(const uint2_t *)(sc + sg * 16 + (lane & 3) * 4);
  m.z = qz ? qz[sg * 2 + ((lane & 3) >> 1)] : 0x88888888u;
  return m;
}

// eight consecutive activations (one 16-byte chunk) -> the four fp16 pairs (k0,k4) (k1,k5) (k2,k6) (k3,k7) a weight word's nibbles pair up as
template <bool BF16>
__device__ __forceinline__ uint4_t moe_x_pairs(uint4_t v) {
  half8_t h;
  if constexpr (BF16) h = bf16x8_to_h8(v);
  else h = __builtin_bit_cast(half8_t, v);
  return __builtin_bit_cast(uint4_t, a_perm_04152637(h));
}

// acc[c] += s_c * sum_k x_k (q_k - z_c) over the lane's 8 k, for its 4 columns
__device__ __forceinline__ void moe_consume(const MoeGroup &m, uint4_t xp, int lane, int add_zero_bias, float acc[4]) {
  const half2_t x0 = as_h2(xp.x), x1 = as_h2(xp.y), x2 = as_h2(xp.z), x3 = as_h2(xp.w);
  const uint32_t words[4] = {m.w.x, m.w.y, m.w.z, m.w.w};
  const uint32_t zsh = (uint32_t)(lane & 1) * 16u;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const uint32_t z = ((m.z >> (zsh + 4 * c)) + (uint32_t)add_zero_bias) & 15u;
    const half2_t nz = as_h2((0xE400u | z) * 0x00010001u);   // (-(1024 + z), -(1024 + z))
    const uint32_t w = words[c];
    float a = __builtin_amdgcn_fdot2(as_h2((w & kNibLo) | kMagic) + nz, x0, 0.f, false);
    a = __builtin_amdgcn_fdot2(as_h2(((w >> 4) & kNibLo) | kMagic) + nz, x1, a, false);
    a = __builtin_amdgcn_fdot2(as_h2(((w >> 8) & kNibLo) | kMagic) + nz, x2, a, false);
    a = __builtin_amdgcn_fdot2(as_h2(((w >> 12) & kNibLo) | kMagic) + nz, x3, a, false);
    const uint32_t s2 = (c & 2) ? m.s.y : m.s.x;
    const float s = (float)__builtin_bit_cast(half_t, (uint16_t)((c & 1) ? (s2 >> 16) : (s2 & 0xffffu)));
    acc[c] = __builtin_fmaf(s, a, acc[c]);
  }
}

// the sum of v over the 16 lanes that share (lane & 3), in butterfly order, in every one of them
__device__ __forceinline__ float moe_rows_sum(float v) {
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 32);
  return v;
}

// v rounded to the activation type, as a float
template <bool BF16>
__device__ __forceinline__ float moe_round(float v) {
  if constexpr (BF16) return __builtin_bit_cast(float, (uint32_t)f32_to_bf16(v) << 16);
  else return (float)(half_t)v;
}
template <bool BF16>
__device__ __forceinline__ uint16_t moe_bits(float v) {
  if constexpr (BF16) return f32_to_bf16(v);
  else return __builtin_bit_cast(uint16_t, (half_t)v);
}

}  // namespace qllm
