// The quantized KV cache: its format, written once for the kernels that write it (kv_quant.hip, the append of attn_decode_quant.hip) and
// those that read it, and the launch parameters of both units.
//
// Format.  A cached row is the D = 64 / 128 elements of one (batch entry, kv head, position), cut into groups of 32 consecutive
// elements.  `act` is the activation type, x the act-type input widened to fp32, every operation IEEE fp32 (the division correctly
// rounded: hipcc's default).
//   8 bits, symmetric:   s = act(max|x| / 127);  code = clamp(rint(x / s), -127, 127) as int8, 0 where s == 0;  value = s * code
//   4 bits, asymmetric:  z = act(min x), s = act((max x - min x) / 15);  code = clamp(rint((x - z) / s), 0, 15), 0 where s == 0;
//                        value = fma(code, s, z)
// codes: uint8 [B, Hkv, L, D * bits / 8]; group g occupies bytes [4 * bits * g, 4 * bits * (g + 1)) of its row.  At 8 bits byte i is
// element i.  At 4 bits element i of the row sits in nibble i: byte i / 2, the low nibble for an even i, the high one for an odd i -- so a
// lane's run of 8 consecutive elements is one little-endian 32-bit word with element e in bits [4e, 4e + 4).
// params: act [B, Hkv, L, P]; 8 bits: P = D / 32 scales; 4 bits: P = D / 16, all scales, then all zeros.
//
// Lanes.  Everywhere a lane owns 8 consecutive elements, so the 4 lanes of a DPP quad own one group: a group's max / min is two
// quad_perm steps, and each of the group's params is loaded or stored by one lane of the quad.
#pragma once
#include "kernels.hpp"

namespace qllm {

struct AttnDecodeQuantParams {
  const void *q, *k_new, *v_new;  // k_new / v_new: both or neither (append)
  void *k_codes, *k_params, *v_codes, *v_params;
  const void *mask;               // mask_kind 0: none; 1: bool bytes; 2: additive, activation type
  void *out;
  const int64_t *kv_len_dev;      // NULL: kv_len
  int64_t kv_len, max_len;
  int64_t q_row, q_head, kn_row, kn_head, vn_row, vn_head, mask_batch;  // strides in elements
  int64_t c_batch, c_head, c_pos;  // codes, in bytes (K and V alike)
  int64_t p_batch, p_head, p_pos;  // params, in elements (K and V alike)
  int64_t chunk;                  // positions per split
  int batch, q_heads, kv_heads, mask_kind, splits;
  float scaling;
  float *partials;                // as AttnDecodeParams'
  int *counters;
};
// grid and workspace are attn_decode_geom's (a lane owns 8 elements here as there: the same tile, the same splits)
int launch_attn_decode_quant(const AttnDecodeQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream);

// attn_chunk_quant.hip: attn_chunk.hip's launch over codes.  k_cache / v_cache are the CODES and c_batch / c_head / c_pos count BYTES;
// everything else of AttnChunkParams means what it means there (grid and workspace: attn_chunk_geom's)
struct AttnChunkQuantParams : AttnChunkParams {
  const void *k_params, *v_params;
  int64_t p_batch, p_head, p_pos;  // params, in elements (K and V alike)
};
int launch_attn_chunk_quant(const AttnChunkQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream);

// attn_prefill_quant.hip: attn_prefill.hip's call without a window over codes, by a kernel of its own.  k_cache / v_cache are the CODES
// and c_batch / c_head / c_pos count BYTES; `window` is not read.  Grid: (ceil(G * q_len / kAttnPrefillQTile), kv_heads, batch)
struct AttnPrefillQuantParams : AttnPrefillParams {
  const void *k_params, *v_params;
  int64_t p_batch, p_head, p_pos;  // params, in elements (K and V alike)
};
int launch_attn_prefill_quant(const AttnPrefillQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream);

struct KvQuantParams {
  const void *src;                // quantize: act rows [B, Hkv, rows, D]
  void *codes, *params;
  void *dst;                      // dequantize: act [B, Hkv, n, D]
  const int64_t *count_dev;       // NULL: count.  quantize: pos0, the first position written; dequantize: n, the positions read
  int64_t count, max_len;         // max_len: the cache's positions (dequantize: at most what dst holds)
  int64_t s_batch, s_head, s_row;  // src or dst, in elements
  int64_t c_batch, c_head, c_pos;  // codes, in bytes
  int64_t p_batch, p_head, p_pos;  // params, in elements
  int batch, kv_heads, rows;      // rows: quantize only
};
int launch_kv_quantize(const KvQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream);
int launch_kv_dequantize(const KvQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream);

#ifdef __HIPCC__
namespace {

template <bool BF16>
__device__ __forceinline__ float kvq_f32(uint32_t raw) {  // an act value in the low 16 bits
  if constexpr (BF16) return __builtin_bit_cast(float, raw << 16);
  else return (float)__builtin_bit_cast(half_t, (uint16_t)raw);
}
template <bool BF16>
__device__ __forceinline__ uint32_t kvq_act(float f) {  // round to nearest even
  if constexpr (BF16) return f32_to_bf16(f);
  else return __builtin_bit_cast(uint16_t, (half_t)f);
}
template <int CTRL>
__device__ __forceinline__ float kvq_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// over the 4 lanes of a quad (all of them active); every one of them gets it
__device__ __forceinline__ float kvq_quad_max(float v) {
  v = fmaxf(v, kvq_dpp<0xB1>(v));  // quad_perm [1,0,3,2]
  return fmaxf(v, kvq_dpp<0x4E>(v));  // quad_perm [2,3,0,1]
}
__device__ __forceinline__ float kvq_quad_min(float v) {
  v = fminf(v, kvq_dpp<0xB1>(v));
  return fminf(v, kvq_dpp<0x4E>(v));
}
// the value of lane I of the quad in all 4 lanes
template <int I>
__device__ __forceinline__ uint32_t kvq_quad_lane(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, I * 0x55, 0xF, 0xF, true);  // quad_perm [I,I,I,I]
}

// The lane's 8 elements x of a group whose other 24 the quad's other lanes hold -> its codes (BITS / 4 words) and the group's scale and
// zero as act bits (the zero 0 at 8 bits); the same s and z in all 4 lanes.
template <bool BF16, int BITS>
__device__ __forceinline__ void kvq_encode(const float (&x)[8], uint32_t (&codes)[BITS / 4], uint32_t &s_raw, uint32_t &z_raw) {
  if constexpr (BITS == 8) {
    float a = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) a = fmaxf(a, fabsf(x[e]));
    s_raw = kvq_act<BF16>(kvq_quad_max(a) / 127.0f);
    z_raw = 0u;
    const float s = kvq_f32<BF16>(s_raw);
    codes[0] = codes[1] = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float c = fminf(fmaxf(rintf(x[e] / s), -127.f), 127.f);
      const int ci = s == 0.f ? 0 : (int)c;
      codes[e / 4] |= (uint32_t)(ci & 0xff) << (8 * (e % 4));
    }
  } else {
    float lo = x[0], hi = x[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) lo = fminf(lo, x[e]), hi = fmaxf(hi, x[e]);
    lo = kvq_quad_min(lo), hi = kvq_quad_max(hi);
    z_raw = kvq_act<BF16>(lo);
    s_raw = kvq_act<BF16>((hi - lo) / 15.0f);
    const float s = kvq_f32<BF16>(s_raw), z = kvq_f32<BF16>(z_raw);
    codes[0] = 0u;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float c = fminf(fmaxf(rintf((x[e] - z) / s), 0.f), 15.f);
      const int ci = s == 0.f ? 0 : (int)c;
      codes[0] |= (uint32_t)ci << (4 * e);
    }
  }
}

// the lane's 8 codes as fp32 (exact)
template <int BITS>
__device__ __forceinline__ void kvq_codes_f32(const uint32_t (&codes)[BITS / 4], float (&c)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    if constexpr (BITS == 8) c[e] = (float)(int)(int8_t)(codes[e / 4] >> (8 * (e % 4)));
    else c[e] = (float)((codes[0] >> (4 * e)) & 15u);
  }
}

// the lane's 8 codes with their group's scale and zero (act bits) -> its 8 values, each rounded once to act: what kv_dequantize writes and
// what attn_quant_tile.hpp puts into LDS (attn_chunk_quant.hip, attn_prefill_quant.hip), one arithmetic for all
template <bool BF16, int BITS>
__device__ __forceinline__ uint4_t kvq_decode(const uint32_t (&codes)[BITS / 4], uint32_t s_raw, uint32_t z_raw) {
  const float s = kvq_f32<BF16>(s_raw), z = BITS == 4 ? kvq_f32<BF16>(z_raw) : 0.f;
  float c[8];
  kvq_codes_f32<BITS>(codes, c);
  uint32_t w[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float lo = BITS == 4 ? __builtin_fmaf(c[2 * i], s, z) : s * c[2 * i], hi = BITS == 4 ? __builtin_fmaf(c[2 * i + 1], s, z) : s * c[2 * i + 1];
    w[i] = kvq_act<BF16>(lo) | (kvq_act<BF16>(hi) << 16);
  }
  return uint4_t{w[0], w[1], w[2], w[3]};
}

}  // namespace
#endif

}  // namespace qllm
