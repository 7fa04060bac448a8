// Rows into and out of the quantized KV cache (kv_quant.hpp has the format): what every route other than attn_decode_quant.hip's needs.
//
// kv_quantize: act rows [B, Hkv, S, D] (batch, head and row strides: the [B, S, H, D] view the projections produce is read in place) ->
// codes and params of positions pos0 .. pos0 + S - 1, pos0 a host integer or an int64 in device memory.  A thread owns 8 consecutive
// elements of one row (one 16-byte load), a DPP quad one group of 32: max (and min) over the quad in two quad_perm steps, the codes in
// one 8- or 4-byte store per thread, the params in one or two 2-byte stores by the quad's leader.  Rows whose position would lie outside
// 0 .. max_len - 1 (only possible with pos0 on the device) are not written.
// kv_dequantize: positions 0 .. n - 1 -> act [B, Hkv, n, D], n host or device (clamped to 0 .. max_len); a thread owns 8 elements, each
// value s * code (8 bits) or fma(code, s, z) (4 bits) in fp32, rounded once to act, one 16-byte store.  The grid covers max_len
// positions with n on the device, n on the host; threads at or beyond n leave at once.
// Neither kernel writes outside its positions.  Plain vector stores only.
#include "kv_quant.hpp"

namespace qllm {

namespace {

template <bool BF16, int D, int BITS>
__global__ __launch_bounds__(256) void kv_quantize_kernel(const KvQuantParams p) {
  constexpr int LPP = D / 8, CW = BITS / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, row = t / LPP;
  const int sub = (int)(t % LPP);
  if (row >= (int64_t)p.batch * p.kv_heads * p.rows) return;  // (a quad lies inside one row: it leaves or stays as one)
  const int64_t s = row % p.rows, h = row / p.rows % p.kv_heads, b = row / p.rows / p.kv_heads;
  const int64_t pos0 = p.count_dev ? *p.count_dev : p.count, pos = pos0 + s;
  if (pos0 < 0 || pos >= p.max_len) return;
  const uint4_t raw = *((const uint4_t *)p.src + (b * p.s_batch + h * p.s_head + s * p.s_row) / 8 + sub);
  float x[8];
  const uint32_t w[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) x[2 * i] = kvq_f32<BF16>(w[i] & 0xffffu), x[2 * i + 1] = kvq_f32<BF16>(w[i] >> 16);
  uint32_t codes[CW], s_raw, z_raw;
  kvq_encode<BF16, BITS>(x, codes, s_raw, z_raw);
  uint8_t *crow = (uint8_t *)p.codes + b * p.c_batch + h * p.c_head + pos * p.c_pos + sub * (4 * CW);
  if constexpr (BITS == 8) *(uint2_t *)crow = uint2_t{codes[0], codes[1]};
  else *(uint32_t *)crow = codes[0];
  if ((sub & 3) == 0) {
    uint16_t *prow = (uint16_t *)p.params + b * p.p_batch + h * p.p_head + pos * p.p_pos + sub / 4;
    prow[0] = (uint16_t)s_raw;
    if constexpr (BITS == 4) prow[D / 32] = (uint16_t)z_raw;
  }
}

template <bool BF16, int D, int BITS>
__global__ __launch_bounds__(256) void kv_dequantize_kernel(const KvQuantParams p, int64_t cover) {
  constexpr int LPP = D / 8, CW = BITS / 4;
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x, row = t / LPP;
  const int sub = (int)(t % LPP);
  int64_t n = p.count_dev ? *p.count_dev : p.count;
  n = n < 0 ? 0 : n > p.max_len ? p.max_len : n;
  if (row >= (int64_t)p.batch * p.kv_heads * cover) return;
  const int64_t pos = row % cover, h = row / cover % p.kv_heads, b = row / cover / p.kv_heads;
  if (pos >= n) return;
  const uint8_t *crow = (const uint8_t *)p.codes + b * p.c_batch + h * p.c_head + pos * p.c_pos + sub * (4 * CW);
  const uint16_t *prow = (const uint16_t *)p.params + b * p.p_batch + h * p.p_head + pos * p.p_pos + sub / 4;
  uint32_t codes[CW];
  if constexpr (BITS == 8) {
    const uint2_t c = *(const uint2_t *)crow;
    codes[0] = c.x, codes[1] = c.y;
  } else {
    codes[0] = *(const uint32_t *)crow;
  }
  *((uint4_t *)p.dst + (b * p.s_batch + h * p.s_head + pos * p.s_row) / 8 + sub) = kvq_decode<BF16, BITS>(codes, prow[0], BITS == 4 ? prow[D / 32] : 0u);
}

template <bool QUANT, bool BF16, int D>
int launch_kvq(const KvQuantParams &p, int bits, int64_t cover, hipStream_t stream) {
  const int64_t threads = (int64_t)p.batch * p.kv_heads * cover * (D / 8);
  if (threads == 0) return QLLM_OK;
  const dim3 grid((unsigned)((threads + 255) / 256));
  if constexpr (QUANT) {
    if (bits == 8) hipLaunchKernelGGL((kv_quantize_kernel<BF16, D, 8>), grid, dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((kv_quantize_kernel<BF16, D, 4>), grid, dim3(256), 0, stream, p);
  } else {
    if (bits == 8) hipLaunchKernelGGL((kv_dequantize_kernel<BF16, D, 8>), grid, dim3(256), 0, stream, p, cover);
    else hipLaunchKernelGGL((kv_dequantize_kernel<BF16, D, 4>), grid, dim3(256), 0, stream, p, cover);
  }
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

template <bool QUANT>
int launch_kvq_d(const KvQuantParams &p, int head_dim, int bits, int act_bf16, int64_t cover, hipStream_t stream) {
  if (head_dim == 128) return act_bf16 ? launch_kvq<QUANT, true, 128>(p, bits, cover, stream) : launch_kvq<QUANT, false, 128>(p, bits, cover, stream);
  return act_bf16 ? launch_kvq<QUANT, true, 64>(p, bits, cover, stream) : launch_kvq<QUANT, false, 64>(p, bits, cover, stream);
}

}  // namespace

// shapes, strides and alignment checked by the entries (capi.hip)
int launch_kv_quantize(const KvQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream) {
  return launch_kvq_d<true>(p, head_dim, bits, act_bf16, p.rows, stream);
}
int launch_kv_dequantize(const KvQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream) {
  return launch_kvq_d<false>(p, head_dim, bits, act_bf16, p.count_dev ? p.max_len : p.count, stream);
}

}  // namespace qllm
