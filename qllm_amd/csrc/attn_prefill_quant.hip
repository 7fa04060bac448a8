// Prefill attention -- S >= 2 query rows per sequence, any number of them -- over a QUANTIZED cache (kv_quant.hpp has the format), the
// codes read in place: what QuantStaticLayer.update + attn_prefill.hip compute, without the two kv_dequantize launches that write every
// valid position of K and of V as act rows and without attn_prefill reading them back.  The cache is never written: the caller has stored
// the S new rows (kv_quantize) and kv_len counts them.
//
// Work split.  attn_prefill_kernel gives a block 128 rows of ONE query head; over codes the G = Hq / Hkv blocks of a group would each load
// and dequantise the same K / V tile.  Here the rows of a kv head are packed token-major as in attn_chunk.hip -- packed row r = i * G + g
// is token i of query head kvh * G + g, R = G * S rows, no upper bound on R -- and a block of 4 waves x 32 rows owns 128 CONSECUTIVE
// packed rows of one (batch entry, kv head): grid (ceil(R / 128), Hkv, B), the heaviest row tiles first.  A staged tile serves all heads
// of the group inside a block, and a block spans 128 / G tokens, so the strip of its last tiles above a row's diagonal -- staged and
// masked away -- is G times narrower than under 128 tokens of one head.  (The number of blocks per kv head, G * S / 128, and so the number
// of tile loads is the same either way.)  G (1..8) need not divide 128: a block may start and end inside a token; a lane derives i = r / G,
// g = r % G once.  The causal limit kv_len - S + i is monotone in r, so attn_prefill_kernel's kend / wkend rules hold on tokens: a block
// reads key tiles up to its last row's limit, a wave skips the tiles above its last row's limit.  Rows >= R compute on zeros and are
// never stored.
//
// Tiles.  64 keys, staged by attn_quant_tile.hpp (attn_chunk_quant.hip's staging): a thread owns runs of 8 elements, a DPP quad a group
// of 32; per run one code load of K and of V (8 bytes at 8 bits, 4 at 4) and ONE 2-byte param load, by the lane's place in the quad, read
// by the other lanes with kvq_quad_lane; codes and params of tile t + 1 are in flight while tile t is computed; kvq_decode
// (kv_dequantize's arithmetic, one rounding to act) runs on the way into the [key][D + 8] LDS rows.  Positions >= kv_len are never loaded
// and decode to zeros.
//
// Arithmetic.  The prefill frame's: S^T = K Q^T and O^T = V^T P^T on mfma_f32_32x32x16, Q in registers for the whole walk (gathered per
// lane from its own token and head), V read transposed from LDS, fp32 scores, fp32 online softmax in the log2 domain, P rounded once to
// act, one rounding at the store into the contiguous [B, S, Hq, D] output.  The MFMAs consume, bit for bit, the values kv_dequantize would
// have written.
//
// No key split, no workspace, no counters, no scratch memory; plain vector loads and stores.  The launch follows the shapes alone: with the
// length on the device one captured launch serves every length.
//
// Not built: the append inside this kernel, a sliding window, quantized ring / sliding layers, fp8, int8 MFMA on the codes.
#include "attn_quant_tile.hpp"

namespace qllm {

namespace {

// blocks per compute unit as attn_prefill_kernel has them: two, but one at head_dim 128 with an additive mask
template <bool BF16, int D, int BITS, int MK>  // MK: the mask kind
__global__ __launch_bounds__(256, (D == 128 && MK == 2) ? 1 : 2) void attn_prefill_quant_kernel(const AttnPrefillQuantParams p) {
  constexpr int LROW = D + 8;          // elements per LDS row: 16 bytes of padding
  constexpr int CPR = D / 8;           // runs of 8 elements per row
  constexpr int NCH = KT * CPR / 256;  // runs of K (and of V) per thread and tile
  constexpr int KSTEPS = D / 16, DB = D / 32;
  static_assert(KT == kAttnChunkKvTile, "attn_quant_tile.hpp stages tiles of kAttnChunkKvTile keys");
  __shared__ __attribute__((aligned(16))) uint16_t sK[KT * LROW];
  __shared__ __attribute__((aligned(16))) uint16_t sV[KT * LROW];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5;
  const int rt = (int)(gridDim.x - 1 - blockIdx.x), kvh = blockIdx.y, b = blockIdx.z;
  const int S = p.q_len, G = p.q_heads / p.kv_heads, R = G * S;

  int64_t len = p.kv_len_dev ? *p.kv_len_dev : p.kv_len;
  len = len < S ? S : len > p.max_len ? p.max_len : len;
  const int64_t q_start = len - S;

  // the packed rows: the block's first, the wave's first, this lane's; its token and head (a lane without a row: the last token's mask
  // row, zeros for q)
  const int r0 = rt * QT, wr0 = r0 + 32 * wave, r = wr0 + (lane & 31);
  const bool row_ok = r < R;
  const int i = row_ok ? r / G : S - 1, g = row_ok ? r - i * G : 0;
  const int hq = kvh * G + g;
  const int blast = ((r0 + QT < R ? r0 + QT : R) - 1) / G;    // the last token of the block's rows (r0 < R always)
  const int wlast = (wr0 + 31 < R ? wr0 + 31 : R - 1) / G;    // the last token of the wave's rows
  const int64_t kend = p.causal ? q_start + blast + 1 : len;  // the keys the block reads: <= len
  const int ntiles = (int)((kend + KT - 1) / KT);
  const int64_t wkend = wr0 < R ? (p.causal ? q_start + wlast + 1 : len) : 0;  // the keys the wave computes on (none: it only stages)

  // Q as the B operand: lane (r, h) holds Q[token i, head hq][16 * step + 8h .. + 7], for the whole walk
  uint4_t qf[KSTEPS];
  {
    const uint16_t *qp = (const uint16_t *)p.q + (int64_t)b * p.q_batch + (int64_t)hq * p.q_head + (int64_t)i * p.q_row + 8 * h;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) qf[s] = row_ok ? *(const uint4_t *)(qp + 16 * s) : uint4_t{0u, 0u, 0u, 0u};
  }

  uint32_t kq[NCH][BITS / 4], vq[NCH][BITS / 4], pq[NCH];  // the tile in flight: codes and one param per run

  f32x16_t o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m = kNoMax, l = 0.f;

  const int64_t mask_off = (int64_t)b * p.mask_batch + (int64_t)i * p.mask_row;
  const uint8_t *mrow8 = (const uint8_t *)p.mask + mask_off;
  const uint16_t *mrow16 = (const uint16_t *)p.mask + mask_off;
  // the transposed V read of this lane: row q = (lane & 15) >> 2 of a 4-key block, columns 16 * ((lane >> 4) & 1) + 4 * (lane & 3) ..
  const int vt_off = (4 * h + ((lane & 15) >> 2)) * LROW + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
  // the keys row r sees lie below `last`: the length, and the diagonal of a causal call
  const int64_t last = !row_ok ? 0 : p.causal && q_start + i + 1 < len ? q_start + i + 1 : len;

  chunk_quant_load<BF16, D, BITS>(p, b, kvh, tid, 0, len, kq, vq, pq);  // (kend >= 1: there is always a tile)
  for (int t = 0; t < ntiles; ++t) {
    __syncthreads();  // every wave has read the tile before
    chunk_quant_store<BF16, D, BITS>(tid, kq, vq, pq, sK, sV);
    __syncthreads();
    if (t + 1 < ntiles) chunk_quant_load<BF16, D, BITS>(p, b, kvh, tid, t + 1, len, kq, vq, pq);
    const int64_t kbase = (int64_t)t * KT;
    if (kbase >= wkend) continue;  // wave-uniform: nothing for this wave in the tile (the barriers above are outside)

    // scores: sub-block sb holds keys kbase + 32 sb + (e & 3) + 8 (e >> 2) + 4h in register e, packed row r on the lane
    f32x16_t sc[2];
    bool on[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      on[sb] = kbase + 32 * sb < wkend;
#pragma unroll
      for (int e = 0; e < 16; ++e) sc[sb][e] = 0.f;
      if (on[sb]) {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
          const uint4_t kf = *(const uint4_t *)(sK + (32 * sb + (lane & 31)) * LROW + 16 * s + 8 * h);
          sc[sb] = ap_mfma<BF16>(kf, qf[s], sc[sb]);
        }
      }
    }
    const int lim = last <= kbase ? 0 : last - kbase >= KT ? KT : (int)(last - kbase);  // relative to kbase
    // every lane reads the mask at in-bounds addresses only (its own token's row, or the last one's; a visible key, or the tile's first,
    // which lies below kv_len whenever the wave computes on the tile) and discards what it does not need: no branch per element
    float mx = m;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = 32 * sb + (e & 3) + 8 * (e >> 2) + 4 * h;
        bool vis = on[sb] && j < lim;
        const int jc = vis ? j : 0;
        float a = 0.f;
        if constexpr (MK == 1) {
          vis = vis && mrow8[kbase + jc] != 0;
        } else if constexpr (MK == 2) {
          const uint32_t raw = mrow16[kbase + jc];
          a = BF16 ? __builtin_bit_cast(float, raw << 16) : (float)__builtin_bit_cast(half_t, (uint16_t)raw);
          vis = vis && !(a <= (BF16 ? -3.3895313892515355e38f : -65504.f));
        }
        const float s = vis ? (p.scaling * sc[sb][e] + a) * kLog2e : -INFINITY;
        sc[sb][e] = s;
        mx = fmaxf(mx, s);
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the other 16 keys of each sub-block are on lane ^ 32: one maximum per row
    const float alpha = __builtin_amdgcn_exp2f(m - mx);
    m = mx;
    float sum = 0.f;
    uint4_t pf[2][2];  // P as the B operand: [sub-block][k-step]
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      float pw[16];
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        pw[e] = __builtin_amdgcn_exp2f(sc[sb][e] - mx);
        sum += pw[e];
      }
#pragma unroll
      for (int s = 0; s < 2; ++s)
        pf[sb][s] = uint4_t{ap_pack2<BF16>(pw[8 * s], pw[8 * s + 1]), ap_pack2<BF16>(pw[8 * s + 2], pw[8 * s + 3]),
                            ap_pack2<BF16>(pw[8 * s + 4], pw[8 * s + 5]), ap_pack2<BF16>(pw[8 * s + 6], pw[8 * s + 7])};
    }
    l = l * alpha + sum;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) o[db][e] *= alpha;

    // O^T += V^T P^T: the A operand's element j of lane half h is V[key 16 s + 8 (j >> 2) + 4h + (j & 3)][d = 32 db + (lane & 31)]
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      if (!on[sb]) continue;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
#pragma unroll
        for (int db = 0; db < DB; ++db) {
          const uint16_t *base = sV + (32 * sb + 16 * s) * LROW + 32 * db + vt_off;
          const ap_short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t *)base);
          const ap_short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t *)(base + 8 * LROW));
          const uint2_t lo2 = __builtin_bit_cast(uint2_t, lo), hi2 = __builtin_bit_cast(uint2_t, hi);
          o[db] = ap_mfma<BF16>(uint4_t{lo2.x, lo2.y, hi2.x, hi2.y}, pf[sb][s], o[db]);
        }
      }
    }
  }

  l += __shfl_xor(l, 32, 64);
  if (!row_ok) return;
  // register e of o[db] is column d = 32 db + (e & 3) + 8 (e >> 2) + 4h of packed row r: four consecutive d per 8-byte store
  uint16_t *op = (uint16_t *)p.out + (((int64_t)b * S + i) * p.q_heads + hq) * D + 4 * h;
#pragma unroll
  for (int db = 0; db < DB; ++db) {
#pragma unroll
    for (int q4 = 0; q4 < 4; ++q4) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = l > 0.f ? o[db][4 * q4 + e] / l : 0.f;  // no visible key: zeros
      *(uint2_t *)(op + 32 * db + 8 * q4) = uint2_t{ap_pack2<BF16>(v[0], v[1]), ap_pack2<BF16>(v[2], v[3])};
    }
  }
}

template <bool BF16, int D, int BITS>
int launch_apq(const AttnPrefillQuantParams &p, hipStream_t stream) {
  const int64_t rows = (int64_t)(p.q_heads / p.kv_heads) * p.q_len;
  const dim3 grid((unsigned)((rows + QT - 1) / QT), (unsigned)p.kv_heads, (unsigned)p.batch);
  switch (p.mask_kind) {
    case 0: hipLaunchKernelGGL((attn_prefill_quant_kernel<BF16, D, BITS, 0>), grid, dim3(256), 0, stream, p); break;
    case 1: hipLaunchKernelGGL((attn_prefill_quant_kernel<BF16, D, BITS, 1>), grid, dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((attn_prefill_quant_kernel<BF16, D, BITS, 2>), grid, dim3(256), 0, stream, p); break;
  }
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

template <bool BF16, int D>
int launch_apq_bits(const AttnPrefillQuantParams &p, int bits, hipStream_t stream) {
  return bits == 8 ? launch_apq<BF16, D, 8>(p, stream) : launch_apq<BF16, D, 4>(p, stream);
}

}  // namespace

// shapes, bits, strides and alignment checked by the entry (capi.hip)
int launch_attn_prefill_quant(const AttnPrefillQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream) {
  if (head_dim == 128) return act_bf16 ? launch_apq_bits<true, 128>(p, bits, stream) : launch_apq_bits<false, 128>(p, bits, stream);
  return act_bf16 ? launch_apq_bits<true, 64>(p, bits, stream) : launch_apq_bits<false, 64>(p, bits, stream);
}

}  // namespace qllm
