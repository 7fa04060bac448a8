// The kernel of attn_prefill.hip (the text there says what it computes) and its launcher.  Two units instantiate it: attn_prefill.hip
// without the sliding window (WIN = false: that instantiation contains no window code and never reads p.window),
// attn_prefill_window.hip with it.
#pragma once
#include "kernels.hpp"

namespace qllm {

namespace {

constexpr int QT = kAttnPrefillQTile, KT = kAttnPrefillKvTile;
constexpr float kLog2e = 1.4426950408889634f;
constexpr float kNoMax = -1e30f;  // the running maximum before any visible key: finite, so that exp2(m - m) never sees inf - inf

typedef float f32x16_t __attribute__((ext_vector_type(16)));
typedef __bf16 ap_bf16x8_t __attribute__((ext_vector_type(8)));
typedef short ap_short4_t __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) ap_short4_t lds_short4_t;

template <bool BF16>
__device__ __forceinline__ f32x16_t ap_mfma(uint4_t a, uint4_t b, f32x16_t c) {
  if constexpr (BF16) return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(ap_bf16x8_t, a), __builtin_bit_cast(ap_bf16x8_t, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), c, 0, 0, 0);
}
template <bool BF16>
__device__ __forceinline__ uint32_t ap_round(float f) {  // one value of the activation type, RNE
  if constexpr (BF16) return __builtin_bit_cast(uint16_t, (__bf16)f);
  else return __builtin_bit_cast(uint16_t, (half_t)f);
}
template <bool BF16>
__device__ __forceinline__ uint32_t ap_pack2(float lo, float hi) { return ap_round<BF16>(lo) | (ap_round<BF16>(hi) << 16); }

// Two blocks per compute unit (at most 256 registers) wherever that leaves no scratch: everywhere but head_dim 128 with an additive mask.
// WIN: the sliding-window variant (p.window >= 1, causal); every use of the window stands under `if constexpr (WIN)`.
template <bool BF16, int D, int MK, bool WIN>  // MK: the mask kind
__global__ __launch_bounds__(256, (D == 128 && MK == 2) ? 1 : 2) void attn_prefill_kernel(const AttnPrefillParams p) {
  constexpr int LROW = D + 8;        // elements per LDS row: 16 bytes of padding
  constexpr int CPR = D / 8;         // 16-byte chunks per row
  constexpr int NCH = KT * CPR / 256;  // chunks of K (and of V) per thread and tile
  constexpr int KSTEPS = D / 16, DB = D / 32;
  __shared__ __attribute__((aligned(16))) uint16_t sK[KT * LROW];
  __shared__ __attribute__((aligned(16))) uint16_t sV[KT * LROW];

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
  const int qt = (int)(gridDim.x - 1 - blockIdx.x), hq = blockIdx.y, b = blockIdx.z;
  const int kvh = hq / (p.q_heads / p.kv_heads);
  const int S = p.q_len;

  int64_t len = p.kv_len_dev ? *p.kv_len_dev : p.kv_len;
  len = len < S ? S : len > p.max_len ? p.max_len : len;
  const int64_t q_start = len - S;
  const int i0 = qt * QT;                        // the block's first query row
  const int wi0 = i0 + 32 * wave, i = wi0 + r;   // the wave's first row; this lane's row
  const bool row_ok = i < S;
  const int blast = (i0 + QT < S ? i0 + QT : S) - 1;      // the block's last row (i0 < S always)
  const int wlast = wi0 + 31 < S - 1 ? wi0 + 31 : S - 1;  // the wave's last row (below wi0 when the wave has none)
  const int64_t kend = p.causal ? q_start + blast + 1 : len;  // the keys the block reads: <= len
  const int ntiles = (int)((kend + KT - 1) / KT);
  const int64_t wkend = wi0 < S ? (p.causal ? q_start + wlast + 1 : len) : 0;  // the keys the wave computes on
  // the window's lower end, the mirror of kend / wkend: the first tile that holds a key the block's first row sees, and the first key the
  // wave's first row sees (later rows see no earlier one)
  int tfirst = 0;
  int64_t wklo = 0;
  if constexpr (WIN) {
    const int64_t blo = q_start + i0 - p.window + 1;
    tfirst = blo > 0 ? (int)(blo / KT) : 0;
    wklo = q_start + wi0 - p.window + 1;
  }

  // Q as the B operand: lane (r, h) holds Q[row r][16 * step + 8h .. + 7]
  uint4_t qf[KSTEPS];
  {
    const uint16_t *qp = (const uint16_t *)p.q + (int64_t)b * p.q_batch + (int64_t)hq * p.q_head + (int64_t)i * p.q_row + 8 * h;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) qf[s] = row_ok ? *(const uint4_t *)(qp + 16 * s) : uint4_t{0u, 0u, 0u, 0u};
  }

  const uint16_t *kc = (const uint16_t *)p.k_cache + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head;
  const uint16_t *vc = (const uint16_t *)p.v_cache + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head;
  uint4_t kreg[NCH], vreg[NCH];
  auto load_tile = [&](int t) {
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int c = tid + 256 * u, row = c / CPR, ch = c % CPR;
      const int64_t pos = (int64_t)t * KT + row;
      kreg[u] = vreg[u] = uint4_t{0u, 0u, 0u, 0u};
      if (pos < len) {
        kreg[u] = *(const uint4_t *)(kc + pos * p.c_pos + 8 * ch);
        vreg[u] = *(const uint4_t *)(vc + pos * p.c_pos + 8 * ch);
      }
    }
  };
  auto store_tile = [&]() {
#pragma unroll
    for (int u = 0; u < NCH; ++u) {
      const int c = tid + 256 * u, row = c / CPR, ch = c % CPR;
      *(uint4_t *)(sK + row * LROW + 8 * ch) = kreg[u];
      *(uint4_t *)(sV + row * LROW + 8 * ch) = vreg[u];
    }
  };

  f32x16_t o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) o[db][e] = 0.f;
  float m = kNoMax, l = 0.f;

  const int64_t mask_off = (int64_t)b * p.mask_batch + (int64_t)(row_ok ? i : S - 1) * p.mask_row;  // (a lane without a row reads the last one's)
  const uint8_t *mrow8 = (const uint8_t *)p.mask + mask_off;
  const uint16_t *mrow16 = (const uint16_t *)p.mask + mask_off;
  // the transposed V read of this lane: row q = (lane & 15) >> 2 of a 4-key block, columns 16 * ((lane >> 4) & 1) + 4 * (lane & 3) ..
  const int vt_off = (4 * h + ((lane & 15) >> 2)) * LROW + 16 * ((lane >> 4) & 1) + 4 * (lane & 3);

  if (tfirst < ntiles) load_tile(tfirst);
  for (int t = tfirst; t < ntiles; ++t) {
    __syncthreads();  // every wave has read the tile before
    store_tile();
    __syncthreads();
    if (t + 1 < ntiles) load_tile(t + 1);
    const int64_t kbase = (int64_t)t * KT;
    if (kbase >= wkend) continue;  // wave-uniform: nothing for this wave in the tile (the barriers above are outside)
    if constexpr (WIN)
      if (kbase + KT <= wklo) continue;  // nor here: the tile lies wholly below the window of the wave's first row

    // scores: sub-block sb holds keys kbase + 32 sb + (e & 3) + 8 (e >> 2) + 4h in register e, query row i on the lane
    f32x16_t sc[2];
    bool live[2];
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      live[sb] = kbase + 32 * sb < wkend;
      if constexpr (WIN) live[sb] = live[sb] && kbase + 32 * sb + 32 > wklo;
#pragma unroll
      for (int e = 0; e < 16; ++e) sc[sb][e] = 0.f;
      if (live[sb]) {
#pragma unroll
        for (int s = 0; s < KSTEPS; ++s) {
          const uint4_t kf = *(const uint4_t *)(sK + (32 * sb + r) * LROW + 16 * s + 8 * h);
          sc[sb] = ap_mfma<BF16>(kf, qf[s], sc[sb]);
        }
      }
    }
    // the keys of this tile that row i sees lie below `lim` (relative to kbase): the length, and the diagonal of a causal call
    const int64_t last = p.causal && q_start + i + 1 < len ? q_start + i + 1 : len;
    const int lim = !row_ok || last <= kbase ? 0 : last - kbase >= KT ? KT : (int)(last - kbase);
    // ... and, with a window, at or above `low`: the first key of the window of row i
    int low = 0;
    if constexpr (WIN) {
      // row 0's, wave-uniform and clamped to INT32_MIN .. KT (below: hidden by nothing, whatever i; KT: every key of the tile hidden),
      // so that adding i stays in 32 bits
      const int64_t row0 = q_start - p.window + 1 - kbase;
      const int r0 = row0 <= INT32_MIN ? INT32_MIN : row0 >= KT ? KT : (int)row0;
      const int first = r0 >= KT ? KT : r0 + i;
      low = first <= 0 ? 0 : first >= KT ? KT : first;
    }
    // every lane reads the mask at in-bounds addresses only (its own row, or the last one; a visible key, or the tile's first, which
    // lies below kv_len whenever the wave computes on the tile) and discards what it does not need: no branch per element
    float mx = m;
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int j = 32 * sb + (e & 3) + 8 * (e >> 2) + 4 * h;  // relative to kbase
        bool vis = live[sb] && j < lim;
        if constexpr (WIN) vis = vis && j >= low;
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
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the other 16 keys of each sub-block are on lane ^ 32: one maximum per query row
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

    // O^T += V^T P^T: the A operand's element j of lane half h is V[key 16 s + 8 (j >> 2) + 4h + (j & 3)][d = 32 db + r]
#pragma unroll
    for (int sb = 0; sb < 2; ++sb) {
      if (!live[sb]) continue;
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
  // register e of o[db] is column d = 32 db + (e & 3) + 8 (e >> 2) + 4h of query row i: four consecutive d per 8-byte store
  uint16_t *op = (uint16_t *)p.out + (((int64_t)b * S + i) * p.q_heads + hq) * D + 4 * h;
#pragma unroll
  for (int db = 0; db < DB; ++db) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float v[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = l > 0.f ? o[db][4 * g + e] / l : 0.f;  // no visible key: zeros
      *(uint2_t *)(op + 32 * db + 8 * g) = uint2_t{ap_pack2<BF16>(v[0], v[1]), ap_pack2<BF16>(v[2], v[3])};
    }
  }
}

// shapes, strides and alignment checked by the entry (capi.hip)
template <bool WIN>
int launch_attn_prefill_variant(const AttnPrefillParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  const dim3 grid((unsigned)((p.q_len + QT - 1) / QT), (unsigned)p.q_heads, (unsigned)p.batch);
#define QLLM_AP_LAUNCH(BF, DD)                                                                                          \
  switch (p.mask_kind) {                                                                                              \
    case 0: hipLaunchKernelGGL((attn_prefill_kernel<BF, DD, 0, WIN>), grid, dim3(256), 0, stream, p); break;          \
    case 1: hipLaunchKernelGGL((attn_prefill_kernel<BF, DD, 1, WIN>), grid, dim3(256), 0, stream, p); break;          \
    default: hipLaunchKernelGGL((attn_prefill_kernel<BF, DD, 2, WIN>), grid, dim3(256), 0, stream, p); break;         \
  }
  if (head_dim == 128) {
    if (act_bf16) { QLLM_AP_LAUNCH(true, 128) } else { QLLM_AP_LAUNCH(false, 128) }
  } else {
    if (act_bf16) { QLLM_AP_LAUNCH(true, 64) } else { QLLM_AP_LAUNCH(false, 64) }
  }
#undef QLLM_AP_LAUNCH
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace

}  // namespace qllm
