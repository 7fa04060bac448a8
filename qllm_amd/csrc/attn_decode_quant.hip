// attn_decode.hip's call -- out = softmax(scaling * q K^T + mask) V for ONE query token per sequence over the first kv_len positions, the
// new token appended in the same launch -- against a QUANTIZED cache: 8- or 4-bit codes with one scale (and at 4 bits one zero) per group
// of 32 elements (kv_quant.hpp has the format).  The cache is read in place; no row is ever dequantised into memory.
//
// The frame is attn_decode.hip's: a block owns one (batch entry, kv head, split of the positions) and all G = 1..8 query heads; D / 8
// lanes share a position and each owns 8 consecutive elements, so the tile, the splits and the workspace are attn_decode_geom's; rows go
// straight into registers (8 bits: 8 bytes of K codes and 8 of V per lane and position, 4 bits: 4 and 4), the next tile's loads are in
// flight while this one is computed; fp32 scores, an fp32 online softmax in the log2 domain, one rounding at the store; the lane groups
// merge by xor shuffles, the waves through LDS, the splits through the workspace where the last block to arrive combines them in split
// order (the text of that part is attn_decode_body.inc's, without the window and the ring).  The grid never depends on the length.
//
// What is new: the dequantisation never happens per element.  A lane's 8 elements lie in ONE group (4 lanes = one DPP quad = one group),
// so with c the codes as fp32 (exact), s / z the group's scale and zero:
//   q . k  over the lane's elements = s * sum(q_e * c_e) + z * sum(q_e)       the integer-valued partial dot, ONE multiply by s per
//                                                                            (lane, position, head), ONE fma with the lane's sum(q_e),
//                                                                            which is computed once per block and head; then the DPP
//                                                                            sum over the position's lanes
//   acc_e += p * (s * c_e + z)     = acc_e += (p * s) * c_e  per element,     ONE multiply p * s per (lane, position, head),
//                                    zacc  += p * z          per lane,       ONE extra accumulator per (lane, head), rescaled with acc
//                                                                            and added to the lane's 8 acc elements after the walk
// A position costs one conversion per element and one FMA per element and head, plus two (8 bits) or four (4 bits) scalar-like
// operations per (lane, head).  The params of a group are loaded once: each lane of the quad fetches ONE of them (K scale, K zero, V
// scale, V zero: one 2-byte load per position and lane, one register), and the other lanes read it by a quad_perm DPP at the point of use.
//
// Append.  The lane group that owns position kv_len reads the new rows from k_new / v_new, quantises them by the format's formulas
// (kvq_encode: max / min over the quad by DPP), stores codes and params with plain vector stores, and attends over the codes and params
// it has just formed: the DEQUANTISED new row, what every later step will see at that position.  With the length on the device and
// kv_len + 1 > L_max nothing is stored and the first L_max positions are attended.
//
// Not built: a quantized ring / sliding layer, per-channel K quantisation, fp8, int8 MFMA on the codes (two or more query rows over codes: attn_chunk_quant.hip, attn_prefill_quant.hip), a full-precision residual
// window, head_dim other than 64 / 128.
#include "attn_decode_kernel.hpp"
#include "kv_quant.hpp"

namespace qllm {

namespace {

template <int BITS>
struct QTile {  // one tile as loaded: kU positions of this lane
  uint32_t kc[kU][BITS / 4], vc[kU][BITS / 4];  // codes
  uint32_t pr[kU];                              // act bits: ONE of the group's params per lane of the quad, by the lane's role
  float bias[kU];
};

template <bool BF16, int D, int G, int BITS>
__global__ __launch_bounds__(256) void attn_decode_quant_kernel(const AttnDecodeQuantParams p) {
  constexpr int LPP = D / 8, GPW = 64 / LPP, TILE = 4 * GPW * kU, CW = BITS / 4;
  constexpr int ROW = D + 2, PROW = D + 4;  // as attn_decode_body.inc's
  __shared__ float red[4 * G * ROW + 1];
  int &s_ticket = *(int *)(red + 4 * G * ROW);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / LPP, sub = lane % LPP;
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int S = gridDim.x;

  int64_t len = p.kv_len_dev ? *p.kv_len_dev : p.kv_len;
  len = len < 0 ? 0 : len > p.max_len ? p.max_len : len;
  const bool append = p.k_new != nullptr && len < p.max_len;
  const int64_t n = len + (append ? 1 : 0), app_pos = append ? len : -1;
  const int64_t beg = (int64_t)split * p.chunk;
  const int64_t end = beg + p.chunk < n ? beg + p.chunk : n;
  const int live = (int)((n + p.chunk - 1) / p.chunk);
  if (split >= live && (split > 0 || live > 0)) return;

  // The roles of a quad's lanes: lane 0 holds the K scale of the quad's group; at 8 bits lane 1 the V scale (lanes 2 and 3 nothing), at
  // 4 bits lane 1 the K zero, lane 2 the V scale, lane 3 the V zero.  ONE 2-byte load per position fetches them all, each once.
  const int role = sub & 3;
  constexpr int kRoleVs = BITS == 4 ? 2 : 1, kRoleKz = BITS == 4 ? 1 : -1, kRoleVz = BITS == 4 ? 3 : -1;
  const bool has_param = BITS == 4 || role < 2;
  uint8_t *kcb = (uint8_t *)p.k_codes + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head + sub * (4 * CW);
  uint8_t *vcb = (uint8_t *)p.v_codes + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head + sub * (4 * CW);
  uint16_t *prb = (uint16_t *)(role < kRoleVs ? p.k_params : p.v_params) + (int64_t)b * p.p_batch + (int64_t)kvh * p.p_head + sub / 4 +
                  (role == kRoleKz || role == kRoleVz ? D / 32 : 0);

  if (beg < end) {
    float qf[G][8], qsum[G], acc[G][8], zacc[G], m[G], l[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint4_t qv = *((const uint4_t *)p.q + ((int64_t)b * p.q_row + (int64_t)(kvh * G + g) * p.q_head) / 8 + sub);
      ad_unpack<BF16>(qv, qf[g]);
      m[g] = kNoMax;
      l[g] = zacc[g] = qsum[g] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] = 0.f, qsum[g] += qf[g][e];
    }
    const uint4_t *kn = p.k_new ? (const uint4_t *)p.k_new + ((int64_t)b * p.kn_row + (int64_t)kvh * p.kn_head) / 8 + sub : nullptr;
    const uint4_t *vn = p.v_new ? (const uint4_t *)p.v_new + ((int64_t)b * p.vn_row + (int64_t)kvh * p.vn_head) / 8 + sub : nullptr;
    const uint8_t *mask8 = (const uint8_t *)p.mask + (int64_t)b * p.mask_batch;
    const uint16_t *mask16 = (const uint16_t *)p.mask + (int64_t)b * p.mask_batch;

    auto load_codes = [&](const uint8_t *at, uint32_t (&c)[CW]) {
      if constexpr (BITS == 8) {
        const uint2_t w = *(const uint2_t *)at;
        c[0] = w.x, c[1] = w.y;
      } else {
        c[0] = *(const uint32_t *)at;
      }
    };
    auto store_codes = [&](uint8_t *at, const uint32_t (&c)[CW]) {
      if constexpr (BITS == 8) *(uint2_t *)at = uint2_t{c[0], c[1]};
      else *(uint32_t *)at = c[0];
    };
    // the new row: quantised, stored, and kept as the codes and params a later step will load
    auto append_row = [&](const uint4_t *src, uint8_t *cat, uint32_t (&c)[CW], uint32_t &s_raw, uint32_t &z_raw) {
      float x[8];
      ad_unpack<BF16>(*src, x);
      kvq_encode<BF16, BITS>(x, c, s_raw, z_raw);
      store_codes(cat, c);
    };
    // one tile: codes and params of this lane's kU positions (zeros where there is none) and what the mask adds to their scores
    auto load_tile = [&](int64_t base, QTile<BITS> &t) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t pos = base + (u * 4 + wave) * GPW + grp;
#pragma unroll
        for (int i = 0; i < CW; ++i) t.kc[u][i] = t.vc[u][i] = 0u;
        t.pr[u] = 0u;
        t.bias[u] = -INFINITY;
        if (pos < end) {
          if (pos == app_pos) {
            uint32_t ks, kz, vs, vz;  // (every lane of the quad forms all of them; it keeps and stores its role's)
            append_row(kn, kcb + pos * p.c_pos, t.kc[u], ks, kz);
            append_row(vn, vcb + pos * p.c_pos, t.vc[u], vs, vz);
            t.pr[u] = role == 0 ? ks : role == kRoleVs ? vs : role == kRoleKz ? kz : vz;
            if (has_param) prb[pos * p.p_pos] = (uint16_t)t.pr[u];
          } else {
            load_codes(kcb + pos * p.c_pos, t.kc[u]);
            load_codes(vcb + pos * p.c_pos, t.vc[u]);
            if (has_param) t.pr[u] = prb[pos * p.p_pos];
          }
          t.bias[u] = 0.f;
          if (p.mask_kind == 1) {
            if (!mask8[pos]) t.bias[u] = -INFINITY;
          } else if (p.mask_kind == 2) {
            const uint32_t raw = mask16[pos];
            const float a = kvq_f32<BF16>(raw);
            t.bias[u] = a <= (BF16 ? -3.3895313892515355e38f : -65504.f) ? -INFINITY : a;
          }
        }
      }
    };
    QTile<BITS> cur, nxt;
    load_tile(beg, cur);
    for (int64_t base = beg; base < end; base += TILE) {
      load_tile(base + TILE, nxt);  // the next tile is on its way while this one is computed (nothing is loaded past `end`)
      float s[kU][G];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float kf[8];
        kvq_codes_f32<BITS>(cur.kc[u], kf);
        const float ks = kvq_f32<BF16>(kvq_quad_lane<0>(cur.pr[u])), kz = BITS == 4 ? kvq_f32<BF16>(kvq_quad_lane<1>(cur.pr[u])) : 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) d = __builtin_fmaf(qf[g][e], kf[e], d);
          d *= ks;
          if constexpr (BITS == 4) d = __builtin_fmaf(kz, qsum[g], d);
          s[u][g] = (p.scaling * ad_group_sum<LPP>(d) + cur.bias[u]) * kLog2e;
        }
      }
      float pw[kU][G];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        float mx = m[g];
#pragma unroll
        for (int u = 0; u < kU; ++u) mx = fmaxf(mx, s[u][g]);
        const float alpha = ad_exp2(m[g] - mx);
        float sum = 0.f;
#pragma unroll
        for (int u = 0; u < kU; ++u) {
          pw[u][g] = ad_exp2(s[u][g] - mx);
          sum += pw[u][g];
        }
        l[g] = l[g] * alpha + sum;
        m[g] = mx;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] *= alpha;
        if constexpr (BITS == 4) zacc[g] *= alpha;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float vf[8];
        kvq_codes_f32<BITS>(cur.vc[u], vf);
        const float vs = kvq_f32<BF16>(kvq_quad_lane<kRoleVs>(cur.pr[u])), vz = BITS == 4 ? kvq_f32<BF16>(kvq_quad_lane<3>(cur.pr[u])) : 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          const float w = pw[u][g] * vs;
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[g][e] = __builtin_fmaf(w, vf[e], acc[g][e]);
          if constexpr (BITS == 4) zacc[g] = __builtin_fmaf(pw[u][g], vz, zacc[g]);
        }
      }
      cur = nxt;
    }
    // the zeros' share, once; then the lane groups of the wave by xor shuffles and lane group 0's state into LDS (attn_decode_body.inc)
#pragma unroll
    for (int g = 0; g < G; ++g) {
      if constexpr (BITS == 4) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[g][e] += zacc[g];
      }
#pragma unroll
      for (int x = LPP; x < 64; x <<= 1) {
        float a2[8];
        const float m2 = __shfl_xor(m[g], x, 64), l2 = __shfl_xor(l[g], x, 64);
#pragma unroll
        for (int e = 0; e < 8; ++e) a2[e] = __shfl_xor(acc[g][e], x, 64);
        ad_merge(m[g], l[g], acc[g], m2, l2, a2);
      }
      if (grp == 0) {
        float *row = red + (wave * G + g) * ROW;
        if (sub == 0) {
          row[0] = m[g];
          row[1] = l[g];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) row[2 + 8 * sub + e] = acc[g][e];
      }
    }
  }
  __syncthreads();

  // From here on: attn_decode_body.inc's text for a linear cache without a window (first = 0).
  // It is a RESTATEMENT, line for line (the wave merge above it too): a fix to the hand-off, the ticket or the combine has to be made in
  // both texts until a later change moves them into one shared .inc and shows the three existing objects' disassembly unchanged.
  // thread (g, sub) of the first G * LPP: chunk `sub` of query head g
  const bool owner = tid < G * LPP;
  const int g = tid / LPP;
  float M = kNoMax, L = 0.f, A[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (owner && beg < end) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float *row = red + (w * G + g) * ROW;
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = row[2 + 8 * sub + e];
      ad_merge(M, L, A, row[0], row[1], a2);
    }
  }
  if (live > 1) {
    // the hand-off: 16-byte stores, drained by every wave; one lane's agent-scope release; one relaxed agent-scope ticket per (batch, kv
    // head); the last of the live blocks to arrive re-arms the counter, acquires, and combines them in split order with 16-byte loads
    const int bh = b * gridDim.y + kvh;
    float4_t *part = (float4_t *)(p.partials + ((size_t)bh * S) * (G * PROW));
    if (owner) {
      float4_t *row = part + ((size_t)split * G + g) * (PROW / 4);
      if (sub == 0) row[0] = float4_t{M, L, 0.f, 0.f};
      row[1 + 2 * sub] = float4_t{A[0], A[1], A[2], A[3]};
      row[2 + 2 * sub] = float4_t{A[4], A[5], A[6], A[7]};
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the stores have left every wave ...
    __syncthreads();
    if (tid == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");  // ... and are visible to the device before the ticket says so
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      s_ticket = __hip_atomic_fetch_add(p.counters + bh, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    if (s_ticket != live - 1) return;
    if (tid == 0) {
      __hip_atomic_store(p.counters + bh, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the other blocks' tickets, and the stores in front of them
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __syncthreads();
    // The combine, in split order: R sets of G * LPP owners; set r folds the r-th run of consecutive live splits from left to right, and
    // the R results are folded in the order of the runs.  The association is fixed by (live, R) alone.
    constexpr int R = G * LPP <= 64 ? 4 : 2, SET = 256 / R;
    const int r = tid / SET, t = tid % SET, cg = t / LPP, csub = t % LPP;
    const int per = (live + R - 1) / R, s_beg = r * per, s_end = s_beg + per < live ? s_beg + per : live;
    M = kNoMax;
    L = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) A[e] = 0.f;
    if (t < G * LPP) {
      for (int sp0 = s_beg; sp0 < s_end; sp0 += kCombine) {
        float4_t ml[kCombine], lo[kCombine], hi[kCombine];
#pragma unroll
        for (int j = 0; j < kCombine; ++j) {
          const int sp = sp0 + j < s_end ? sp0 + j : s_end - 1;  // (past the run's last: loaded again, not merged)
          const float4_t *row = part + ((size_t)sp * G + cg) * (PROW / 4);
          ml[j] = row[0], lo[j] = row[1 + 2 * csub], hi[j] = row[2 + 2 * csub];
        }
#pragma unroll
        for (int j = 0; j < kCombine; ++j) {
          const float a2[8] = {lo[j].x, lo[j].y, lo[j].z, lo[j].w, hi[j].x, hi[j].y, hi[j].z, hi[j].w};
          if (sp0 + j < s_end) ad_merge(M, L, A, ml[j].x, ml[j].y, a2);
        }
      }
      float *row = red + (r * G + cg) * ROW;  // (the waves' rows were read two barriers ago)
      if (csub == 0) {
        row[0] = M;
        row[1] = L;
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) row[2 + 8 * csub + e] = A[e];
    }
    __syncthreads();
    if (!owner) return;
    M = kNoMax;
    L = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) A[e] = 0.f;
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
      const float *row = red + (rr * G + g) * ROW;
      float a2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a2[e] = row[2 + 8 * sub + e];
      ad_merge(M, L, A, row[0], row[1], a2);
    }
  }
  if (!owner) return;
  float o[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) o[e] = L > 0.f ? A[e] / L : 0.f;  // no visible key: zeros
  *((uint4_t *)p.out + ((int64_t)b * p.q_heads + kvh * G + g) * LPP + sub) = ad_pack<BF16>(o);
}

template <bool BF16, int D, int BITS>
int launch_q(const AttnDecodeQuantParams &p, int G, dim3 grid, hipStream_t stream) {
  switch (G) {
#define QLLM_ADQ_CASE(GG)                                                                                              \
  case GG:                                                                                                             \
    hipLaunchKernelGGL((attn_decode_quant_kernel<BF16, D, GG, BITS>), grid, dim3(256), 0, stream, p);                  \
    break;
    QLLM_ADQ_CASE(1) QLLM_ADQ_CASE(2) QLLM_ADQ_CASE(3) QLLM_ADQ_CASE(4) QLLM_ADQ_CASE(5) QLLM_ADQ_CASE(6) QLLM_ADQ_CASE(7) QLLM_ADQ_CASE(8)
#undef QLLM_ADQ_CASE
    default:
      return set_error(QLLM_ERR_UNSUPPORTED, "attn_decode_quant serves 1..%d query heads per kv head (got %d)", kAttnDecodeMaxGroup, G);
  }
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

template <bool BF16, int D>
int launch_q_bits(const AttnDecodeQuantParams &p, int bits, int G, dim3 grid, hipStream_t stream) {
  return bits == 8 ? launch_q<BF16, D, 8>(p, G, grid, stream) : launch_q<BF16, D, 4>(p, G, grid, stream);
}

}  // namespace

// shapes, bits, strides and alignment checked by the entry (capi.hip); p.splits / p.chunk from attn_decode_geom
int launch_attn_decode_quant(const AttnDecodeQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream) {
  const dim3 grid((unsigned)p.splits, (unsigned)p.kv_heads, (unsigned)p.batch);
  const int G = p.q_heads / p.kv_heads;
  if (head_dim == 128) return act_bf16 ? launch_q_bits<true, 128>(p, bits, G, grid, stream) : launch_q_bits<false, 128>(p, bits, G, grid, stream);
  return act_bf16 ? launch_q_bits<true, 64>(p, bits, G, grid, stream) : launch_q_bits<false, 64>(p, bits, G, grid, stream);
}

}  // namespace qllm
