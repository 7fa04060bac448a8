  // The body of attn_chunk_kernel (attn_chunk_kernel.hpp) and of attn_chunk_quant_kernel (attn_chunk_quant.hip): in scope are the kernel's
  // argument `p` (an AttnChunkParams, or the AttnChunkQuantParams that extends it), the compile-time BF16, D and MK, and QBITS: 0 for a
  // cache of act rows, 8 / 4 for one of codes (kv_quant.hpp).  Everything but the tile staging is this one text.
  constexpr int CT = kAttnChunkKvTile;  // keys per block step
  constexpr int LROW = D + 8;           // elements per LDS row: 16 bytes of padding
  constexpr int CPR = D / 8;            // 16-byte chunks per row
  constexpr int NCH = CT * CPR / 256;   // chunks of K (and of V) per thread and tile
  constexpr int KSTEPS = D / 16, DB = D / 32;
  constexpr int kChunkCombine = 4;      // splits whose partial rows the combining block loads at a time
  constexpr int PROW = D + 4;           // floats per row in the workspace: m, l, two pads, O[D] (16-byte pieces)
  __shared__ __attribute__((aligned(16))) uint16_t sK[CT * LROW];
  __shared__ __attribute__((aligned(16))) uint16_t sV[CT * LROW];
  __shared__ int s_ticket;

  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, h = lane >> 5;
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int S = p.q_len, G = p.q_heads / p.kv_heads, R = G * S, NT = (R + 31) >> 5;

  int64_t len = p.kv_len_dev ? *p.kv_len_dev : p.kv_len;
  len = len < S ? S : len > p.max_len ? p.max_len : len;
  const int64_t q_start = len - S;
  // the splits that hold a position below the length (the last row sees every one of them, causal or not): every block knows them, so
  // a block beyond them leaves at once and the arrival counter counts the live blocks only.  len >= S >= 2: there is always one.
  const int live = (int)((len + p.chunk - 1) / p.chunk);
  if (split >= live) return;
  const int64_t beg = (int64_t)split * p.chunk;
  const int64_t end = beg + p.chunk < len ? beg + p.chunk : len;
  const int t0 = (int)(beg / CT), t1 = (int)((end + CT - 1) / CT);  // the split's key tiles (the chunk is a multiple of the tile)

  // the row space of the kv head, token-major: r = i * G + g is token i of query head kvh * G + g, so the causal limit is monotone in r
  const int r = 32 * wave + (lane & 31);
  const bool computes = wave < NT, row_ok = r < R;
  const int i = row_ok ? r / G : S - 1, g = row_ok ? r - i * G : 0;  // (a lane without a row: the last token's mask row, zeros for q)
  const int hq = kvh * G + g;
  const int wlast = (32 * wave + 31 < R ? 32 * wave + 31 : R - 1) / G;              // the last token of the wave's rows
  const int64_t wkend = computes ? (p.causal ? q_start + wlast + 1 : len) : 0;  // the keys the wave computes on: <= len

  // Q as the B operand: lane (r, h) holds Q[row r][16 * step + 8h .. + 7], for the whole walk
  uint4_t qf[KSTEPS];
  {
    const uint16_t *qp = (const uint16_t *)p.q + (int64_t)b * p.q_batch + (int64_t)hq * p.q_head + (int64_t)i * p.q_row + 8 * h;
#pragma unroll
    for (int s = 0; s < KSTEPS; ++s) qf[s] = computes && row_ok ? *(const uint4_t *)(qp + 16 * s) : uint4_t{0u, 0u, 0u, 0u};
  }

  // Tile staging, the one part with two forms: the registers of the tile in flight, load_tile(t) into them (positions >= len are never
  // loaded) and store_tile() as [key][LROW] act rows in LDS (zeros at positions >= len).  QBITS == 0: act rows, 16-byte chunks.
  // Otherwise codes and params travel, and chunk_quant_store dequantises them on their way into LDS (attn_chunk_quant.hip).
  constexpr int QB = QBITS == 4 ? 4 : 8;  // (the width the quantized form's registers are declared with; they do not exist at QBITS == 0)
  const uint16_t *kc = (const uint16_t *)p.k_cache + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head;
  const uint16_t *vc = (const uint16_t *)p.v_cache + (int64_t)b * p.c_batch + (int64_t)kvh * p.c_head;
  uint4_t kreg[NCH], vreg[NCH];
  [[maybe_unused]] uint32_t kq[NCH][QB / 4], vq[NCH][QB / 4], pq[NCH];
  auto load_tile = [&](int t) {
    if constexpr (QBITS != 0) {
      chunk_quant_load<BF16, D, QB>(p, b, kvh, tid, t, len, kq, vq, pq);
    } else {
#pragma unroll
      for (int u = 0; u < NCH; ++u) {
        const int c = tid + 256 * u, row = c / CPR, ch = c % CPR;
        const int64_t pos = (int64_t)t * CT + row;
        kreg[u] = vreg[u] = uint4_t{0u, 0u, 0u, 0u};
        if (pos < len) {
          kreg[u] = *(const uint4_t *)(kc + pos * p.c_pos + 8 * ch);
          vreg[u] = *(const uint4_t *)(vc + pos * p.c_pos + 8 * ch);
        }
      }
    }
  };
  auto store_tile = [&]() {
    if constexpr (QBITS != 0) {
      chunk_quant_store<BF16, D, QB>(tid, kq, vq, pq, sK, sV);
    } else {
#pragma unroll
      for (int u = 0; u < NCH; ++u) {
        const int c = tid + 256 * u, row = c / CPR, ch = c % CPR;
        *(uint4_t *)(sK + row * LROW + 8 * ch) = kreg[u];
        *(uint4_t *)(sV + row * LROW + 8 * ch) = vreg[u];
      }
    }
  };

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

  load_tile(t0);
  for (int t = t0; t < t1; ++t) {
    __syncthreads();  // every wave has read the tile before
    store_tile();
    __syncthreads();
    if (t + 1 < t1) load_tile(t + 1);
    const int64_t kbase = (int64_t)t * CT;
    if (kbase >= wkend) continue;  // wave-uniform: nothing for this wave in the tile, or a wave that only stages (the barriers are above)

    // scores: sub-block sb holds keys kbase + 32 sb + (e & 3) + 8 (e >> 2) + 4h in register e, row r on the lane
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
    const int lim = last <= kbase ? 0 : last - kbase >= CT ? CT : (int)(last - kbase);  // relative to kbase
    // every lane reads the mask at in-bounds addresses only (its own row, or the last one; a visible key, or the tile's first, which
    // lies below kv_len whenever the wave computes on the tile) and discards what it does not need: no branch per element
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

  // register e of o[db] is column d = 32 db + (e & 3) + 8 (e >> 2) + 4h of row r: four consecutive d per piece
  if (live == 1) {  // one live split: the block stores directly
    if (!computes || !row_ok) return;
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
    return;
  }

  // The hand-off of attn_decode_body.inc: per row (m, l) and the unnormalised fp32 O[D] in 16-byte stores, drained by every wave; one
  // lane's agent-scope release; one relaxed agent-scope ticket per (batch entry, kv head); the last of the live blocks to arrive re-arms
  // the counter, acquires, and combines the live splits in split order.  A row that saw no key in this split hands over m = kNoMax,
  // l = 0, O = 0: weight 0 in the combine.
  const int bh = b * p.kv_heads + kvh;
  float *part = p.partials + (size_t)bh * p.splits * R * PROW;  // [split][row][PROW]
  if (computes && row_ok) {
    float4_t *row = (float4_t *)(part + ((size_t)split * R + r) * PROW);
    if (h == 0) row[0] = float4_t{m, l, 0.f, 0.f};
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) row[1 + 8 * db + 2 * q4 + h] = float4_t{o[db][4 * q4], o[db][4 * q4 + 1], o[db][4 * q4 + 2], o[db][4 * q4 + 3]};
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

  // The combine: a thread owns 8 columns of one row at a time and folds the live splits from left to right (kChunkCombine splits'
  // loads issued together, then merged one after the other).  The association is fixed by `live` alone, so the bits do not depend on
  // which block arrives last.
  for (int item = tid; item < R * CPR; item += 256) {
    const int row = item / CPR, c = item - row * CPR;
    float M = kNoMax, L = 0.f, A[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int sp0 = 0; sp0 < live; sp0 += kChunkCombine) {
      float4_t ml[kChunkCombine], lo[kChunkCombine], hi[kChunkCombine];
#pragma unroll
      for (int j = 0; j < kChunkCombine; ++j) {
        const int sp = sp0 + j < live ? sp0 + j : live - 1;  // (past the last: loaded again, not merged)
        const float4_t *src = (const float4_t *)(part + ((size_t)sp * R + row) * PROW);
        ml[j] = src[0], lo[j] = src[1 + 2 * c], hi[j] = src[2 + 2 * c];
      }
#pragma unroll
      for (int j = 0; j < kChunkCombine; ++j) {
        if (sp0 + j >= live) continue;
        const float a2[8] = {lo[j].x, lo[j].y, lo[j].z, lo[j].w, hi[j].x, hi[j].y, hi[j].z, hi[j].w};
        const float m2 = fmaxf(M, ml[j].x), f = __builtin_amdgcn_exp2f(M - m2), f2 = __builtin_amdgcn_exp2f(ml[j].x - m2);
        L = L * f + ml[j].y * f2;
#pragma unroll
        for (int e = 0; e < 8; ++e) A[e] = A[e] * f + a2[e] * f2;
        M = m2;
      }
    }
    uint32_t w[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) w[e] = L > 0.f ? ap_pack2<BF16>(A[2 * e] / L, A[2 * e + 1] / L) : 0u;  // no visible key anywhere: zeros
    const int ti = row / G, tg = row - ti * G;
    *(uint4_t *)((uint16_t *)p.out + (((int64_t)b * S + ti) * p.q_heads + kvh * G + tg) * D + 8 * c) = uint4_t{w[0], w[1], w[2], w[3]};
  }
