  // The body of attn_decode_kernel and of attn_decode_ring_kernel (attn_decode_kernel.hpp includes it into both): in scope are the
  // kernel's argument `p` and the compile-time BF16, D, G, WIN and RING.
  constexpr int LPP = D / 8, GPW = 64 / LPP, TILE = 4 * GPW * kU;
  constexpr int ROW = D + 2, PROW = D + 4;  // m, l, acc[D] of one query head in LDS; m, l, two pads, acc[D] in the workspace (16-byte pieces)
  __shared__ float red[4 * G * ROW + 1];
  int &s_ticket = *(int *)(red + 4 * G * ROW);  // (one LDS object: the ticket lives behind the waves' rows)
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, grp = lane / LPP, sub = lane % LPP;
  const int split = blockIdx.x, kvh = blockIdx.y, b = blockIdx.z;
  const int S = gridDim.x;

  int64_t len = p.kv_len_dev ? *p.kv_len_dev : p.kv_len;
  if constexpr (RING) len = len < 0 ? 0 : len;  // the total of a ring: no upper end
  else len = len < 0 ? 0 : len > p.max_len ? p.max_len : len;
  const bool append = p.k_new != nullptr && (RING || len < p.max_len);
  // Ring: `len` tokens were counted before the call, the query at len (+ 1 with an append) - 1 sees the v <= W positions from lo on, and
  // position lo + r lives in slot (lo + r) mod C (C = p.max_len slots).  From here on the block works on r = 0 .. v - 1 as the linear
  // kernel works on positions 0 .. n - 1 -- n, app_pos, beg, end, the splits and the mask's columns are all relative to lo -- and only a
  // cache address turns r into its slot: slot0 + r, minus C once (r < W <= C).  ONE 64-bit modulo per block, wave-uniform.
  int64_t ring_v = 0, slot0 = 0;
  if constexpr (RING) {
    const int64_t total = len + (append ? 1 : 0), lo = total > p.window ? total - p.window : 0;
    ring_v = total - lo;
    slot0 = (int64_t)((uint64_t)lo % (uint64_t)p.max_len);
  }
  const int64_t n = RING ? ring_v : len + (append ? 1 : 0), app_pos = append ? (RING ? ring_v - 1 : len) : -1;  // n <= max_len positions count
  // the splits that hold a position the query sees.  Every block knows them, so a block outside them leaves at once -- it has nothing to
  // hand over, and the arrival counter counts the live blocks only -- except that with no position at all split 0 stores the zeros.
  // Without a window: the `live` splits that hold a position < n.  With one (WIN) the query at n - 1 sees positions lo .. n - 1 only:
  // the splits from `first`, the one that holds lo, on; that one starts its walk at lo.
  int64_t beg = (int64_t)split * p.chunk;
  const int64_t end = beg + p.chunk < n ? beg + p.chunk : n;
  int first = 0, live = (int)((n + p.chunk - 1) / p.chunk);
  if constexpr (WIN) {
    const int64_t lo = n > p.window ? n - p.window : 0;
    first = (int)(lo / p.chunk);
    live -= first;
    if ((split < first || split >= first + live) && (split > 0 || live > 0)) return;
    beg = beg > lo ? beg : lo;
  } else {
    if (split >= live && (split > 0 || live > 0)) return;
  }

  const uint4_t *kc = (const uint4_t *)p.k_cache + ((int64_t)b * p.c_batch + (int64_t)kvh * p.c_head) / 8 + sub;
  const uint4_t *vc = (const uint4_t *)p.v_cache + ((int64_t)b * p.c_batch + (int64_t)kvh * p.c_head) / 8 + sub;
  const int64_t cpos = p.c_pos / 8;

  if (beg < end) {
    float qf[G][8], acc[G][8], m[G], l[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      const uint4_t qv = *((const uint4_t *)p.q + ((int64_t)b * p.q_row + (int64_t)(kvh * G + g) * p.q_head) / 8 + sub);
      ad_unpack<BF16>(qv, qf[g]);
      m[g] = kNoMax;
      l[g] = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[g][e] = 0.f;
    }
    const uint4_t *kn = p.k_new ? (const uint4_t *)p.k_new + ((int64_t)b * p.kn_row + (int64_t)kvh * p.kn_head) / 8 + sub : nullptr;
    const uint4_t *vn = p.v_new ? (const uint4_t *)p.v_new + ((int64_t)b * p.vn_row + (int64_t)kvh * p.vn_head) / 8 + sub : nullptr;
    const uint8_t *mask8 = (const uint8_t *)p.mask + (int64_t)b * p.mask_batch;
    const uint16_t *mask16 = (const uint16_t *)p.mask + (int64_t)b * p.mask_batch;

    // one tile: K and V rows of this lane's kU positions (zeros where there is none) and what the mask adds to their scores: 0, a finite
    // value, or -inf (hidden, or no such position)
    auto load_tile = [&](int64_t base, uint4_t (&kk)[kU], uint4_t (&vv)[kU], float (&bias)[kU]) {
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int64_t pos = base + (u * 4 + wave) * GPW + grp;
        kk[u] = vv[u] = uint4_t{0u, 0u, 0u, 0u};
        bias[u] = -INFINITY;
        if (pos < end) {
          int64_t slot = pos;
          if constexpr (RING) {
            slot += slot0;
            slot -= slot >= p.max_len ? p.max_len : 0;
          }
          if (pos == app_pos) {
            kk[u] = *kn;
            vv[u] = *vn;
            *((uint4_t *)kc + slot * cpos) = kk[u];
            *((uint4_t *)vc + slot * cpos) = vv[u];
          } else {
            kk[u] = kc[slot * cpos];
            vv[u] = vc[slot * cpos];
          }
          bias[u] = 0.f;
          if (p.mask_kind == 1) {
            if (!mask8[pos]) bias[u] = -INFINITY;
          } else if (p.mask_kind == 2) {
            const uint32_t raw = mask16[pos];
            const float a = BF16 ? __builtin_bit_cast(float, raw << 16) : (float)__builtin_bit_cast(half_t, (uint16_t)raw);
            bias[u] = a <= (BF16 ? -3.3895313892515355e38f : -65504.f) ? -INFINITY : a;
          }
        }
      }
    };
    uint4_t kk[kU], vv[kU], nk[kU], nv[kU];
    float bias[kU], nbias[kU];
    load_tile(beg, kk, vv, bias);
    for (int64_t base = beg; base < end; base += TILE) {
      load_tile(base + TILE, nk, nv, nbias);  // the next tile is on its way while this one is computed (nothing is loaded past `end`)
      float s[kU][G];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float kf[8];
        ad_unpack<BF16>(kk[u], kf);
#pragma unroll
        for (int g = 0; g < G; ++g) {
          float d = 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) d = __builtin_fmaf(qf[g][e], kf[e], d);
          s[u][g] = (p.scaling * ad_group_sum<LPP>(d) + bias[u]) * kLog2e;
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
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        float vf[8];
        ad_unpack<BF16>(vv[u], vf);
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[g][e] = __builtin_fmaf(pw[u][g], vf[e], acc[g][e]);
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) kk[u] = nk[u], vv[u] = nv[u], bias[u] = nbias[u];
    }
    // the lane groups of the wave: xor shuffles (both partners compute the same bits), then lane group 0 holds the wave's state
#pragma unroll
    for (int g = 0; g < G; ++g) {
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
    // the hand-off of strip1_body.inc: 16-byte stores, drained by every wave; one lane's agent-scope release; one relaxed agent-scope
    // ticket per (batch, kv head); the last of the live blocks to arrive re-arms the counter, acquires, and combines them in split order
    // with 16-byte loads.  (One live split: its block stores directly.)
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
    // The combine, in split order: the block's threads form R sets of G * LPP owners; set r folds the r-th run of consecutive live splits
    // from left to right (kCombine splits' loads issued together, then merged one after the other), and the R results are folded in the
    // order of the runs.  The association is fixed by (live, R) alone, so the bits do not depend on which block arrives last.
    constexpr int R = G * LPP <= 64 ? 4 : 2, SET = 256 / R;
    const int r = tid / SET, t = tid % SET, cg = t / LPP, csub = t % LPP;
    const int per = (live + R - 1) / R, s_beg = first + r * per, s_end = s_beg + per < first + live ? s_beg + per : first + live;
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
