// The body of strip1_kernel, strip1_swiglu_kernel, strip1_norm_kernel and the two RESID kernels (strip1_kernel.hpp, which documents it):
// included inside all five, with NW, MAXS, EXACT, NCH, LVL, DBG, AR, G64, MR, B3, SWIGLU, NORM, NORM_PARK and RESID constants of the
// enclosing function and `p` its Strip1Params.
  static_assert(MAXS % 4 == 0 && MAXS >= 8 && MAXS <= 64, "rounds are whole 128-wide groups, at most 16 of them (round 6: 40 .. 64 k-steps for K up to 32768)");
  static_assert(!(G64 && AR), "the fused all-reduce form is built for 128-wide groups");
  static_assert(MR == 1 || (MR == 4 && !G64 && !AR && !DBG && LVL == 4), "four batch rows: 128-wide groups, the plain form");
  static_assert(!B3 || (MR == 1 && !AR && !DBG && LVL == 4), "3 bits: the plain batch-1 form");
  static_assert(!SWIGLU || (!AR && !DBG && LVL == 4), "act(gate) * up: the plain forms");
  static_assert(!NORM || (!SWIGLU && MR == 1 && !AR && !DBG && LVL == 4), "RMSNorm(x): the plain batch-1 forms");
  static_assert(!RESID || (!NORM && MR == 1 && !AR && !DBG && LVL == 4), "residual + y: the plain and the SWIGLU batch-1 forms");
  constexpr int KPG = G64 ? 2 : 4;        // k-steps per group
  constexpr int NG = MAXS / KPG;          // groups per wave
  constexpr int NPASS = (MAXS + 15) / 16; // accumulator sets: one per 16 k-steps (four 128-wide groups / eight 64-wide ones)
  constexpr int GPL = G64 ? 2 : 1;        // groups per lane and pass
  constexpr int XL = (MAXS * 4 + 63) / 64;  // 16-byte activation chunks per lane
  constexpr int RS = strip1_rs(NW);       // floats per column of the reduction buffer (16-byte aligned rows, 2-way banks at most)
  extern __shared__ __attribute__((aligned(16))) float lds[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int b = blockIdx.x;
  // the problem record and the header in ONE batch of scalar loads: the empty asm "uses" every word here, so hipcc cannot leave
  // any of them for a second round trip behind the surplus-block test
  const Strip1Problem pr = p.prob[blockIdx.y];
  asm volatile("" ::"s"(pr.qweight), "s"(pr.scales), "s"(pr.qzeros), "s"(pr.bias), "s"(pr.y), "s"(pr.n_strips), "s"(pr.zero_kind), "s"(p.x),
               "s"(p.T), "s"(p.n_groups), "s"(p.add_zero_bias), "s"(p.act_bf16));
  if constexpr (SWIGLU) asm volatile("" ::"s"(p.x2));  // (the up vector's base: the same batch)
  if constexpr (NORM) asm volatile("" ::"s"(p.norm_w), "s"(p.norm_eps), "s"(p.rstd_out));  // (the norm's weight, epsilon, report slot)
  if constexpr (RESID) asm volatile("" ::"s"(p.residual));  // (the residual row's base: the same batch)
  // the two flags the uniform branches and the tail read: taken from the first batch of scalar loads (as outputs of an asm they cannot
  // be re-loaded next to their use -- hipcc otherwise sinks a second s_load of each into the decode branch and in front of the y store)
  int add_zero_bias = p.add_zero_bias, act_bf16 = p.act_bf16;
  asm volatile("" : "+s"(add_zero_bias), "+s"(act_bf16));
  uint64_t *dbg_slot = nullptr;
  if constexpr (DBG) {
    if (p.dbg && wave == 0 && blockIdx.y == 0) {
      if (b == 0) dbg_slot = p.dbg;
      else if (b == (int)gridDim.x / 2) dbg_slot = p.dbg + 8;
      else if (b == (int)gridDim.x - 1) dbg_slot = p.dbg + 16;
    }
    if (dbg_slot && lane == 0) dbg_slot[0] = __builtin_amdgcn_s_memrealtime();
  }
  if (b >= pr.n_strips) return;  // (groups of layers of different widths)

  const int T = p.T;
  const int t0 = wave * MAXS;                              // the wave owns k-steps [t0, min(t0 + MAXS, T))
  const int tb = EXACT ? t0 : min(t0, T - MAXS);           // its window [tb, tb + MAXS): shifted back into the strip at the end of K
  // ---- every load of the wave, back to back: x chunk(s), one scale + one zero word per pass, MAXS weight words -----------------
  // RESID: the residual of output column 16 b + i, first of the batch (loads return in order: it has arrived before the activations).
  // Every lane issues it -- no branch in the prologue, N = 16 n_strips keeps it inside the row -- and holds it in ONE register until the
  // epilogue, where lanes 0..15 of wave 0 use theirs: no round trip behind the cross-wave sum.
  // RESID_LATE (the SWIGLU forms that sit AT their register bound with the up chunks live across the load batch -- rounds of 24 at 64
  // registers, rounds of 56 / 64 at 128: one more register there is scratch): the load is issued behind the last MFMA instead, where the
  // weight words are dead, and returns under the per-group corrections, the LDS pass and the barrier -- still not behind the sum
  constexpr bool RESID_LATE = RESID && SWIGLU && (MAXS >= 56 || (MAXS == 24 && !G64 && !B3));
  uint32_t resid = 0;
  if constexpr (RESID && !RESID_LATE) resid = ((const uint16_t *)p.residual)[b * 16 + i];
  uint4_t xa[MR][XL];
  uint4_t xb[SWIGLU ? MR : 1][(SWIGLU || NORM) ? XL : 1];   // (SWIGLU: the up vector's chunks; NORM: the norm weight's)
  bool xkeep[XL];
#pragma unroll
  for (int u = 0; u < XL; ++u) {
    const int c = lane + 64 * u;                           // 16-byte chunk of the window: k-step tb + c / 4
    const int cc = min(c, MAXS * 4 - 1);
#pragma unroll
    for (int m = 0; m < MR; ++m) {                         // (MR = 4: batch row m of x, row stride K = 32 T halves; rows past M stay zero)
      xa[m][u] = uint4_t{0, 0, 0, 0};
      if (MR == 1 || m < p.M) xa[m][u] = *(const uint4_t *)((const uint16_t *)p.x + (size_t)m * 32 * T + 32 * tb + 8 * cc);
      if constexpr (SWIGLU) {
        xb[m][u] = uint4_t{0, 0, 0, 0};
        if (MR == 1 || m < p.M) xb[m][u] = *(const uint4_t *)((const uint16_t *)p.x2 + (size_t)m * 32 * T + 32 * tb + 8 * cc);
      }
    }
    if constexpr (NORM) xb[0][u] = *(const uint4_t *)((const uint16_t *)p.norm_w + 32 * tb + 8 * cc);   // (a [K] vector: no row term)
    const int t = tb + (c >> 2);
    xkeep[u] = EXACT ? (c < MAXS * 4) : (c < MAXS * 4 && t >= t0 && t < T);
  }
  const int G0 = tb / KPG;
  const size_t grow = (size_t)b * p.n_groups + G0;         // first group row of the wave in the strip's scale / zero tables
  const int zk = pr.zero_kind;
  half_t sc[NPASS][GPL];
  uint32_t zraw[NPASS][GPL], zraw2[B3 ? NPASS : 1][GPL];  // (zraw2: packed 3-bit zero points are bit 3 i of the group row's 64-bit pair)
  uint32_t w[MAXS], wh[B3 ? MAXS : 1];
  {
    // a wave-uniform base (the wave's first group row) + a 32-bit lane offset: element (gj, i) of the [group][16] scale rows is
    // 16 gj + i; its zero point sits in dword (16 gj + i) >> 3 of the packed rows (2 dwords per group), >> 1 of the fp16 rows (8).
    // A symmetric layer has no table: the host points qzeros at the scales (a valid dword, never decoded)
    const char *sbase = (const char *)(pr.scales + grow * 16);
    const int zmul = (zk == ZK_PACKED) ? 2 : 8;          // dwords per group row
    const char *zb = (const char *)((const uint32_t *)pr.qzeros + grow * zmul);
    const uint32_t zsh = (zk == ZK_PACKED) ? 3u : 1u, pair = (B3 && zk == ZK_PACKED) ? 1u : 0u;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
      for (int h = 0; h < GPL; ++h) {
        // the lane's group(s) of the pass: 4 ps + g (128-wide), 8 ps + 2 g + h (64-wide)
        const uint32_t gj = (uint32_t)min((G64 ? 8 * ps + 2 * g + h : 4 * ps + g), NG - 1);  // (lanes past the last group re-read it; their sums of x are zero)
        const uint32_t e = gj * 16 + (uint32_t)i;
        sc[ps][h] = *(const half_t *)(sbase + e * 2);
        if constexpr (B3) {                              // packed: both words of the pair; fp16 / symmetric: the one dword twice
          zraw[ps][h] = *(const uint32_t *)(zb + ((e >> zsh) & ~pair) * 4);
          zraw2[ps][h] = *(const uint32_t *)(zb + ((e >> zsh) | pair) * 4);
        } else {
          zraw[ps][h] = *(const uint32_t *)(zb + (e >> zsh) * 4);
        }
      }
  }
  if constexpr (B3) {
    // the strip is [3 T word rows][16]: k-step t = rows 3 t .. 3 t + 2; the lane's 24-bit field straddles rows {0,0,1,2}[g] / {0,1,2,2}[g]
    const uint32_t *wl3 = pr.qweight + ((size_t)b * T + tb) * 48 + i;
    const int lo_off = (g == 0 ? 0 : g - 1) * 16, hi_off = (g == 3 ? 2 : g) * 16;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) {
      w[s] = __builtin_nontemporal_load(wl3 + s * 48 + lo_off);
      wh[s] = __builtin_nontemporal_load(wl3 + s * 48 + hi_off);
    }
  } else {
    const uint32_t *wl = pr.qweight + ((size_t)b * T + tb) * 64 + lane;
#pragma unroll
    for (int s = 0; s < MAXS; ++s) w[s] = __builtin_nontemporal_load(wl + s * 64);
  }
  __builtin_amdgcn_sched_barrier(0);
  if constexpr (DBG) {
    if (dbg_slot && lane == 0) dbg_slot[1] = __builtin_amdgcn_s_memrealtime();
  }

  // wave-private LDS: staged activations (XL KB: chunk c at 16 c) and 256 zero bytes
  char *wbase = (char *)lds + 16 * MR * RS * 4 + wave * (MR * XL * 1024 + 256);   // (MR = 4: batch row m's chunks at + m XL KB)
  char *zeros = wbase + MR * XL * 1024;
  uint32_t fold = 0;  // (LVL < 4: keeps the loaded values alive)

  // ---- activations -> LDS (needs only the OLDEST loads; the weights stay in flight) ---------------------------------------------
  float sx[MR][XL], sxp[MR][XL], sx2[XL], sxp2[XL];  // (sx2 / sxp2: the lane's second group of the pass, 64-wide groups only)
  if constexpr (LVL >= 2) {
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int u = 0; u < XL; ++u) asm volatile("" : "+v"(xa[m][u]));  // (pins the staging below the weight loads: strip_kernel.hpp)
    *(uint32_t *)(zeros + 4 * lane) = 0u;
    if constexpr (SWIGLU) {
      // act(gate) * up in the activation type, in place of the gate chunk (one wave-uniform branch per launch, like the conversion
      // below); rows past M are silu(0) * 0 = 0.
      // PARK (the forms whose twins sit next to their register bound: four batch rows with two chunks each, rounds of 24 at 64 registers,
      // rounds of 64): the up chunks are live from the load batch on, next to the gate chunks and every weight word -- once they have
      // arrived they wait in the chunk's OWN slot of the wave's staging area (the slot its product is written to below: same lane, same
      // address, one wave's LDS operations stay in order) and come back one chunk at a time.  No more LDS than the twin's.
      constexpr bool PARK = (MR * XL >= 8) || MAXS >= 64 || (MAXS == 24 && MR == 1 && !G64 && !B3);
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int u = 0; u < XL; ++u) asm volatile("" : "+v"(xb[m][u]));
      if constexpr (PARK) {
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int u = 0; u < XL; ++u) *(uint4_t *)(wbase + m * (XL * 1024) + 16 * (lane + 64 * u)) = xb[m][u];
        asm volatile("" ::: "memory");  // (the chunks are read back from LDS, not kept in registers behind the store)
      }
      if (act_bf16) {
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int u = 0; u < XL; ++u) {
            const uint4_t ub = PARK ? *(const uint4_t *)(wbase + m * (XL * 1024) + 16 * (lane + 64 * u)) : xb[m][u];
            xa[m][u] = swiglu_chunk<true>(xa[m][u], ub);
            asm volatile("" : "+v"(xa[m][u]));
          }
      } else {
#pragma unroll
        for (int m = 0; m < MR; ++m)
#pragma unroll
          for (int u = 0; u < XL; ++u) {
            const uint4_t ub = PARK ? *(const uint4_t *)(wbase + m * (XL * 1024) + 16 * (lane + 64 * u)) : xb[m][u];
            xa[m][u] = swiglu_chunk<false>(xa[m][u], ub);
            asm volatile("" : "+v"(xa[m][u]));
          }
      }
    }
    if constexpr (NORM) {
      // RMSNorm(x) in place of the x chunk (strip1_kernel.hpp, NORM).  PARK as for SWIGLU: the weight's chunks wait in the chunk's own slot
      // of the wave's staging area across the sum and the barrier
      constexpr bool PARK = NORM_PARK;
#pragma unroll
      for (int u = 0; u < XL; ++u) asm volatile("" : "+v"(xb[0][u]));
      if constexpr (PARK) {
#pragma unroll
        for (int u = 0; u < XL; ++u) *(uint4_t *)(wbase + 16 * (lane + 64 * u)) = xb[0][u];
        asm volatile("" ::: "memory");
      }
      float ss = 0.f;   // the lane's kept elements, chunk by chunk, element by element
      if (act_bf16) {
#pragma unroll
        for (int u = 0; u < XL; ++u) { float q = sumsq_chunk<true>(xa[0][u]); asm volatile("" : "+v"(q)); ss += xkeep[u] ? q : 0.f; }
      } else {
#pragma unroll
        for (int u = 0; u < XL; ++u) { float q = sumsq_chunk<false>(xa[0][u]); asm volatile("" : "+v"(q)); ss += xkeep[u] ? q : 0.f; }
      }
      // the wave's sum: all-reduce over each 16-lane row (xor 1, xor 2, half-row mirror, row mirror), then the four rows in order
      ss = dpp_add1<0xB1>(ss);
      ss = dpp_add1<0x4E>(ss);
      ss = dpp_add1<0x141>(ss);
      ss = dpp_add1<0x140>(ss);
      const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ss), 0));
      const float r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ss), 16));
      const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ss), 32));
      const float r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ss), 48));
      float *part = (float *)((char *)lds + strip1_lds_bytes<NW, MAXS, MR>());   // (LDS of its own: NW floats behind the staging areas)
      if (lane == 0) part[wave] = (r0 + r1) + (r2 + r3);
      __syncthreads();   // (every wave of the block is here: the surplus-block test above is block-uniform)
      float tot = part[0];
#pragma unroll
      for (int q = 1; q < NW; ++q) tot += part[q];   // index order: the same bits in every wave of every block of the launch
      const float rstd = rms_rstd(tot, 32 * T, p.norm_eps);
      if (p.rstd_out && b == 0 && blockIdx.y == 0 && threadIdx.x == 0) *p.rstd_out = rstd;
      // (the chunks are opaque again: nothing the sum derived from them -- their fp32 conversions -- is kept in registers across the barrier)
#pragma unroll
      for (int u = 0; u < XL; ++u) asm volatile("" : "+v"(xa[0][u]));
      if (act_bf16) {
#pragma unroll
        for (int u = 0; u < XL; ++u) {
          const uint4_t wb = PARK ? *(const uint4_t *)(wbase + 16 * (lane + 64 * u)) : xb[0][u];
          xa[0][u] = norm_chunk<true>(xa[0][u], wb, rstd);
          asm volatile("" : "+v"(xa[0][u]));
        }
      } else {
#pragma unroll
        for (int u = 0; u < XL; ++u) {
          const uint4_t wb = PARK ? *(const uint4_t *)(wbase + 16 * (lane + 64 * u)) : xb[0][u];
          xa[0][u] = norm_chunk<false>(xa[0][u], wb, rstd);
          asm volatile("" : "+v"(xa[0][u]));
        }
      }
    }
    // bf16 activations: converted in place behind ONE wave-uniform branch (the asm keeps hipcc from turning the branch back into
    // convert-then-select on every launch); fp16 launches execute none of it
    if (act_bf16) {
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int u = 0; u < XL; ++u) {
          xa[m][u] = __builtin_bit_cast(uint4_t, bf16x8_to_h8(xa[m][u]));
          asm volatile("" : "+v"(xa[m][u]));
        }
    }
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
    for (int u = 0; u < XL; ++u) {
      const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
      half8_t xv = __builtin_bit_cast(half8_t, xa[m][u]);   // (bf16: converted above)
      xv = xkeep[u] ? xv : zero8;
      // fragment slot order and per-slot divisors (the B-fragment construction below):
      //   4 bits: (k0,k4 | k1,k5 | k2,k6 | k3,k7), divisors (1,1 | 16,16 | 1,1 | 16,16);  3 bits: (k0,k5 | k1,k6 | k2,k7 | k3,k4), (2,1 | 16,8 | 128,64 | 1,1)
      const half8_t pv = B3 ? __builtin_shufflevector(xv, xv, 0, 5, 1, 6, 2, 7, 3, 4) : a_perm_04152637(xv);
      const half2_t p0 = {pv[0], pv[1]}, p1 = {pv[2], pv[3]}, p2 = {pv[4], pv[5]}, p3 = {pv[6], pv[7]};
      const half2_t d0 = B3 ? half2_t{(half_t)0.5f, (half_t)1.f} : half2_t{(half_t)1.f, (half_t)1.f};
      const half2_t d1 = B3 ? half2_t{(half_t)0.0625f, (half_t)0.125f} : half2_t{(half_t)0.0625f, (half_t)0.0625f};
      const half2_t d2 = B3 ? half2_t{(half_t)0.0078125f, (half_t)0.015625f} : half2_t{(half_t)1.f, (half_t)1.f};
      const half2_t d3 = B3 ? half2_t{(half_t)1.f, (half_t)1.f} : half2_t{(half_t)0.0625f, (half_t)0.0625f};
      const half2_t q0 = B3 ? p0 * d0 : p0, q1 = p1 * d1, q2 = B3 ? p2 * d2 : p2, q3 = B3 ? p3 : p3 * d3;
      const half2_t one = {(half_t)1.f, (half_t)1.f};
      float a = __builtin_amdgcn_fdot2(p0, one, 0.f, false);
      a = __builtin_amdgcn_fdot2(p1, one, a, false);
      a = __builtin_amdgcn_fdot2(p2, one, a, false);
      a = __builtin_amdgcn_fdot2(p3, one, a, false);
      float c = __builtin_amdgcn_fdot2(q0, one, 0.f, false);
      c = __builtin_amdgcn_fdot2(q1, one, c, false);
      c = __builtin_amdgcn_fdot2(q2, one, c, false);
      c = __builtin_amdgcn_fdot2(q3, one, c, false);
      // all-reduce over the 16 lanes of the row (= the 128 k of one group): xor 1, xor 2, half-row mirror, row mirror
      a = dpp_add1<0xB1>(a); c = dpp_add1<0xB1>(c);
      a = dpp_add1<0x4E>(a); c = dpp_add1<0x4E>(c);
      a = dpp_add1<0x141>(a); c = dpp_add1<0x141>(c);
      if constexpr (G64) {
        // 64-wide groups: the 8-lane halves of the row are two groups (2 g, 2 g + 1 of the pass); every lane needs both
        const float ao = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, a), 0x140, 0xF, 0xF, true));
        const float co = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, c), 0x140, 0xF, 0xF, true));
        const bool lo = (lane & 8) == 0;
        sx[m][u] = lo ? a : ao; sxp[m][u] = lo ? c : co;      // group 8 u + 2 g
        sx2[u] = lo ? ao : a; sxp2[u] = lo ? co : c;    // group 8 u + 2 g + 1
      } else {
        a = dpp_add1<0x140>(a); c = dpp_add1<0x140>(c);
        sx[m][u] = a; sxp[m][u] = c;   // lane (g, i): sums of group 4 u + g of the wave (batch row m)
      }
      *(half8_t *)(wbase + m * (XL * 1024) + 16 * (lane + 64 * u)) = half8_t{q0.x, q0.y, q1.x, q1.y, q2.x, q2.y, q3.x, q3.y};
    }
  } else {
#pragma unroll
    for (int u = 0; u < XL; ++u) { fold ^= xa[0][u].x ^ xa[0][u].y ^ xa[0][u].z ^ xa[0][u].w; sx[0][u] = sxp[0][u] = sx2[u] = sxp2[u] = 0.f; }
  }
  if constexpr (DBG) {
    if (dbg_slot && lane == 0) dbg_slot[2] = __builtin_amdgcn_s_memrealtime();
  }

  // ---- per lane: scale and correction of ITS group (pass ps: group 4 ps + g), while the weights are in flight ------------------
  constexpr int NCF = (MR > 1) ? MR : GPL;   // corrections per lane and pass: its group(s), or its four batch rows
  float sf[NPASS][GPL], cf[NPASS][NCF];
  if constexpr (LVL >= 4) {
    // a launch decodes its own kind of zero point only: one wave-uniform three-way branch (the asm keeps it a branch)
    float zfs[NPASS][GPL];
    if (zk == ZK_PACKED) {
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int h = 0; h < GPL; ++h) {
          const uint32_t zr = zraw[ps][h];
          if constexpr (B3) zfs[ps][h] = (float)(((uint32_t)(((((uint64_t)zraw2[ps][h]) << 32) | zr) >> (3 * i)) + (uint32_t)add_zero_bias) & 7u);
          else zfs[ps][h] = (float)(((zr >> (4 * (i & 7))) + (uint32_t)add_zero_bias) & 15u);
          asm volatile("" : "+v"(zfs[ps][h]));
        }
    } else if (zk == ZK_F16) {
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int h = 0; h < GPL; ++h) {
          const uint32_t zr = zraw[ps][h];
          zfs[ps][h] = (float)__builtin_bit_cast(half_t, (uint16_t)((i & 1) ? (zr >> 16) : (zr & 0xffffu)));
          asm volatile("" : "+v"(zfs[ps][h]));
        }
    } else {
#pragma unroll
      for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
        for (int h = 0; h < GPL; ++h) zfs[ps][h] = B3 ? 4.0f : 8.0f;
    }
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
      for (int h = 0; h < GPL; ++h) {
        const float zf = zfs[ps][h];
        sf[ps][h] = (float)sc[ps][h];
        if constexpr (MR > 1) {
#pragma unroll
          for (int m = 0; m < MR; ++m) cf[ps][m] = sf[ps][0] * __builtin_fmaf(zf, sx[m][ps], 1024.f * sxp[m][ps]);
        } else {
          cf[ps][h] = sf[ps][h] * __builtin_fmaf(zf, h ? sx2[ps] : sx[0][ps], 1024.f * (h ? sxp2[ps] : sxp[0][ps]));
        }
      }
  } else if constexpr (LVL >= 1) {
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps)
#pragma unroll
      for (int h = 0; h < GPL; ++h) fold ^= zraw[ps][h] ^ (uint32_t)__builtin_bit_cast(uint16_t, sc[ps][h]);
  }

  // ---- A fragment addresses: lane (g, i) is row i of the A operand; rows 4 j .. 4 j + 3 belong to group j of the pass -----------
  // k-step s reads at byte offset 64 s (an immediate): from the staged chunk if the row belongs to the k-step's group, else from
  // the zero block (whose address is pre-biased by the group's first offset)
  // k-step s = KPG j + r of pass ps reads at a_ptr[j] + 1024 ps + 64 r (an immediate): a row of the group finds its staged chunk there
  // -- the own-group address is ONE per-lane value: row i belongs to group i / 4 (i / 2) of every pass -- and every other row the zero
  // block at + 64 r: a compare and a select per group.  (Pointers, not offsets: the LDS base is added once, not per group.)
  const char *a_ptr[NG];
  const char *xs_own = wbase + 16 * g + 64 * KPG * (G64 ? (i >> 1) : (i >> 2)) + (MR > 1 ? (i & 3) * (XL * 1024) : 0);
#pragma unroll
  for (int j = 0; j < NG; ++j)
    a_ptr[j] = (G64 ? ((i >> 1) == (j & 7)) : ((i >> 2) == (j & 3))) ? xs_own : zeros + 16 * g - 1024 * ((KPG * j) >> 4);

  float4_t acc[NPASS][NCH];
  const uint32_t mask_lo = nib_mask_vgpr();  // 0x000f000f
  const uint32_t mask_hi = mask_lo << 4;     // 0x00f000f0
  // 3-bit field masks, derived from the opaque VGPR so hipcc can fuse each (x & m) | magic into one v_and_or_b32
  const uint32_t m3a = ((mask_lo & 0x7u) << 1) | (mask_lo & 0x00070000u);  // 0x0007000E
  const uint32_t m3b = m3a << 3, m3c = m3a << 6;                           // 0x00380070, 0x01C00380
  const uint32_t m3d = mask_lo & 0x00000007u, m3e = mask_lo & 0x00070000u;
  const uint32_t shift3 = (uint32_t)((32 - 8 * g) & 31);                   // funnel shift {0, 24, 16, 8}[g]
#pragma unroll
  for (int s = 0; s < MAXS; ++s) {
    const int j = s / KPG, ps = s >> 4, ch = s % NCH;
    if constexpr (LVL >= 2) {
      const half8_t av = *(const half8_t *)(a_ptr[j] + 1024 * ps + 64 * (s % KPG));
      if constexpr (LVL >= 3) {
        half2_t b0, b1, b2, b3;
        if constexpr (B3) {
          // f: the lane's 8 three-bit values at bits 0, 3, .., 21.  f1 = f << 1 puts q5, q6, q7 at bits 16, 19, 22 (upper half, offsets
          // 0, 3, 6) and q0, q1, q2 at bits 1, 4, 7 (lower half): three v_and_or give (2 q0, q5), (16 q1, 8 q6), (128 q2, 64 q7) on top of
          // 1024; q3, q4 (bits 9, 12) are moved to bit 0 / bit 16 separately
          const uint32_t f = __builtin_amdgcn_alignbit(wh[s], w[s], shift3), f1 = f << 1;
          b0 = as_h2((f1 & m3a) | kMagic);
          b1 = as_h2((f1 & m3b) | kMagic);
          b2 = as_h2((f1 & m3c) | kMagic);
          b3 = as_h2(((f << 4) & m3e) | (((f >> 9) & m3d) | kMagic));
        } else {
          const uint32_t wv = w[s], w8 = wv >> 8;
          b0 = as_h2((wv & mask_lo) | kMagic); b1 = as_h2((wv & mask_hi) | kMagic);
          b2 = as_h2((w8 & mask_lo) | kMagic); b3 = as_h2((w8 & mask_hi) | kMagic);
        }
        const half8_t bf = {b0.x, b0.y, b1.x, b1.y, b2.x, b2.y, b3.x, b3.y};
        const bool first = (s - 16 * ps) < NCH;  // the chain's first k-step of this pass
        const float4_t cin = first ? float4_t{0.f, 0.f, 0.f, 0.f} : acc[ps][ch];
        acc[ps][ch] = __builtin_amdgcn_mfma_f32_16x16x32_f16(av, bf, cin, 0, 0, 0);
      } else {
        const uint4_t ar = __builtin_bit_cast(uint4_t, av);
        fold ^= w[s] ^ ar.x ^ ar.y ^ ar.z ^ ar.w;
      }
    } else {
      fold ^= w[s];
    }
  }
  if constexpr (DBG) {
    if (dbg_slot && lane == 0) dbg_slot[3] = __builtin_amdgcn_s_memrealtime();
  }

  if constexpr (RESID_LATE) resid = ((const uint16_t *)p.residual)[b * 16 + i];
  // ---- the lane's value: its group's partial of column i; then one pass over [column][wave][g] -------------------------------------
  float val[MR];
  if constexpr (LVL >= 3) {
#pragma unroll
    for (int m = 0; m < MR; ++m) val[m] = 0.f;
#pragma unroll
    for (int ps = 0; ps < NPASS; ++ps) {
      if constexpr (MR > 1) {
#pragma unroll
        for (int m = 0; m < MR; ++m) {   // (register m of the lane's accumulators: batch row m of its group)
          float a = acc[ps][0][m];
#pragma unroll
          for (int ch = 1; ch < NCH; ++ch)
            if (16 * ps + ch < MAXS) a += acc[ps][ch][m];
          val[m] += __builtin_fmaf(sf[ps][0], a, -cf[ps][m]);
        }
      } else {
        float a = acc[ps][0][0], a2 = acc[ps][0][2];   // (rows 4 g, 4 g + 2 of the lane's column: its first / second group of the pass)
#pragma unroll
        for (int ch = 1; ch < NCH; ++ch)
          if (16 * ps + ch < MAXS) { a += acc[ps][ch][0]; a2 += acc[ps][ch][2]; }
        if constexpr (LVL >= 4) {
          val[0] += __builtin_fmaf(sf[ps][0], a, -cf[ps][0]);
          if constexpr (G64) val[0] += __builtin_fmaf(sf[ps][1], a2, -cf[ps][1]);
        } else val[0] += a;
      }
    }
    if constexpr (LVL < 4) val[0] = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, val[0]) ^ fold);
  } else {
    val[0] = __builtin_bit_cast(float, fold);
  }
  // (the early load stays up there, not behind the barrier; every weight word is long consumed: no wait.  The late one is waited for where it is used)
  if constexpr (RESID && !RESID_LATE) asm volatile("" : "+v"(resid));
#pragma unroll
  for (int m = 0; m < MR; ++m) lds[(m * 16 + i) * RS + wave * 4 + g] = val[m];
  __syncthreads();
  if constexpr (DBG) {
    if (dbg_slot && lane == 0) dbg_slot[4] = __builtin_amdgcn_s_memrealtime();
  }
  float vfin = 0.f;  // (lanes 0..15 of wave 0: the block's 16 outputs; MR = 4: threads 16 m .. 16 m + 15 hold batch row m)
  if (threadIdx.x < 16 * MR) {
    const float4_t *row = (const float4_t *)(lds + threadIdx.x * RS);
    float4_t t[NW];
#pragma unroll
    for (int q = 0; q < NW; ++q) t[q] = row[q];
    float v;
    if constexpr (LVL >= 3) {
#pragma unroll
      for (int st = 1; st < NW; st *= 2)
#pragma unroll
        for (int q = 0; q + st < NW; q += 2 * st) t[q] = t[q] + t[q + st];
      v = (t[0][0] + t[0][1]) + (t[0][2] + t[0][3]);
    } else {
      uint32_t f = 0;
#pragma unroll
      for (int q = 0; q < NW; ++q) { const uint4_t r = __builtin_bit_cast(uint4_t, t[q]); f ^= r.x ^ r.y ^ r.z ^ r.w; }
      v = (float)(f & 1023u);
    }
    const int n = b * 16 + (threadIdx.x & 15), mrow = threadIdx.x >> 4;
    if (pr.bias) v += (float)pr.bias[n];
    vfin = v;
    if constexpr (RESID) {
      // y = residual + linear(..) as the eager add of two tensors rounds it: the launch's own output rounded to the activation type (the
      // value the plain form stores), the sum in fp32, rounded again.  y may BE the residual row: this thread alone reads element n, and
      // it read it in the prologue
      if (act_bf16) {
        const float h = __builtin_bit_cast(float, (uint32_t)f32_to_bf16(v) << 16);
        ((uint16_t *)pr.y)[n] = f32_to_bf16(h + __builtin_bit_cast(float, resid << 16));
      } else {
        const half_t h = (half_t)v;
        ((half_t *)pr.y)[n] = (half_t)((float)h + (float)__builtin_bit_cast(half_t, (uint16_t)resid));
      }
    } else if constexpr (!AR) {
      if (MR == 1 || mrow < p.M) {
        const size_t at = (size_t)mrow * pr.n_strips * 16 + n;   // (y is [M][N], N = 16 n_strips)
        if (act_bf16) ((uint16_t *)pr.y)[at] = f32_to_bf16(v);
        else ((half_t *)pr.y)[at] = (half_t)v;
      }
    }
  }
  if constexpr (AR) {
    // ---- push: the 16 partial outputs as two 16-byte system-scope stores per peer (lanes 0 and 1 of wave 0, through LDS) ------------
    const int world = p.ar_world, rank = p.ar_rank;
    const size_t slot = p.ar_slot_bytes, payload = 2 * (size_t)world * slot;
    CommCtl *own = (CommCtl *)((char *)p.ar_peers[rank] + payload);
    // (every block reads the epoch before it takes its ticket; the last block bumps it after the last ticket)
    const uint32_t epoch = __hip_atomic_load(&own->epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
    const int parity = (int)(epoch & 1u);
    uint16_t *stage = (uint16_t *)(lds + 16 * RS);  // (the first wave's staging area: its activations are long consumed)
    int *s_last = (int *)(lds + 16 * RS) + 16;
    if (wave == 0) {
      if (lane < 16) stage[lane] = act_bf16 ? f32_to_bf16(vfin) : __builtin_bit_cast(uint16_t, (half_t)vfin);
      if (lane < 2) {
        const uint4_t chunk = *(const uint4_t *)(stage + 8 * lane);
        for (int q = 0; q < world; ++q) {
          char *dst = (char *)p.ar_peers[q] + ((size_t)parity * world + rank) * slot + ((size_t)b * 16 + 8 * lane) * 2;
          store16_sys(dst, chunk);
        }
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the write-through stores have left ...
      if (lane == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // ... (system scope) before the ticket says so
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t ticket = __hip_atomic_fetch_add(&own->ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *s_last = (ticket == gridDim.x - 1) ? 1 : 0;
      }
    }
    __syncthreads();
    if (*s_last == 0) return;
    // ---- the rank's last block: every block's slice is in every peer's slot.  Publish, wait for the world, sum in rank order ----------
    if (threadIdx.x == 0) __hip_atomic_store(&own->ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-arm (graph replay)
    if ((int)threadIdx.x < world) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");  // the other blocks' tickets (and the stores in front of them)
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      CommCtl *peer = (CommCtl *)((char *)p.ar_peers[threadIdx.x] + payload);
      __hip_atomic_store(&peer->flag[parity][rank], epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      unsigned spins = 0;
      while (__hip_atomic_load(&own->flag[parity][threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != epoch) {
        __builtin_amdgcn_s_sleep(2);
        if (++spins > (1u << 26)) {  // a peer never arrived (seconds): report instead of hanging the GPU
          if (p.ar_status) *p.ar_status = 1;
          break;
        }
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
    }
    __syncthreads();
    const char *mine = (const char *)p.ar_peers[rank] + (size_t)parity * world * slot;
    const int n16 = (int)gridDim.x * 2;  // 16-byte chunks of the output row (16 columns per block)
    for (int c = threadIdx.x; c < n16; c += NW * 64) {
      float a8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      for (int r = 0; r < world; ++r) {
        const uint4_t v = load16_sys(mine + (size_t)r * slot + (size_t)c * 16);
        const uint32_t wds[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (act_bf16) {
            a8[2 * j] += __builtin_bit_cast(float, wds[j] << 16);
            a8[2 * j + 1] += __builtin_bit_cast(float, wds[j] & 0xffff0000u);
          } else {
            const half2_t h = as_h2(wds[j]);
            a8[2 * j] += (float)h.x;
            a8[2 * j + 1] += (float)h.y;
          }
        }
      }
      uint32_t o[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (act_bf16) o[j] = (uint32_t)f32_to_bf16(a8[2 * j]) | ((uint32_t)f32_to_bf16(a8[2 * j + 1]) << 16);
        else o[j] = as_u32(half2_t{(half_t)a8[2 * j], (half_t)a8[2 * j + 1]});
      }
      *((uint4_t *)pr.y + c) = uint4_t{o[0], o[1], o[2], o[3]};
    }
    if (threadIdx.x == 0) __hip_atomic_store(&own->epoch, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if constexpr (DBG) {
    if (dbg_slot && lane == 0) dbg_slot[5] = __builtin_amdgcn_s_memrealtime();
  }
