// The routed experts of a sparse MoE block (Mixtral, Qwen3-MoE) for MORE than the decode pair's four tokens -- prompts, chunked prefill,
// batched decode, long verify steps -- as four launches, whatever the routing, with nothing going back to the host:
//
//   route     ids [T, top_k] -> the routing table (kernels.hpp, MoeRouteTable): slots sorted by expert, segments padded to row tiles
//   gate/up   h[slot] = act(x[t] . W_gate[e]) * (x[t] . W_up[e])          a grouped MFMA GEMM over the table's row tiles
//   down      prod[slot] = round(round(h[slot] . W_down[e]) * w[slot])     the same GEMM body
//   combine   y[t] = sum of its slots' prod rows in ascending expert id, one rounding per add, from +0
//
// Format of the layers and the contract y += s . sum x (q - z) on the unrounded W: moe_decode_kernel.hpp.
//
// Route.  ONE block of 16 waves, a counting sort.  Wave w owns a contiguous run of slots.  (1) every wave counts its run per expert in
// LDS (an atomic add whose result is not used: the counts do not depend on arrival order); (2) thread e turns expert e's 16 wave counts
// into exclusive prefixes and their total; (3) a block scan over the totals rounded up to whole tiles gives every expert's first row;
// thread e writes its count, its tiles (expert, first row) and -1 into its padding rows; (4) every wave walks its run again, 64 slots at
// a time: lanes with the same expert are found by ballot, their rank is the number of lower such lanes, and lane 0 advances the wave's
// running count of that expert.  A slot's row is  first row of its expert + slots of that expert in earlier waves + in earlier batches
// of the wave + in lower lanes:  ascending slot within an expert, the same table for the same ids every time.
//
// The GEMM.  grid (row-tile bound S / BM + min(E, S), column panels), 4 waves.  A block reads the tile count first and leaves when its
// tile does not exist; else its expert e and its BM sorted rows.  Every wave owns TWO B streams of 16 columns: gate and up of the same
// strip (panel = 64 columns of I), or two neighbouring strips of W_down (panel = 128 columns of H).  K is walked in tiles of 256 (two
// groups):
//   A  thread (row r = tid / 32 + 8 j, 16-byte chunk tid % 32) loads its piece of the gathered row -- x[slot / top_k] or h[slot]; a
//      padding row is zeros -- of tile kt + 1 into registers while tile kt is multiplied, converts bf16 to fp16 and writes it to the other
//      LDS buffer: [2][BM rows][512 + 16 bytes] (the 16 spread the rows of a fragment read over all banks); one barrier per tile;
//   B  lane (g, i) of a wave holds, per stream and k-step of 32, the ONE word with k = 8 g .. 8 g + 7 of column i (256 contiguous bytes
//      per wave and load), requested one tile ahead.  A fragment is the raw (1024 + q | 64 + q) fp16 patterns minus (1024 + z | 64 + z):
//      the exact integers q - z (panel.hip's construction), so a group of four v_mfma_f32_16x16x32_f16 ends with one fp32 fma by the
//      scale per accumulator and no sum carries a 1024-sized term.
// BM / 16 row tiles share every B fragment.  The epilogue stays in registers: a lane has rows 4 g .. 4 g + 3 of column i; it rounds,
// swaps with its column neighbour and the even lane stores two columns (gate/up: swiglu_pair; down: round(d) * w in fp32, rounded again
// behind moe_down_kernel's fold-preventing barrier) to the row of the slot -- slot order, so h is ops.moe_gate_up's layout.
//
// Combine.  grid (H / 8 / 256, T): thread (token, 8 columns) adds the token's product rows in ascending (expert, slot).
#include "kernels.hpp"
#include "moe_decode_kernel.hpp"

namespace qllm {

namespace {

__global__ __launch_bounds__(kMoeRouteThreads) void moe_route_kernel(const int64_t *ids, int *tab, const MoeRouteTable tb, const int S, const int E,
                                                                     const int BM) {
  extern __shared__ int route_lds[];               // wcount[16][E] | off[E] | cnt[E] | wsum[16]
  int *wcount = route_lds, *off = wcount + kMoeRouteWaves * E, *cnt = off + E, *wsum = cnt + E;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < kMoeRouteWaves * E; i += kMoeRouteThreads) wcount[i] = 0;
  __syncthreads();

  const int per = ((S + kMoeRouteWaves - 1) / kMoeRouteWaves + 63) / 64 * 64;
  const int s0 = wave * per, s1 = min(S, s0 + per);
  for (int s = s0 + lane; s < s1; s += 64) {
    const int64_t e = ids[s];
    if (e >= 0 && e < E) atomicAdd(&wcount[wave * E + (int)e], 1);
  }
  __syncthreads();
  for (int e = tid; e < E; e += kMoeRouteThreads) {
    int run = 0;
    for (int w = 0; w < kMoeRouteWaves; ++w) {
      const int c = wcount[w * E + e];
      wcount[w * E + e] = run;
      run += c;
    }
    cnt[e] = run;
  }
  __syncthreads();

  // exclusive scan of the padded counts over the experts (E <= 1024 = one per thread)
  const int c = tid < E ? cnt[tid] : 0;
  const int v = (c + BM - 1) / BM * BM;
  int inc = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int n = __shfl_up(inc, d);
    if (lane >= d) inc += n;
  }
  if (lane == 63) wsum[wave] = inc;
  __syncthreads();
  int base = 0;
  for (int w = 0; w < wave; ++w) base += wsum[w];
  const int first = base + inc - v;
  if (tid == kMoeRouteThreads - 1) {
    tab[0] = (base + inc) / BM;
    tab[1] = BM;
  }
  if (tid < E) {
    off[tid] = first;
    tab[tb.counts + tid] = c;
    for (int i = 0; i < v / BM; ++i) {
      tab[tb.tile_expert + first / BM + i] = tid;
      tab[tb.tile_row0 + first / BM + i] = first + i * BM;
    }
    for (int r = first + c; r < first + v; ++r) tab[tb.sorted + r] = -1;
  }
  __syncthreads();

  for (int b = s0; b < s1; b += 64) {
    const int s = b + lane;
    int e = -1;
    if (s < s1) {
      const int64_t id = ids[s];
      if (id >= 0 && id < E) e = (int)id;
    }
    uint64_t todo = __ballot(e >= 0);
    while (todo) {
      const int le = __shfl(e, __ffsll((long long)todo) - 1);
      const uint64_t same = __ballot(e == le);
      int seen = 0;
      if (lane == 0) {                             // (lane 0 alone reads and writes the wave's running counts)
        seen = wcount[wave * E + le];
        wcount[wave * E + le] = seen + __popcll(same);
      }
      seen = __shfl(seen, 0);
      if (e == le) tab[tb.sorted + off[le] + seen + __popcll(same & ((1ull << lane) - 1ull))] = s;
      todo &= ~same;
    }
  }
}

template <int BM, bool DOWN, bool BF16>
__global__ __launch_bounds__(kMoePrefillThreads) void moe_prefill_gemm_kernel(const MoePrefillParams p) {
  constexpr int MT = BM / 16, NR = BM / 8;         // row tiles; rows a thread stages per K tile
  constexpr int KS = kMoePrefillKT / 32;           // k-steps per K tile
  constexpr int ROWB = kMoePrefillKT * 2 + 16;     // bytes of a staged row
  extern __shared__ __attribute__((aligned(16))) uint8_t moe_a[];   // [2][BM][ROWB]
  const int tile = blockIdx.x;
  if (tile >= p.table[0]) return;
  const int e = p.table[p.tb.tile_expert + tile];
  const int *srt = p.table + p.tb.sorted + p.table[p.tb.tile_row0 + tile];

  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int K = p.K, N = p.N, G = K >> 7, NS = N >> 4, nkt = (K + kMoePrefillKT - 1) / kMoePrefillKT, kchunks = K >> 3;

  // ---- A: the pieces this thread stages ----
  const int ac = tid & 31, ar = tid >> 5;
  const uint4_t *rowp[NR];
#pragma unroll
  for (int j = 0; j < NR; ++j) {
    const int slot = srt[ar + 8 * j];
    rowp[j] = slot < 0 ? nullptr : (const uint4_t *)p.a + (int64_t)(DOWN ? slot : slot / p.top_k) * kchunks;
  }
  uint4_t av[NR];
  auto load_a = [&](const int kt) __attribute__((always_inline)) {
    const int ck = kt * (kMoePrefillKT / 8) + ac;
#pragma unroll
    for (int j = 0; j < NR; ++j) av[j] = (rowp[j] && ck < kchunks) ? rowp[j][ck] : uint4_t{0u, 0u, 0u, 0u};
  };
  auto store_a = [&](const int buf) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < NR; ++j) {
      uint4_t v = av[j];
      if constexpr (BF16) v = __builtin_bit_cast(uint4_t, bf16x8_to_h8(v));
      *(uint4_t *)(moe_a + (buf * BM + ar + 8 * j) * ROWB + ac * 16) = v;
    }
  };

  // ---- B: two streams of 16 columns per wave ----
  int strip[2];
  const uint32_t *wq[2], *zq[2];
  const half_t *sq[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    strip[j] = DOWN ? ((int)blockIdx.y * kMoePrefillWaves + wave) * 2 + j : (int)blockIdx.y * kMoePrefillWaves + wave;
    const int64_t sg0 = ((int64_t)e * NS + strip[j]) * G;          // (strip, group 0) counted over the whole stack
    const uint32_t *qw = (DOWN || j == 0) ? p.q0 : p.q1, *qz = (DOWN || j == 0) ? p.z0 : p.z1;
    const half_t *sc = (DOWN || j == 0) ? p.s0 : p.s1;
    wq[j] = qw + sg0 * 256 + lane;
    sq[j] = sc + sg0 * 16 + i;
    zq[j] = qz ? qz + sg0 * 2 + (i >> 3) : nullptr;
  }
  const uint32_t zsh = 4u * (uint32_t)(i & 7);
  uint32_t w[2][KS], wn[2][KS], zr[2][2], zrn[2][2];
  half_t sc[2][2], scn[2][2];
  auto load_b = [&](const int kt) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int gl = 0; gl < 2; ++gl) {
        const int gi = min(kt * 2 + gl, G - 1);
        scn[j][gl] = sq[j][gi * 16];
        zrn[j][gl] = zq[j] ? zq[j][gi * 2] : 0x88888888u;
      }
#pragma unroll
      for (int s = 0; s < KS; ++s) wn[j][s] = wq[j][(int64_t)min(kt * KS + s, (K >> 5) - 1) * 64];
    }
  };

  const uint32_t mask_lo = nib_mask_vgpr(), mask_hi = mask_lo << 4;
  constexpr uint32_t kMagic64 = 0x54005400u;       // (64.0h, 64.0h): a nibble at bits 4-7 of an fp16 in [64, 128) weighs exactly 1
  float4_t yacc[MT][2];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) yacc[mt][0] = yacc[mt][1] = float4_t{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](const int kt, const int buf) __attribute__((always_inline)) {
    const uint8_t *ab = moe_a + buf * BM * ROWB + i * ROWB + g * 16;
    float4_t gacc[MT][2];
    half2_t nz[2][2];
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int gl = s / 4;
      if (kt * 2 + gl < G) {                       // (block-uniform: the last tile of an odd number of groups has one)
        if (s % 4 == 0) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float zf = (float)(((zr[j][gl] >> zsh) + (uint32_t)p.add_zero_bias) & 15u);
            nz[j][0] = splat2((half_t)(-1024.f - zf));   // exact: integers below 2048
            nz[j][1] = splat2((half_t)(-64.f - zf));
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) gacc[mt][j] = float4_t{0.f, 0.f, 0.f, 0.f};
          }
        }
        half8_t af[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) af[mt] = *(const half8_t *)(ab + mt * 16 * ROWB + s * 64);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const uint32_t wv = w[j][s], w8 = wv >> 8;
          const half2_t b0 = as_h2((wv & mask_lo) | kMagic) + nz[j][0], b1 = as_h2((wv & mask_hi) | kMagic64) + nz[j][1];
          const half2_t b2 = as_h2((w8 & mask_lo) | kMagic) + nz[j][0], b3 = as_h2((w8 & mask_hi) | kMagic64) + nz[j][1];
          // registers hold (k0,k4) (k1,k5) (k2,k6) (k3,k7): four v_perm_b32 put them in natural order
          const uint32_t c0 = __builtin_amdgcn_perm(as_u32(b1), as_u32(b0), 0x05040100u), c2 = __builtin_amdgcn_perm(as_u32(b1), as_u32(b0), 0x07060302u);
          const uint32_t c1 = __builtin_amdgcn_perm(as_u32(b3), as_u32(b2), 0x05040100u), c3 = __builtin_amdgcn_perm(as_u32(b3), as_u32(b2), 0x07060302u);
          const half8_t bf = __builtin_bit_cast(half8_t, uint4_t{c0, c1, c2, c3});
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) gacc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[mt], bf, gacc[mt][j], 0, 0, 0);
        }
        if (s % 4 == 3) {                          // y += scale * sum x (q - z) of the group
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const float sf = (float)sc[j][gl];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
              for (int q = 0; q < 4; ++q) yacc[mt][j][q] = __builtin_fmaf(sf, gacc[mt][j][q], yacc[mt][j][q]);
          }
        }
      }
    }
  };

  // ---- main loop: tile kt + 1 travels to registers while tile kt is multiplied; one barrier per tile ----
  load_a(0);
  load_b(0);
  store_a(0);
  __syncthreads();
  for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int s = 0; s < KS; ++s) w[j][s] = wn[j][s];
#pragma unroll
      for (int gl = 0; gl < 2; ++gl) sc[j][gl] = scn[j][gl], zr[j][gl] = zrn[j][gl];
    }
    if (kt + 1 < nkt) {
      load_a(kt + 1);
      load_b(kt + 1);
    }
    compute(kt, kt & 1);
    if (kt + 1 < nkt) store_a((kt + 1) & 1);
    __syncthreads();
  }

  // ---- epilogue: lane (g, i) has rows 16 mt + 4 g + q of column i of both streams ----
  uint32_t *out = (uint32_t *)p.out;
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int slot = srt[16 * mt + 4 * g + q];
      if constexpr (!DOWN) {
        const uint32_t gb = moe_bits<BF16>(yacc[mt][0][q]), ub = moe_bits<BF16>(yacc[mt][1][q]);
        const uint32_t g2 = gb | ((uint32_t)__shfl_xor((int)gb, 1) << 16), u2 = ub | ((uint32_t)__shfl_xor((int)ub, 1) << 16);
        if (slot >= 0 && !(i & 1)) out[((int64_t)slot * N + strip[0] * 16 + i) >> 1] = swiglu_pair<BF16>(g2, u2);
      } else {
        float wt = 0.f;
        if (slot >= 0) {
          if (p.weights_f32) wt = ((const float *)p.weights)[slot];
          else if constexpr (BF16) wt = __builtin_bit_cast(float, (uint32_t)((const uint16_t *)p.weights)[slot] << 16);
          else wt = (float)((const half_t *)p.weights)[slot];
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          // the product is an fp32 value that is rounded again, as eager rounds it: the empty asm keeps hipcc from folding the multiply
          // and the conversion into one v_fma_mixlo_f16 (moe_down_kernel has the case)
          float prod = moe_round<BF16>(yacc[mt][j][q]) * wt;
          asm volatile("" : "+v"(prod));
          const uint32_t pb = moe_bits<BF16>(prod);
          const uint32_t p2 = pb | ((uint32_t)__shfl_xor((int)pb, 1) << 16);
          if (slot >= 0 && !(i & 1)) out[((int64_t)slot * N + strip[j] * 16 + i) >> 1] = p2;
        }
      }
    }
}

template <bool BF16>
__global__ __launch_bounds__(256) void moe_combine_kernel(const MoeCombineParams p) {
  __shared__ int eid[kMoeMaxTopK];
  const int tid = threadIdx.x, t = blockIdx.y, top_k = p.top_k, chunks = p.H >> 3;
  const int c = blockIdx.x * 256 + tid;
  if (tid < top_k) {
    const int64_t e = p.ids[(int64_t)t * top_k + tid];
    eid[tid] = (e >= 0 && e < p.E) ? (int)e : -1;
  }
  __syncthreads();
  if (c >= chunks) return;
  float y[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const uint4_t *rows = (const uint4_t *)p.prod + (int64_t)t * top_k * chunks + c;
  int last = -1;
  for (int n = 0; n < top_k; ++n) {                // ascending expert id (equal ids: ascending slot), one rounding per add, from +0
    int best = 0x7fffffff, bs = -1;
    for (int s = 0; s < top_k; ++s) {
      const int key = eid[s] * kMoeMaxTopK + s;
      if (eid[s] >= 0 && key > last && key < best) best = key, bs = s;
    }
    if (bs < 0) break;
    last = best;
    const uint4_t v = rows[(int64_t)bs * chunks];
    const uint32_t vw[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float lo, hi;
      if constexpr (BF16) lo = __builtin_bit_cast(float, vw[k] << 16), hi = __builtin_bit_cast(float, vw[k] & 0xffff0000u);
      else lo = (float)as_h2(vw[k]).x, hi = (float)as_h2(vw[k]).y;
      y[2 * k] = moe_round<BF16>(y[2 * k] + lo);
      y[2 * k + 1] = moe_round<BF16>(y[2 * k + 1] + hi);
    }
  }
  uint32_t o[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) o[k] = (uint32_t)moe_bits<BF16>(y[2 * k]) | ((uint32_t)moe_bits<BF16>(y[2 * k + 1]) << 16);
  ((uint4_t *)p.y)[(int64_t)t * chunks + c] = uint4_t{o[0], o[1], o[2], o[3]};
}

template <int BM, bool DOWN>
int launch_gemm(const MoePrefillParams &p, int S, int E, int act_bf16, hipStream_t stream) {
  static DeviceLatch latch[2];
  auto kernel = act_bf16 ? moe_prefill_gemm_kernel<BM, DOWN, true> : moe_prefill_gemm_kernel<BM, DOWN, false>;
  const size_t lds = moe_prefill_lds_bytes(BM);
  if (lds > 64 * 1024)
    if (int rc = lds_optin(latch[act_bf16 ? 1 : 0], (const void *)kernel)) return rc;
  const dim3 grid(moe_prefill_max_tiles(S, E, BM), p.N / (DOWN ? 128 : 64));
  hipLaunchKernelGGL(kernel, grid, dim3(kMoePrefillThreads), lds, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace

size_t moe_prefill_lds_bytes(int tile_rows) { return (size_t)2 * tile_rows * (kMoePrefillKT * 2 + 16); }
size_t moe_route_lds_bytes(int E) { return ((size_t)(kMoeRouteWaves + 2) * E + kMoeRouteWaves) * sizeof(int); }

// shapes, ranges, types, alignment and the workspace's size: checked by the entries (capi.hip, check_moe_prefill)
int launch_moe_route(const int64_t *ids, int *table, int S, int E, int tile_rows, hipStream_t stream) {
  static DeviceLatch latch;
  const size_t lds = moe_route_lds_bytes(E);
  if (lds > 64 * 1024)
    if (int rc = lds_optin(latch, (const void *)moe_route_kernel)) return rc;
  hipLaunchKernelGGL(moe_route_kernel, dim3(1), dim3(kMoeRouteThreads), lds, stream, ids, table, moe_route_table(S, E), S, E, tile_rows);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

int launch_moe_prefill_gemm(const MoePrefillParams &p0, int down, int S, int E, int tile_rows, int act_bf16, hipStream_t stream) {
  MoePrefillParams p = p0;
  if (!p.z0 || (!down && !p.z1)) p.add_zero_bias = 0;   // (the symmetric grid has no stored zero point to offset)
  if (tile_rows == kMoePrefillTileLo)
    return down ? launch_gemm<kMoePrefillTileLo, true>(p, S, E, act_bf16, stream) : launch_gemm<kMoePrefillTileLo, false>(p, S, E, act_bf16, stream);
  return down ? launch_gemm<kMoePrefillTileHi, true>(p, S, E, act_bf16, stream) : launch_gemm<kMoePrefillTileHi, false>(p, S, E, act_bf16, stream);
}

int launch_moe_combine(const MoeCombineParams &p, int T, int act_bf16, hipStream_t stream) {
  auto kernel = act_bf16 ? moe_combine_kernel<true> : moe_combine_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((p.H / 8 + 255) / 256, T), dim3(256), 0, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
