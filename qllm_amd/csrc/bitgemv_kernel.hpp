// The bit-stream matvec's kernel body, shared by its three translation units: bitgemv.hip (the decomposition is described there),
// bitgemv_ao.hip (the gathering form for act-order layers) and bitgemv_group.hip (up to four layers sharing x in one launch).  Each of
// them instantiates 7 widths x 5 row tiles under a kernel name of its own.
#pragma once
#include "kernels.hpp"

namespace qllm {
namespace bg {

#ifndef QLLM_BG_COLS
#define QLLM_BG_COLS 32
#endif
#ifndef QLLM_BG_FILL
#define QLLM_BG_FILL 2   // K is split over blocks until the launch has this many blocks per CU (rounded up)
#endif
constexpr int kCols = QLLM_BG_COLS;     // columns per block
constexpr int kPar = 64 / kCols;        // unit parities per wave (64 lanes = kCols columns x kPar)
constexpr int kNW = 8;        // waves per block
constexpr int kSlots = kNW * kPar;  // lane slots a block's units are dealt to
constexpr int kXsBytes = 112 * 1024;  // LDS budget of the staged activations (+ their sums; the reduction scratch reuses it)

// units of a lane whose words are in flight together: at most 32 registers of packed words at 1-2 rows (80 registers in all: three blocks per CU; 48 words cost a third of the resident blocks and 25 % on the 11008-wide shapes), 40 at 4 rows -- fewer with many activation rows, whose
// accumulators need the registers (16 rows: 16 words; every instantiation spill-free, tests/test_kernel_resources_cpu.py)
__host__ __device__ constexpr int round_units(int bits, int mt) {
  const int budget = mt <= 2 ? 32 : (mt == 4 ? 40 : (mt == 8 ? 24 : 16)), most = mt <= 4 ? 8 : (mt == 8 ? 4 : 2);
  return budget / bits > most ? most : (budget / bits < 1 ? 1 : budget / bits);
}

// how the 32 fields of a unit pair up into 16 packed operands: pair p = fields (a(p), b(p))
template <int BITS>
struct Pairing {
  static constexpr bool kShared = (16 % BITS) == 0;  // fields 16 bits apart in one word share a shift
  static constexpr int kPerWord = 32 / BITS, kHalf = 16 / BITS;
  __host__ __device__ static constexpr int a(int p) { return kShared ? (p / (kHalf ? kHalf : 1)) * kPerWord + p % (kHalf ? kHalf : 1) : 2 * p; }
  __host__ __device__ static constexpr int b(int p) { return kShared ? a(p) + kHalf : 2 * p + 1; }
};

// packed operand (q_a, q_b) as exact fp16 of pair P (compile-time) from the unit's words
template <int BITS, int P>
__device__ __forceinline__ half2_t pair_of(const uint32_t *w) {
  constexpr uint32_t mask = (1u << BITS) - 1u;
  uint32_t v;
  if constexpr (Pairing<BITS>::kShared) {
    constexpr int half = Pairing<BITS>::kHalf, wd = P / half, sh = BITS * (P % half);
    v = ((w[wd] >> sh) & (mask | (mask << 16))) | kMagic;
  } else {
    constexpr int o0 = 2 * P * BITS, wi = o0 >> 5, sh = o0 & 31;
    uint32_t win;
    if constexpr (sh + 2 * BITS <= 32) win = w[wi] >> sh;
    else win = __builtin_amdgcn_alignbit(w[wi + 1], w[wi], sh);
    v = (win & mask) | ((win << (16 - BITS)) & (mask << 16)) | kMagic;
  }
  return as_h2(v) - splat2((half_t)1024.0f);  // exact: 1024 + q, q <= 255, is an integer below 2048
}

// staging: pair K (0..7) of a half unit from its 16 natural-order halves (lo = halves 0..7, hi = 8..15), converted to fp16 if the
// caller's activations are bf16; adds the pair's two values to `sum`.  The pairings keep a half unit's pairs inside it.
template <int I>
__device__ __forceinline__ uint32_t half_of(const uint4_t &lo, const uint4_t &hi) {
  constexpr int r = I >> 1;
  const uint32_t word = r == 0 ? lo.x : r == 1 ? lo.y : r == 2 ? lo.z : r == 3 ? lo.w : r == 4 ? hi.x : r == 5 ? hi.y : r == 6 ? hi.z : hi.w;
  return (I & 1) ? (word >> 16) : (word & 0xffffu);
}
template <int BITS, int K>
__device__ __forceinline__ uint32_t stage_pair(const uint4_t &lo, const uint4_t &hi, bool bf16, float &sum) {
  constexpr int a = Pairing<BITS>::a(K), b = Pairing<BITS>::b(K);
  static_assert(a < 16 && b < 16, "a half unit's pairs stay inside it");
  uint32_t v = half_of<a>(lo, hi) | (half_of<b>(lo, hi) << 16);
  if (bf16) v = as_u32(bf16x2_to_h2(v));
  const half2_t hh = as_h2(v);
  sum += (float)hh.x + (float)hh.y;
  return v;
}

template <int BITS, int MT, int Q>
__device__ __forceinline__ void quad_dot(const uint32_t *w, const uint32_t *xs_u, int x_stride, float (&acc)[MT]) {
  // 4 pairs per ds_read_b128 (the 16 lanes of a unit parity read the same address: a broadcast)
  const half2_t q0 = pair_of<BITS, 4 * Q>(w), q1 = pair_of<BITS, 4 * Q + 1>(w), q2 = pair_of<BITS, 4 * Q + 2>(w), q3 = pair_of<BITS, 4 * Q + 3>(w);
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const uint4_t xv = *(const uint4_t *)(xs_u + m * x_stride + 4 * Q);
    float a = acc[m];
    a = __builtin_amdgcn_fdot2(as_h2(xv.x), q0, a, false);
    a = __builtin_amdgcn_fdot2(as_h2(xv.y), q1, a, false);
    a = __builtin_amdgcn_fdot2(as_h2(xv.z), q2, a, false);
    a = __builtin_amdgcn_fdot2(as_h2(xv.w), q3, a, false);
    acc[m] = a;
  }
}

// The kernel body of bitgemv.hip (GATHER = false: x as it is) and bitgemv_ao.hip (GATHER = true: x[:, perm], an act-order layer served
// from its row-sorted copy).  The two differ in the staging pass alone -- where a thread's 16 activations come from; the LDS image, the
// order of every sum and hence the result are those of the plain kernel run on a gathered copy of x.  `bid`: the block's id among the
// blocks of THIS layer -- blockIdx.x in both of them; bitgemv_group.hip, whose launch carries several layers, passes a local one.
template <int BITS, int MT, bool GATHER>
__device__ __forceinline__ void bitgemv_body(const BitGemvParams p, const int32_t *__restrict__ perm, const uint32_t bid) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // (the gathering form of 7 bits x 16 rows does not fit two units' words next to its 16 indices and activations -- 256 registers and
  //  27 spilled, against 212 of the plain kernel: it keeps ONE unit in flight (157).  A lane walks its units in the same order for every
  //  UB, so no sum changes)
  constexpr int UB = (GATHER && BITS == 7 && MT == 16) ? 1 : round_units(BITS, MT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int col = lane % kCols, slot = wave * kPar + lane / kCols;
  const int nbc = p.n_col_blocks;
  const int j = bid % nbc, kb = bid / nbc;
  // block id -> column block: consecutive ids go round the 8 XCDs, so ids j and j + 8 run on one XCD back to back -- give them the two
  // 64-byte halves of one 128-byte line of the word rows (whole multiples of 16 column blocks only; else the identity)
  const int nb = (kCols == 16 && nbc % 16 == 0) ? 2 * (((j >> 3) >> 1) * 8 + (j & 7)) + ((j >> 3) & 1) : j;
  const int n = nb * kCols + col;
  const int nc = n < p.N ? n : p.N - 1;  // (dead lanes of a ragged last block re-read the last column and store nothing)
  const int U = p.K / 32;
  const int u_begin = (int)((long long)U * kb / p.ksplit), u_end = (int)((long long)U * (kb + 1) / p.ksplit);
  // LDS: [MT][chunk units][16 pairs] u32 | [MT][chunk units] f32 sums; the reduction scratch reuses it at the end
  uint32_t *xs = (uint32_t *)smem;
  const int cu = p.chunk_units, x_stride = cu * 16;
  float *sx = (float *)(smem + (size_t)MT * cu * 64);

  float y[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) y[m] = 0.f;
  const uint32_t *wcol = p.qweight + nc;
  const int zk = p.zero_kind;
  const int zwords = (p.N * BITS) >> 5;  // packed zero points: words per group row
  uint32_t w[UB][BITS];
  uint32_t sc[UB];   // raw fp16 bits
  uint32_t zr0[UB], zr1[UB];  // zero point of (group, column), raw: the fp16 value, or the two words its packed field may straddle
  const int zbit = nc * BITS, zw = zbit >> 5, zw1 = min(zw + 1, zwords - 1);
  // the words of round r of the chunk starting at unit c0: units c0 + slot + kSlots (r UB + i) -- with their group's scale and zero
  // point (a lane's units are kSlots apart: nearly every one is in another group, and a load inside the arithmetic would be one
  // exposed round trip per unit)
  auto load_round = [&](int c0, int c1, int r) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < UB; ++i) {
      const int u = c0 + slot + kSlots * (r * UB + i);
      if (u < c1) {
        const uint32_t *src = wcol + (size_t)u * BITS * p.N;
#pragma unroll
        for (int b = 0; b < BITS; ++b) w[i][b] = __builtin_nontemporal_load(src + (size_t)b * p.N);
        const size_t g = (size_t)((32 * u) / p.group_size);
        sc[i] = ((const uint16_t *)p.scales)[g * p.N + nc];
        // (ONE store pattern for every zero-point kind: stores under a per-kind branch get merged into a dynamically indexed one, and
        //  the arrays then live in scratch memory)
        if (zk != ZK_SYM) {
          const size_t i0 = zk == ZK_F16 ? (g * p.N + nc) >> 1 : g * zwords + zw;   // fp16 zero points: the dword holding the half (N is even)
          const size_t i1 = zk == ZK_F16 ? i0 : g * zwords + zw1;
          zr0[i] = ((const uint32_t *)p.qzeros)[i0];
          zr1[i] = ((const uint32_t *)p.qzeros)[i1];
        }
      }
    }
  };
  auto zero_of = [&](int i) __attribute__((always_inline)) -> float {
    if (zk == ZK_F16) return (float)__builtin_bit_cast(half_t, (uint16_t)((nc & 1) ? (zr0[i] >> 16) : zr0[i]));
    if (zk == ZK_SYM) return (float)(1 << (BITS - 1));
    const uint64_t v = ((uint64_t)zr1[i] << 32) | zr0[i];   // (zw1 == zw only when the field ends inside word zw)
    return (float)(((uint32_t)(v >> (zbit & 31)) + (uint32_t)p.add_zero_bias) & ((1u << BITS) - 1u));
  };

  for (int c0 = u_begin; c0 < u_end; c0 += cu) {
    const int c1 = min(c0 + cu, u_end), nu = c1 - c0;
    load_round(c0, c1, 0);            // in flight while x is staged
    __builtin_amdgcn_sched_barrier(0);
    __syncthreads();                  // (the previous chunk's readers are done)
    // ---- stage x[m][32 c0 .. 32 c1) as fp16 pairs in the unit's pairing (rows past M: zeros) + the sum of every unit's activations.
    //      One thread = half a unit: two 16-byte loads, its 8 pairs (the pairings keep a half unit's pairs inside it), two 16-byte
    //      LDS stores; the two halves of a unit are neighbouring lanes ------------------------------------------------------------
    for (int i0 = 0; i0 < MT * nu * 2; i0 += kNW * 64) {
      const int i = i0 + tid;
      const bool in = i < MT * nu * 2;
      const int h = i & 1, u = in ? (i >> 1) % nu : 0, m = in ? (i >> 1) / nu : MT;
      uint4_t lo = uint4_t{0, 0, 0, 0}, hi = uint4_t{0, 0, 0, 0};
      if (m < p.M) {
        if constexpr (GATHER) {
          // the half unit's 16 perm entries are 64 contiguous bytes; its activations are 16 two-byte loads of row m (<= 16 K 2 bytes:
          // L2-resident).  Every index is clamped to 0..K-1: a perm that is no permutation gives a wrong number, never an access
          // outside x.  (perm is re-read per row: the entries of a half unit do not depend on m, and the flat (row, unit, half) loop
          //  keeps the plain kernel's shape)
          const int4 *pr = (const int4 *)(perm + 32 * (c0 + u) + 16 * h);
          const int4 p0 = pr[0], p1 = pr[1], p2 = pr[2], p3 = pr[3];
          // (32-bit element offsets from the uniform base of x -- the entry point refuses M K >= 2^31 -- cost one register per address;
          //  the halves are moved as bits, fp16 or bf16 alike)
          const half_t *xb = (const half_t *)p.x;
          const uint32_t row0 = (uint32_t)m * (uint32_t)p.K;
          const int kmax = p.K - 1;
          auto two = [&](int a, int b) __attribute__((always_inline)) -> uint32_t {
            half2_t v;
            v.x = xb[row0 + (uint32_t)min(max(a, 0), kmax)];
            v.y = xb[row0 + (uint32_t)min(max(b, 0), kmax)];
            return as_u32(v);
          };
          lo = uint4_t{two(p0.x, p0.y), two(p0.z, p0.w), two(p1.x, p1.y), two(p1.z, p1.w)};
          hi = uint4_t{two(p2.x, p2.y), two(p2.z, p2.w), two(p3.x, p3.y), two(p3.z, p3.w)};
        } else {
          const uint4_t *xr = (const uint4_t *)((const uint16_t *)p.x + (size_t)m * p.K + 32 * (c0 + u) + 16 * h);
          lo = xr[0];
          hi = xr[1];
        }
      }
      float sum = 0.f;
      const bool bf = p.act_bf16;
      const uint32_t o0 = stage_pair<BITS, 0>(lo, hi, bf, sum), o1 = stage_pair<BITS, 1>(lo, hi, bf, sum), o2 = stage_pair<BITS, 2>(lo, hi, bf, sum),
                     o3 = stage_pair<BITS, 3>(lo, hi, bf, sum), o4 = stage_pair<BITS, 4>(lo, hi, bf, sum), o5 = stage_pair<BITS, 5>(lo, hi, bf, sum),
                     o6 = stage_pair<BITS, 6>(lo, hi, bf, sum), o7 = stage_pair<BITS, 7>(lo, hi, bf, sum);
      sum += __shfl_xor(sum, 1, 64);
      if (in) {
        uint4_t *dst = (uint4_t *)(xs + m * x_stride + u * 16 + 8 * h);
        dst[0] = uint4_t{o0, o1, o2, o3};
        dst[1] = uint4_t{o4, o5, o6, o7};
        if (h == 0) sx[m * cu + u] = sum;
      }
    }
    __syncthreads();

    const int rounds = (nu + kSlots * UB - 1) / (kSlots * UB);
    for (int r = 0; r < rounds; ++r) {
      if (r) load_round(c0, c1, r);
#pragma unroll
      for (int i = 0; i < UB; ++i) {
        const int u = c0 + slot + kSlots * (r * UB + i);
        if (u < c1) {  // (no `break`: the loop must unroll completely, or the register arrays above turn into scratch memory)
          const float s_g = (float)__builtin_bit_cast(half_t, (uint16_t)sc[i]), z_g = zero_of(i);
          float acc[MT];
#pragma unroll
          for (int m = 0; m < MT; ++m) acc[m] = 0.f;
          const uint32_t *xu = xs + (u - c0) * 16;
          quad_dot<BITS, MT, 0>(w[i], xu, x_stride, acc);
          quad_dot<BITS, MT, 1>(w[i], xu, x_stride, acc);
          quad_dot<BITS, MT, 2>(w[i], xu, x_stride, acc);
          quad_dot<BITS, MT, 3>(w[i], xu, x_stride, acc);
#pragma unroll
          for (int m = 0; m < MT; ++m) y[m] += s_g * (acc[m] - z_g * sx[m * cu + (u - c0)]);
        }
      }
    }
  }

  // ---- parities and waves: fixed-order sum through LDS (the staged activations are dead) -----------------------------------------------
  __syncthreads();
  float *red = (float *)smem;
#pragma unroll
  for (int m = 0; m < MT; ++m) red[(slot * MT + m) * kCols + col] = y[m];
  __syncthreads();
  float *blk = red + kSlots * MT * kCols;  // [MT][16] sums of this block
  const int S = p.ksplit;
  for (int i = tid; i < MT * kCols; i += kNW * 64) {
    const int c = i % kCols, m = i / kCols;
    float v = 0.f;
#pragma unroll
    for (int q = 0; q < kSlots; ++q) v += red[(q * MT + m) * kCols + c];
    blk[i] = v;
  }
  __syncthreads();
  int &s_ticket = *(int *)(blk + MT * kCols);
  if (S > 1) {
    // fp32 slab [ksplit][M][N]: write-through stores, drained; one relaxed agent-scope ticket per column block; the last arriver sums
    // the S slabs in fixed order (deterministic) and re-arms the counter
    for (int i = tid; i < p.M * kCols; i += kNW * 64) {
      const int c = i % kCols, m = i / kCols;
      if (nb * kCols + c < p.N) st_sc1(p.slabs + ((size_t)kb * p.M + m) * p.N + nb * kCols + c, blk[m * kCols + c]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(p.counters + nb, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != S - 1) return;
    for (int i = tid; i < p.M * kCols; i += kNW * 64) {
      const int c = i % kCols, m = i / kCols;
      float v = 0.f;
      if (nb * kCols + c < p.N)
        for (int sp = 0; sp < S; ++sp) v += ld_sc1(p.slabs + ((size_t)sp * p.M + m) * p.N + nb * kCols + c);
      blk[m * kCols + c] = v;
    }
    if (tid == 0) __hip_atomic_store(p.counters + nb, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
  }
  for (int i = tid; i < p.M * kCols; i += kNW * 64) {
    const int c = i % kCols, m = i / kCols, nn = nb * kCols + c;
    if (nn >= p.N) continue;
    float v = blk[m * kCols + c];
    if (p.bias) v += (float)p.bias[nn];
    if (p.act_bf16) ((uint16_t *)p.y)[(size_t)m * p.N + nn] = f32_to_bf16(v);
    else ((half_t *)p.y)[(size_t)m * p.N + nn] = (half_t)v;
  }
}

// launch geometry of both forms: column blocks, the units of x staged per chunk, dynamic LDS, grid (p.ksplit is dropped to 1 without a
// workspace)
constexpr int row_tile(int M) { return M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : (M <= 8 ? 8 : 16))); }  // the MT instantiation that serves M rows
struct Geometry { int mt, grid; size_t lds; };
inline Geometry geometry(BitGemvParams &p) {
  Geometry g;
  g.mt = row_tile(p.M);
  p.n_col_blocks = (p.N + kCols - 1) / kCols;
  if (p.ksplit < 1 || !p.slabs || !p.counters) p.ksplit = 1;
  const int U = p.K / 32, per_block = (U + p.ksplit - 1) / p.ksplit;
  const int fit = kXsBytes / (g.mt * 68);  // units whose staged activations (64 B per row) and sums (4 B) fit the LDS budget
  p.chunk_units = per_block < fit ? per_block : fit;
  const size_t x_bytes = (size_t)g.mt * p.chunk_units * 68, red_bytes = (size_t)(kSlots + 1) * g.mt * kCols * 4 + 16;
  g.lds = x_bytes > red_bytes ? x_bytes : red_bytes;
  g.grid = p.n_col_blocks * p.ksplit;
  return g;
}

}  // namespace bg
}  // namespace qllm
