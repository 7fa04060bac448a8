// bitpanel: fused dequant + GEMM for mid-batch calls (17 <= M <= 512) on the reference's row-stream layouts READ IN PLACE (GPTQ / HQQ
// qweight i32 [K / 32 * bits][N]) at every width from 2 to 8 bits -- the widths the strip-major native layout and panel.hip do not take
// (2, 5, 6, 7, 8), and the 3- / 4-bit layers the planner refuses (ragged N).  Until now such a call wrote the whole fp16 W with
// qllm_dequant (2 K N bytes), read it back in a dense GEMM and paid a launch boundary, where the packed words are bits / 16 of that.
// Reached through qllm_linear_forward_bitpanel only: the planner, its routes and qllm_plan_describe do not know it.  (More than 512 rows --
// and, by measurement, the row counts from which every 128-row block rebuilding its panel's fragments loses: bitgemm.hip.)
//
//   * block = a panel of 64 columns (wave w: columns 16 w .. 16 w + 15) x a K range (all of K, or one of S splits when the panels
//     alone leave CUs idle) x a row block of up to 128 rows: MT = 2, 4 or 8 row tiles of v_mfma_f32_16x16x32_f16.  Calls of more
//     than 128 rows have ceil(M / 128) row blocks of eight row tiles as a grid dimension; the block ids are ordered so that the row
//     blocks of one (panel, split) follow each other at a distance of 8 ids -- ids 8 apart share an XCD, hence an L2 -- and re-read
//     the panel's words from there.  Rows past M are zero-filled (out-of-range buffer addresses) and never stored; columns past N
//     re-read the last column and store nothing;
//   * A: the x tile of 8 k-steps goes into LDS once per block by LDS-DMA, in the XOR-swizzled [k-pair][row tile][16 rows][128 B]
//     image of panel.hip / strip_dma.hpp (lds_row_swizzle), double-buffered; all four waves read the same ds_read_b128 fragments.
//     bf16 activations are converted to fp16 in place when a tile has landed (as bitgemv does while it stages) and give a bf16 y;
//   * B: one unit (32 k of one column = `bits` words) is one MFMA k-step.  Lane (g = lane >> 4, i = lane & 15) needs the 8 fields at
//     stream bits [8 bits g, 8 bits (g + 1)) of column i: a window of at most 64 bits over 1 (2, 4 bits), 2 (3, 5, 6, 8) or 3 (7)
//     words.  Two ingests are built (template flag LDSW, knob QLLM_BITPANEL_LDS; A/B in profiles/bitpanel.md).  Default: the lane
//     loads exactly those words straight into registers (four 64-byte segments per instruction, the other half of each 128-byte line
//     is the neighbouring wave's; a tile ahead, the second register set).  The other: the block moves the tile's word rows into LDS
//     with full-line loads (one 256-byte row x 64 columns per wave instruction, LDS-DMA, double-buffered) and the lane reads its words
//     from there.  Either way the lane funnel-shifts them to a window that starts at bit 0 (v_alignbit) and builds each pair of
//     fields with the idiom of bitgemv_kernel.hpp's pair_of: shift / alignbit, mask, OR with kMagic, minus 1024, minus z.  Fragments
//     exist in registers only -- never as fp16 in LDS or in memory (the pipeline panel.hip's header measures at 1.4 TB/s);
//   * numerics: panel.hip's contract.  The fragment holds the exact integers q - z (packed / symmetric zero points: q and q - z are
//     integers below 2048) or q - z with the reference's one fp16 rounding (fp16 zero points); one fp32 y += s_g * acc_g per group
//     and accumulator; no sum-of-x bookkeeping; y is rounded once.  ONE code path for the three zero-point kinds (no stores under a
//     per-kind branch: DESIGN.md 3.7);
//   * split-K: the protocol of panel.hip / skinny.hip -- fp32 partial panels through write-through slabs, one relaxed agent-scope
//     ticket per (panel, row block), the last arriver sums in split order and re-arms the counter: deterministic.  A split is a whole
//     number of groups where the group size allows it.  Without a workspace there is no split;
//   * epilogue through LDS: 16-byte row-contiguous stores where N % 8 == 0 and y is 16-byte aligned, else two-byte stores.
// K % 32 == 0, group_size % 32 == 0 (any such size: the group walk is a counter, not a template parameter), any N >= 1.
#include "kernels.hpp"
#include "planner.hpp"

namespace qllm {

namespace {

constexpr int kBpWaves = 4;
constexpr int kBpKTS = 8;    // k-steps (units) per K-tile
constexpr int kBpCols = 64;  // columns of a panel
typedef __attribute__((address_space(3))) void lds_void_t;

// words of a unit that hold a lane group's 8 fields
__host__ __device__ constexpr int window_words(int bits) { return bits == 7 ? 3 : ((bits == 2 || bits == 4) ? 1 : 2); }

// pair P (fields 2 P, 2 P + 1 of the lane's 8: natural k order) as (1024 + q_a, 1024 + q_b) from the 64-bit window (lo, hi) whose bit 0
// is the lane's first field -- the idiom of bg::pair_of with compile-time positions
template <int BITS, int P>
__device__ __forceinline__ uint32_t magic_pair(uint32_t lo, uint32_t hi) {
  constexpr uint32_t mask = (1u << BITS) - 1u;
  constexpr int o = 2 * P * BITS;
  uint32_t win;
  if constexpr (o + 2 * BITS <= 32) win = lo >> o;
  else if constexpr (o >= 32) win = hi >> (o - 32);
  else win = __builtin_amdgcn_alignbit(hi, lo, o);
  return (win & mask) | ((win << (16 - BITS)) & (mask << 16)) | kMagic;
}

// LDSW: how the packed words reach the lanes.  false: every lane loads its window words straight into registers (8 x NWIN loads per
// wave and tile, four 64-byte segments each).  true: the block moves the tile's word rows -- [8 x BITS rows][64 columns], one full
// 256-byte row per wave instruction -- into LDS by LDS-DMA next to the x tile (double-buffered: BITS x 4 KB more LDS) and every lane
// reads its window words from there (ds_read_b32) a k-step ahead.  The fragment build is the same.  QLLM_BITPANEL_LDS chooses;
// profiles/bitpanel.md has the A/B.
template <int BITS, int MT, bool LDSW>
__global__ __launch_bounds__(kBpWaves * 64) void bitpanel_kernel(const BitPanelParams p) {
  constexpr int NW = kBpWaves, KTS = kBpKTS, KP = KTS / 2;
  constexpr int TILE_BYTES = KP * MT * 2048;  // one A buffer: [k-pair][row tile][16 rows][128 B]
  constexpr int PPW = KP * MT * 2 / NW;       // 1 KB DMA pieces per wave and tile
  constexpr int NMT = MT / 2;                 // distinct row tiles among a wave's pieces
  constexpr int NWIN = window_words(BITS);
  constexpr int WTILE_BYTES = KTS * BITS * 256;  // LDSW: one buffer of word rows, [8 BITS rows][64 columns] dwords
  constexpr int RPW = KTS * BITS / NW;        // LDSW: word rows per wave and tile
  constexpr int EPS = kBpCols + 8;            // epilogue row stride in halves (16-byte aligned, bank-spread)
  static_assert(MT == 2 || MT == 4 || MT == 8, "row tiles");
  // A[2][TILE_BYTES] (the epilogue re-uses it) | LDSW: W[2][WTILE_BYTES].  (No static LDS: the opt-in to 160 KiB of dynamic LDS is refused next to any.)
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g = lane >> 4, i = lane & 15;
  const int S = p.split_k, RB = p.row_blocks;
  // block id -> (panel, split, row block): ids 8 apart share an XCD, so the row blocks of one (panel, split) sit 8 ids apart
  const int slot = (int)blockIdx.x & 7, rest = (int)blockIdx.x >> 3;
  const int rb = rest % RB, pk = (rest / RB) * 8 + slot;
  if (pk >= p.n_panels * S) return;  // (the last group of 8 may be ragged; before any barrier)
  const int ksplit = pk % S, panel = pk / S;
  const int tile_id = panel * RB + rb;  // slab / counter index
  const int M = p.M, N = p.N, T = p.K >> 5;
  const int row0 = rb * 128;
  const int t0 = ksplit * p.chunk, t1 = min(t0 + p.chunk, T);  // this block's units (t0 is even: whole k-pairs of the A image)
  const int tiles = t1 > t0 ? (t1 - t0 + KTS - 1) / KTS : 0;
  const int spg = p.group_size >> 5;  // units per group
  const int Gmax = (p.K + p.group_size - 1) / p.group_size - 1;

  // ---- addressing: raw buffer loads (range-checked), per-lane byte offset (loop constant) + wave-uniform scalar offset ----------
  const int n0 = panel * kBpCols;
  const int n = n0 + wave * 16 + i, nc = min(n, N - 1);
  const int zk = p.zero_kind;
  const int zwords = (N * BITS) >> 5;  // packed zero points: words per group row
  const int zbytes = (zk == ZK_PACKED) ? (Gmax + 1) * zwords * 4 : (Gmax + 1) * N * 2;  // (symmetric layers re-read their scales)
  const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void *)p.qweight, 0, T * BITS * N * 4, 0x00020000);
  const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void *)p.scales, 0, (Gmax + 1) * N * 2, 0x00020000);
  const auto rs_z = __builtin_amdgcn_make_buffer_rsrc((zk == ZK_SYM) ? (void *)p.scales : (void *)p.qzeros, 0, zbytes, 0x00020000);
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void *)p.x, 0, M * p.K * 2, 0x00020000);
  // the lane's window: stream bits [8 BITS g, 8 BITS (g + 1)) of the unit = words w0 .. w0 + NWIN - 1 (clamped into the unit: a word
  // past the window is loaded by some lane groups and never used), shifted down by sh
  const int wbit = 8 * BITS * g, w0 = wbit >> 5;
  const uint32_t sh = (uint32_t)(wbit & 31);
  int lane_w[NWIN];
#pragma unroll
  for (int t = 0; t < NWIN; ++t) lane_w[t] = (min(w0 + t, BITS - 1) * N + nc) * 4;
  const int lane_s = nc * 2;
  // LDSW: the DMA's column (lane l moves column n0 + l of a word row) and the lane's window words inside a unit's rows in LDS
  const int dma_col = min(n0 + lane, N - 1) * 4;
  int lane_wl[NWIN];
#pragma unroll
  for (int t = 0; t < NWIN; ++t) lane_wl[t] = min(w0 + t, BITS - 1) * 256 + (wave * 16 + i) * 4;
  // zero points: packed -- the field at bit nc BITS of the group's row may straddle into a second word; fp16 -- the dword holding the
  // half (N is even); symmetric -- a scale word, loaded and never decoded
  const int zbit = nc * BITS, zw = zbit >> 5;
  const int lane_z0 = (zk == ZK_PACKED) ? zw * 4 : ((zk == ZK_F16) ? (nc >> 1) * 4 : 0);
  const int lane_z1 = (zk == ZK_PACKED) ? min(zw + 1, zwords - 1) * 4 : lane_z0;
  const int zrow = (zk == ZK_PACKED) ? zwords * 4 : ((zk == ZK_F16) ? N * 2 : 0);  // bytes per group row
  const uint32_t zsh = (uint32_t)(zbit & 31);
  // A pieces of this wave: q = wave + NW r -> half h = wave & 1 (rows 8 h .. 8 h + 7 of the row tile), row tile (q >> 1) % MT,
  // k-pair (q >> 1) / MT; lane l moves the 16-byte chunk (l & 7) ^ swizzle of row 8 h + (l >> 3)
  const int ar = 8 * (wave & 1) + (lane >> 3);
  const int achunk = (lane & 7) ^ lds_row_swizzle(ar);
  const int asub = achunk >> 2;  // which unit of the k-pair the chunk belongs to
  // M K 2 < 2^30 (the entry checks): kOut, and kOut twice over, are past the buffer and below 2^32 (unsigned arithmetic)
  constexpr uint32_t kOut = 0x40000000u;
  uint32_t a_voff[NMT];
#pragma unroll
  for (int u = 0; u < NMT; ++u) {
    const int mt = ((wave >> 1) + 2 * u) % MT;
    const int row = row0 + 16 * mt + ar;
    a_voff[u] = row < M ? (uint32_t)(row * p.K * 2 + (achunk << 4)) : kOut;
  }
  int a_rd[2];  // fragment read of k-step parity e: logical chunk 4 e + g of row i
#pragma unroll
  for (int e = 0; e < 2; ++e) a_rd[e] = i * 128 + (((4 * e + g) ^ lds_row_swizzle(i)) << 4);

  uint32_t w[2][LDSW ? 1 : KTS][NWIN], zr0[2][KTS], zr1[2][KTS];
  half_t sc[2][KTS];
  float4_t yacc[MT], gacc[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) yacc[mt] = gacc[mt] = float4_t{0.f, 0.f, 0.f, 0.f};
  // the group walk: two counters each for the loads (a tile ahead) and for the arithmetic
  int rq_g = t0 / spg, rq_pos = t0 - rq_g * spg, cp_pos = rq_pos;
  half_t cur_nz = (half_t)0.f;  // the running group's minus zero point and scale
  float cur_sf = 0.f;

  // tile kt: activation pieces -> buffer kt & 1 (units past the block's range and rows past M: zeros), per unit its window words and
  // per group its scale and zero-point words -> register set `set` (units past K: the last unit's, multiplied by zeros)
  auto request = [&](const int kt, const int set) __attribute__((always_inline)) {
    const int tb = t0 + kt * KTS;
    // (the buffer's offset is made opaque: the pieces' LDS addresses are then formed where they are used -- hoisted out of the tile loop,
    //  two buffers x PPW of them spill scalar registers)
    int boff = (kt & 1) * TILE_BYTES;
    asm volatile("" : "+s"(boff));
    uint8_t *dstb = smem + boff;
#pragma unroll
    for (int r = 0; r < PPW; ++r) {
      const int q = wave + NW * r;                     // (wave-uniform)
      const int kp = 2 * r / MT;                       // == (q >> 1) / MT = ((wave >> 1) + 2 r) / MT: wave >> 1 is 0 or 1, MT is even
      // live units of the k-pair (wave-uniform): 2 or more; 1 (an odd K / 32 only): the chunks of its second unit go out of range; none:
      // the whole pair does.  The out-of-range value goes into the per-lane offset, as in panel.hip; the scalar offset stays inside a row
      const int left = t1 - tb - 2 * kp;
      const uint32_t vo = a_voff[r % NMT] + (left <= 0 ? kOut : (uint32_t)asub * (left == 1 ? kOut : 0u));
      const int so = (tb + 2 * kp) * 64;               // byte offset of the k-pair inside a row
      lds_void_t *dst = (lds_void_t *)(dstb + q * 1024);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, dst, 16, (int)vo, so, 0, 0);
      __builtin_amdgcn_sched_barrier(0);  // (keeps every load's scalar offsets next to it: hoisted, they spill scalar registers)
    }
    if constexpr (LDSW) {
      // word row wave + NW r of the tile (wave-uniform): running offsets, one add and one min per row (products formed per row get hoisted
      // and spill scalar registers); rows past K: the last row, multiplied by zeros
      int dcur = 2 * TILE_BYTES + (kt & 1) * WTILE_BYTES + wave * 256;
      int scur = (tb * BITS + wave) * (N * 4);
      const int slast = (T * BITS - 1) * (N * 4), sstep = NW * N * 4;
      asm volatile("" : "+s"(dcur), "+s"(scur));
#pragma unroll
      for (int r = 0; r < RPW; ++r) {
        lds_void_t *dst = (lds_void_t *)(smem + dcur);
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_w, dst, 4, dma_col, min(scur, slast), 0, 0);
        dcur += NW * 256;
        scur += sstep;
        asm volatile("" : "+s"(dcur), "+s"(scur));
      }
    }
#pragma unroll
    for (int s = 0; s < KTS; ++s) {
      const int u = min(tb + s, T - 1), G = min(rq_g, Gmax);
      const int so = u * (BITS * N * 4);
      if constexpr (!LDSW) {
#pragma unroll
        for (int t = 0; t < NWIN; ++t) w[set][s][t] = __builtin_amdgcn_raw_buffer_load_b32(rs_w, lane_w[t], so, 0);
      }
      // scale and zero-point words: once per group and tile, with the group's first unit of the tile (wave-uniform branch; the
      // arithmetic reads them under the same condition, every index a compile-time constant)
      if (s == 0 || rq_pos == 0) {
        sc[set][s] = __builtin_bit_cast(half_t, __builtin_amdgcn_raw_buffer_load_b16(rs_s, lane_s, G * N * 2, 0));
        zr0[set][s] = __builtin_amdgcn_raw_buffer_load_b32(rs_z, lane_z0, G * zrow, 0);
        zr1[set][s] = __builtin_amdgcn_raw_buffer_load_b32(rs_z, lane_z1, G * zrow, 0);
      }
      if (++rq_pos == spg) { rq_pos = 0; ++rq_g; }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // One K-tile.  The fragments of k-step s + 1 are read before the MFMAs of k-step s are issued (the order is pinned, as in panel.hip).
  auto compute = [&](const int kt, const int set) __attribute__((always_inline)) {
    const uint8_t *ab = smem + (kt & 1) * TILE_BYTES;
    const int tb = t0 + kt * KTS;
    uint4_t ar4[2][MT];
    auto read_a = [&](const int s, uint4_t (&dst)[MT]) __attribute__((always_inline)) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) dst[mt] = *(const uint4_t *)(ab + ((s >> 1) * MT + mt) * 2048 + a_rd[s & 1]);
    };
    const uint8_t *wb = smem + 2 * TILE_BYTES + (kt & 1) * WTILE_BYTES;
    uint32_t wr[2][NWIN];
    auto read_w = [&](const int s, uint32_t (&dst)[NWIN]) __attribute__((always_inline)) {
#pragma unroll
      for (int t = 0; t < NWIN; ++t) dst[t] = *(const uint32_t *)(wb + s * (BITS * 256) + lane_wl[t]);
    };
    read_a(0, ar4[0]);
    if constexpr (LDSW) read_w(0, wr[0]);
#pragma unroll
    for (int s = 0; s < KTS; ++s) {
      if (s + 1 < KTS) read_a(s + 1, ar4[(s + 1) & 1]);
      if constexpr (LDSW) { if (s + 1 < KTS) read_w(s + 1, wr[(s + 1) & 1]); }
      __builtin_amdgcn_sched_barrier(0);
      // the group's scale and minus its zero point as fp16 -- the integer (packed / symmetric: exact) or the stored half -- decoded
      // with the group's first unit of the tile
      if (s == 0 || cp_pos == 0) {
        half_t zh;
        if (zk == ZK_F16) {
          zh = __builtin_bit_cast(half_t, (uint16_t)((nc & 1) ? (zr0[set][s] >> 16) : zr0[set][s]));
        } else if (zk == ZK_SYM) {
          zh = (half_t)(float)(1 << (BITS - 1));
        } else {
          const uint32_t field = __builtin_amdgcn_alignbit(zr1[set][s], zr0[set][s], zsh);  // (zr1 == zr0 only when the field ends inside its word)
          zh = (half_t)(float)((field + (uint32_t)p.add_zero_bias) & ((1u << BITS) - 1u));
        }
        cur_nz = -zh;
        cur_sf = (float)sc[set][s];
      }
      const half2_t nz = splat2(cur_nz), m1024 = splat2((half_t)-1024.f);
      // the window, shifted to bit 0
      uint32_t ww[NWIN];
#pragma unroll
      for (int t = 0; t < NWIN; ++t) ww[t] = LDSW ? wr[s & 1][t] : w[set][LDSW ? 0 : s][t];
      uint32_t lo, hi = 0;
      if constexpr (NWIN == 1) {
        lo = ww[0] >> sh;
      } else {
        lo = __builtin_amdgcn_alignbit(ww[1], ww[0], sh);
        if constexpr (NWIN == 2) hi = ww[1] >> sh;
        else hi = __builtin_amdgcn_alignbit(ww[2], ww[1], sh);
      }
      // (1024 + q) - 1024 = q: exact; q - z: exact for integer z, one rounding for an fp16 z (the reference's own)
      const half2_t b0 = (as_h2(magic_pair<BITS, 0>(lo, hi)) + m1024) + nz, b1 = (as_h2(magic_pair<BITS, 1>(lo, hi)) + m1024) + nz,
                    b2 = (as_h2(magic_pair<BITS, 2>(lo, hi)) + m1024) + nz, b3 = (as_h2(magic_pair<BITS, 3>(lo, hi)) + m1024) + nz;
      const half8_t bf = __builtin_bit_cast(half8_t, uint4_t{as_u32(b0), as_u32(b1), as_u32(b2), as_u32(b3)});
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
        gacc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, ar4[s & 1][mt]), bf, gacc[mt], 0, 0, 0);
      // the group (or the block's K range) ends with this unit: y += scale * sum x (q - z) (wave-uniform branch)
      // (cp_pos keeps step with the loads' rq_pos past the block's range too: the units there multiply zeros by a scale that was loaded)
      const bool group_end = ++cp_pos == spg;
      if (group_end) cp_pos = 0;
      if (group_end || tb + s + 1 == t1) {
        const float sf = cur_sf;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
          for (int q = 0; q < 4; ++q) yacc[mt][q] = __builtin_fmaf(sf, gacc[mt][q], yacc[mt][q]);
          gacc[mt] = float4_t{0.f, 0.f, 0.f, 0.f};
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  };

  // bf16 activations: the landed tile is converted to fp16 in place, once per block; one more barrier per tile
  auto convert_tile = [&](const int kt) __attribute__((always_inline)) {
    uint8_t *tb = smem + (kt & 1) * TILE_BYTES + threadIdx.x * 16;
#pragma unroll
    for (int r = 0; r < TILE_BYTES / (NW * 1024); ++r) {
      const uint4_t v = *(const uint4_t *)(tb + r * (NW * 1024));
      *(half8_t *)(tb + r * (NW * 1024)) = bf16x8_to_h8(v);
    }
  };

  // ---- main loop: [tile kt landed] barrier [request tile kt + 1 into the buffer / register set tile kt - 1 used] compute tile kt ----
  if (tiles > 0) request(0, 0);
  for (int kt = 0; kt < tiles; kt += 2) {  // the register sets alternate by name
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (kt + 1 < tiles) request(kt + 1, 1);
    if (p.act_bf16) { convert_tile(kt); __syncthreads(); }
    __builtin_amdgcn_sched_barrier(0);
    compute(kt, 0);
    __builtin_amdgcn_sched_barrier(0);
    if (kt + 1 < tiles) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (kt + 2 < tiles) request(kt + 2, 0);
      if (p.act_bf16) { convert_tile(kt + 1); __syncthreads(); }
      __builtin_amdgcn_sched_barrier(0);
      compute(kt + 1, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  __syncthreads();  // every wave is done with the A buffers: the epilogue re-uses them

  // ---- split-K: fp32 partial panels through write-through slabs + one ticket per (panel, row block); the last arriver sums in split order
  if (S > 1) {
    constexpr int WREGS = MT * 4;
    int &s_ticket = *(int *)(smem + MT * 4096);  // (past the epilogue's staging rows, MT x 2304 bytes; the A buffers are MT x 16 KB)
    const size_t slab_floats = (size_t)NW * WREGS * 64;
    float *slab = p.slabs + ((size_t)tile_id * S + ksplit) * slab_floats + (size_t)wave * (WREGS * 64) + lane;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) st_sc1(slab + (mt * 4 + r) * 64, yacc[mt][r]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) s_ticket = __hip_atomic_fetch_add(p.counters + tile_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != S - 1) return;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) yacc[mt] = float4_t{0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
      const float *src = p.slabs + ((size_t)tile_id * S + s) * slab_floats + (size_t)wave * (WREGS * 64) + lane;
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) yacc[mt][r] += ld_sc1(src + (mt * 4 + r) * 64);
    }
    if (threadIdx.x == 0) __hip_atomic_store(p.counters + tile_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }

  // ---- epilogue: + bias, round once, [row][panel columns] through LDS, row-contiguous stores ---------------------------------------
  uint16_t *ep = (uint16_t *)smem;
  {
    const int col = wave * 16 + i;
    const float bv = p.bias ? (float)p.bias[nc] : 0.f;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = yacc[mt][r] + bv;
        ep[(16 * mt + 4 * g + r) * EPS + col] = p.act_bf16 ? f32_to_bf16(v) : __builtin_bit_cast(uint16_t, (half_t)v);
      }
  }
  __syncthreads();
  const int rows = min(M - row0, MT * 16);
  uint16_t *yb = (uint16_t *)p.y + (size_t)row0 * N;
  if ((N & 7) == 0 && ((uintptr_t)p.y & 15) == 0) {  // (whole 16-byte chunks: a chunk is inside N or outside it)
    for (int c = threadIdx.x; c < rows * (kBpCols / 8); c += NW * 64) {
      const int row = c >> 3, col = (c & 7) * 8;
      if (n0 + col < N) *(uint4_t *)(yb + (size_t)row * N + n0 + col) = *(const uint4_t *)(ep + row * EPS + col);
    }
  } else {  // ragged edge / odd N: two-byte stores
    for (int c = threadIdx.x; c < rows * kBpCols; c += NW * 64) {
      const int row = c >> 6, col = c & 63;
      if (n0 + col < N) yb[(size_t)row * N + n0 + col] = ep[row * EPS + col];
    }
  }
}

template <int BITS, bool LDSW>
int launch_b(const BitPanelParams &p, int grid, size_t lds, hipStream_t stream) {
#define QLLM_BP(MT_)                                                                                              \
  {                                                                                                               \
    static DeviceLatch attr_done; /* per (kernel, device): the LDS opt-in is a per-device attribute */              \
    if (int rc = lds_optin(attr_done, (const void *)bitpanel_kernel<BITS, MT_, LDSW>)) return rc;                  \
    hipLaunchKernelGGL((bitpanel_kernel<BITS, MT_, LDSW>), dim3(grid), dim3(kBpWaves * 64), lds, stream, p);      \
  }                                                                                                               \
  break
  switch (p.mt) {
    case 2: QLLM_BP(2);
    case 4: QLLM_BP(4);
    default: QLLM_BP(8);
  }
#undef QLLM_BP
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace

// what the kernel takes apart from the row count (bitgemv_ok's shapes, with 32-bit byte offsets): NULL, or why not
const char *bitpanel_refusal(const qllm_weight_t &w) {
  if (w.layout != QLLM_LAYOUT_GPTQ && w.layout != QLLM_LAYOUT_HQQ) return "the layout must be GPTQ or HQQ (row-stream words in place)";
  if (w.bits < 2 || w.bits > 8) return "bits must be 2..8";
  if (w.K % 32 != 0) return "K must be a multiple of 32";
  if (w.group_size % 32 != 0) return "group_size must be a multiple of 32";
  if (w.N < 1) return "N must be at least 1";
  if (w.layout == QLLM_LAYOUT_HQQ && (w.N % 2 != 0 || (uintptr_t)w.qzeros % 4)) return "fp16 zero points need an even N and 4-byte alignment";
  if ((uintptr_t)w.qweight % 4 || (uintptr_t)w.scales % 2 || (uintptr_t)w.qzeros % 4 || (uintptr_t)w.bias % 2) return "qweight / qzeros must be 4-byte, scales / bias 2-byte aligned";
  if ((double)w.K * w.N * w.bits / 8 >= 2147483648.0 || (double)kBitPanelMaxM * w.K * 2 >= 1073741824.0) return "the packed words must be below 2 GiB and 512 rows of x below 1 GiB";
  return nullptr;
}

// ONE function for the launch and for qllm_bitpanel_describe / qllm_bitpanel_workspace_bytes.  `ws_bytes`: bytes of a usable workspace
// (0: none -> no split).  Split K until the launch covers the CUs: at least two K-tiles per split, at most 16 splits, whole groups
// (and whole k-pairs) per split.
BitPanelGeom bitpanel_geometry(const qllm_weight_t &w, int M, size_t ws_bytes) {
  BitPanelGeom g;
  g.mt = M <= 32 ? 2 : (M <= 64 ? 4 : 8);
  g.row_blocks = (M + 127) / 128;
  g.n_panels = (w.N + kBpCols - 1) / kBpCols;
  const int T = w.K / 32, spg = w.group_size / 32;
  const int blocks = g.n_panels * g.row_blocks;
  int S = compute_units() / blocks;
  const int by_len = T / (2 * kBpKTS);
  S = S > 16 ? 16 : S;
  S = S > by_len ? by_len : S;
  S = S < 1 ? 1 : S;
  const int even_T = (T + 1) / 2 * 2;
  auto chunk_for = [&](int s) {
    int align = spg % 2 == 0 ? spg : 2 * spg;
    if (align > even_T) align = even_T;  // (one group spans all of K: whole k-pairs is all that is left to keep)
    return ((T + s - 1) / s + align - 1) / align * align;
  };
  g.chunk = chunk_for(S);
  g.split_k = (T + g.chunk - 1) / g.chunk;
  g.slab_bytes = g.split_k > 1 ? (size_t)blocks * g.split_k * g.mt * 4096 : 0;  // [panel x row block][split][4 waves x MT x 4 x 64] fp32
  if (g.split_k > 1 && (ws_bytes < kCounterBytes + g.slab_bytes || blocks > (int)(kCounterBytes / sizeof(int)))) {  // (the counter page every route shares)
    g.split_k = 1;
    g.chunk = even_T;
    g.slab_bytes = 0;
  }
  g.lds_words = knob("QLLM_BITPANEL_LDS", 0) ? 1 : 0;  // the ingest of the packed words (0: direct register loads, the measured default)
  g.lds = (size_t)2 * (kBpKTS / 2) * g.mt * 2048 + (g.lds_words ? (size_t)2 * kBpKTS * w.bits * 256 : 0);
  g.grid = (g.n_panels * g.split_k + 7) / 8 * 8 * g.row_blocks;
  return g;
}

int launch_bitpanel(const BitPanelParams &p, const BitPanelGeom &g, hipStream_t stream) {
  switch (p.bits) {
    case 2: return g.lds_words ? launch_b<2, true>(p, g.grid, g.lds, stream) : launch_b<2, false>(p, g.grid, g.lds, stream);
    case 3: return g.lds_words ? launch_b<3, true>(p, g.grid, g.lds, stream) : launch_b<3, false>(p, g.grid, g.lds, stream);
    case 4: return g.lds_words ? launch_b<4, true>(p, g.grid, g.lds, stream) : launch_b<4, false>(p, g.grid, g.lds, stream);
    case 5: return g.lds_words ? launch_b<5, true>(p, g.grid, g.lds, stream) : launch_b<5, false>(p, g.grid, g.lds, stream);
    case 6: return g.lds_words ? launch_b<6, true>(p, g.grid, g.lds, stream) : launch_b<6, false>(p, g.grid, g.lds, stream);
    case 7: return g.lds_words ? launch_b<7, true>(p, g.grid, g.lds, stream) : launch_b<7, false>(p, g.grid, g.lds, stream);
    case 8: return g.lds_words ? launch_b<8, true>(p, g.grid, g.lds, stream) : launch_b<8, false>(p, g.grid, g.lds, stream);
  }
  return set_error(QLLM_ERR_UNSUPPORTED, "bitpanel: bits must be 2..8 (got %d)", p.bits);
}

}  // namespace qllm
