// bitgemm: fused dequant + prefill GEMM (M >= 129) on the reference's row-stream layouts READ IN PLACE (GPTQ / HQQ qweight i32
// [K / 32 * bits][N]) at every width from 2 to 8 bits: the widths gemm3.hip does not take (2, 5, 6, 7, 8) and the 3- / 4-bit layers
// gemm3_ok refuses (N % 128 != 0).  Above bitpanel's rows such a call used to write the whole fp16 W with qllm_dequant (2 K N bytes),
// read it back in a dense GEMM and pay two launches, on every forward call.  Reached through qllm_linear_forward_bitgemm only: the
// planner, its routes and qllm_plan_describe do not know it.
//
// The structure is gemm3.hip's LAYOUT 2 / MW = 8 form, copied (nothing is shared through headers, so that gemm3's object stays what it
// is): block tile 256 x 128 x 64, twelve waves.
//   * waves 0-7, "matrix": 64 x 64 each = 2 x 2 tiles of v_mfma_f32_32x32x16_f16.  The x tile arrives by LDS-DMA into a 3-deep ring
//     (lds_row_swizzle applied to the SOURCE address), 4 pieces per wave and k-tile, one between the two halves of every sub-step's
//     MFMAs; fragment reads are pinned a sub-step ahead with sched_barrier; a counted vmcnt(4) sits in front of the raw s_barrier.
//     These waves issue no other vector memory operation and nothing is conditional around a load (gemm3.hip: a branch there
//     collapses the counted vmcnt to vmcnt(0)).  Rows past M re-read row M - 1 and are never stored;
//   * waves 8-11, "dequant": thread t owns column n0 + (t & 127) and the unit t >> 7 of the k-tile (a unit = 32 k of one column =
//     BITS consecutive word rows; t >> 7 is wave-uniform).  Raw buffer loads with loop-constant per-lane offsets, the k-tile and the
//     group advance are scalar offsets; two register sets requested ~1.5 k-tiles ahead; loads past the last tile re-read it.  The 32
//     fields are cut from the 32 BITS-bit window in natural k order (shift / v_alignbit / mask with compile-time positions: the idiom
//     of bitpanel.hip's magic_pair; 8 bits: one v_perm_b32 per pair), every pair goes through deq_pair (common.hpp: exact for
//     q <= 1023), and four ds_write_b128 per thread land at tile_off(bcol, brow + r): the B image gemm3's LAYOUT 2 writes.  One
//     16-bit scale load and two zero-point words per thread and k-tile; the three zero-point kinds (packed with add_zero_bias, NULL:
//     z = 2^(BITS-1), fp16) run ONE code path.  The group of a unit is k0 / group_size kept as a counter: any group_size % 32 == 0,
//     group_size == K and a ragged last group included.  Columns >= N of the last column tile re-read column N - 1 (words, scale,
//     zero point: never past a buffer) and fill B columns nobody stores;
//   * LDS: A 3 x 32 KB + B 2 x 16 KB = 128 KB, dynamic only (bitpanel.hip: the opt-in is refused next to static LDS); one block
//     barrier per k-tile;
//   * epilogue: + bias (clamped read), one rounding, transposed through wave-private LDS, 16-byte row-contiguous stores; a chunk is
//     stored only if its first column is < N (N % 8 == 0: a chunk is inside N or outside it) and its row is < M;
//   * split-K: gemm3's protocol -- fp32 partial tiles to slabs with write-through stores, one relaxed agent-scope ticket per tile in
//     the shared counter page, the last arriver sums in split order and re-arms the counter.  The blocks' k-tile counts may differ by
//     one (KT0 = K / 64 * ksplit / S).  Block ids run through xcd_run;
//   * numerics: gemm3's fp16 contract.  The B tile holds fp16(q s) - fp16(z s), bit for bit what qllm_dequant produces; fp32 sums; y
//     rounded once (bf16 output: fp32 -> fp16 -> bf16, as gemm3); deterministic with and without a split.
// K % 64 == 0, N % 8 == 0, group_size % 32 == 0, fp16 x (bf16 callers convert first and ask for a bf16 y).
#include "kernels.hpp"

namespace qllm {

namespace {

constexpr int BM = 256, BN = 128, BK = 64;
constexpr int kATile = BM * BK, kBTile = BN * BK;  // halves per stage
constexpr int kMW = 8;                             // matrix waves; four dequant waves behind them
typedef float float16_t __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) void lds_void_t;

__device__ __forceinline__ int tile_off(int row, int slot) { return row * BK + ((slot ^ lds_row_swizzle(row)) & 7) * 8; }  // in halves

// fields F, F + 1 (F even) of a unit's 32 as (1024 + q_F, 1024 + q_F+1): every position is a compile-time constant
template <int BITS, int F>
__device__ __forceinline__ uint32_t unit_pair(const uint32_t (&w)[8]) {
  constexpr int o = F * BITS, wi = o >> 5, sh = o & 31;
  if constexpr (BITS == 8) {
    // bytes sh / 8 and sh / 8 + 1 of the word under the high byte of 1024.0: one v_perm_b32 (selector bytes 4..7 = the constant)
    constexpr uint32_t sel = 0x04000400u | (uint32_t)(sh >> 3) | ((uint32_t)((sh >> 3) + 1) << 16);
    return __builtin_amdgcn_perm(0x64646464u, w[wi], sel);
  } else {
    constexpr uint32_t mask = (1u << BITS) - 1u;
    uint32_t win;
    if constexpr (sh + 2 * BITS <= 32) win = w[wi] >> sh;
    else win = __builtin_amdgcn_alignbit(w[wi + 1], w[wi], sh);  // (a pair that crosses a word ends inside the unit: wi + 1 < BITS)
    return (win & mask) | ((win << (16 - BITS)) & (mask << 16)) | kMagic;
  }
}

// the 8 values of fields 8 R .. 8 R + 7, natural k order
template <int BITS, int R>
__device__ __forceinline__ half8_t unit_row(const uint32_t (&w)[8], const ColConst &cc) {
  const half2_t b0 = deq_pair(unit_pair<BITS, 8 * R>(w), cc), b1 = deq_pair(unit_pair<BITS, 8 * R + 2>(w), cc),
                b2 = deq_pair(unit_pair<BITS, 8 * R + 4>(w), cc), b3 = deq_pair(unit_pair<BITS, 8 * R + 6>(w), cc);
  return half8_t{b0.x, b0.y, b1.x, b1.y, b2.x, b2.y, b3.x, b3.y};
}

template <int BITS>
__global__ __launch_bounds__((kMW + 4) * 64) void bitgemm_kernel(const BitGemmParams p) {
  constexpr int MW = kMW;
  constexpr int AM = 2;         // 32-row MFMA tiles per matrix wave along M
  constexpr int WROWS = 64;     // rows per matrix wave
  constexpr int NP = 4;         // activation DMA pieces (8 rows x 128 B) per matrix wave and k-tile
  extern __shared__ __attribute__((aligned(16))) half_t smem[];
  half_t *As = smem;               // [3][256][64]  (LDS-DMA ring)
  half_t *Bs = smem + 3 * kATile;  // [2][128 n][64 k]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int N = p.N;
  const int tiles_n = (N + BN - 1) / BN;
  const int tiles_all = ((p.M + BM - 1) / BM) * tiles_n;  // (a ragged last column tile counts as one)
  auto xcd_run = [](int b, int n) {  // each XCD (block id % 8) walks a contiguous run of the n blocks
    const int q = n / 8, r = n % 8, xcd = b % 8, idx = b / 8;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
  };
  const int S = __builtin_amdgcn_readfirstlane(p.split_k);
  const int bid = xcd_run(blockIdx.x, tiles_all * S);
  const int ksplit = bid % S, tile_id = bid / S;
  // n fastest: an XCD's run shares activation rows, which stay in its L2 while the small packed weights stream
  const int tm = tile_id / tiles_n, tn = tile_id % tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  // this block's k-tiles [KT0, KT0 + KT): the S blocks of a tile own k-tile counts that differ by one at most
  const int KT0 = p.K / BK * ksplit / S;
  const int KT = p.K / BK * (ksplit + 1) / S - KT0;

  if (wave >= MW) {
    // ================================================= dequant waves ==================================================
    const int t = tid - MW * 64;  // 0..255
    const int unit = __builtin_amdgcn_readfirstlane(t >> 7);  // which 32 k of the k-tile (waves 8, 9: 0; waves 10, 11: 1)
    const int bcol = t & 127, brow = 4 * unit;
    const int nB = min(n0 + bcol, N - 1);  // columns >= N re-read column N - 1; their B columns are never stored
    const int zk = p.zero_kind;
    const int Gn = (p.K + p.group_size - 1) / p.group_size;
    // zero points: packed -- the field at bit nB BITS of the group's row may straddle into a second word; fp16 -- the dword holding
    // the half (N is even); symmetric -- a scale word, loaded and never decoded
    const int zwords = (N * BITS) >> 5;
    const int zbit = nB * BITS, zw = zbit >> 5;
    const int voff_z0 = (zk == ZK_PACKED) ? zw * 4 : ((zk == ZK_F16) ? (nB >> 1) * 4 : 0);
    const int voff_z1 = (zk == ZK_PACKED) ? min(zw + 1, zwords - 1) * 4 : voff_z0;
    const int zrow = (zk == ZK_PACKED) ? zwords * 4 : ((zk == ZK_F16) ? N * 2 : 0);  // bytes per group row
    const int zbytes = (zk == ZK_PACKED) ? Gn * zwords * 4 : Gn * N * 2;              // (symmetric layers re-read their scales)
    const uint32_t zsh = (uint32_t)(zbit & 31);
    struct BSet {
      uint32_t w[8];  // BITS of them are used
      uint32_t sraw, z, z2;
    };
    BSet bset[2];
    // buffer loads: per-lane byte offsets are loop constants, the k-tile / group advance is a scalar offset (SALU only)
    const int wrow_bytes = N * 4;
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void *)p.qweight, 0, (p.K >> 5) * BITS * wrow_bytes, 0x00020000);
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void *)p.scales, 0, Gn * N * 2, 0x00020000);
    const auto rs_z = __builtin_amdgcn_make_buffer_rsrc((zk == ZK_SYM) ? (void *)p.scales : (void *)p.qzeros, 0, zbytes, 0x00020000);
    const int ktile_bytes = 2 * BITS * wrow_bytes;  // word rows per k-tile: 2 units
    const int voff_w = nB * 4, voff_s = nB * 2;
    const int so_unit = unit * BITS * wrow_bytes;
    // the group walk: this wave's unit of the tile the NEXT load_b asks for is unit index 2 (KT0 + kt) + unit; the calls ask for
    // kt = 0, 1, 2, ... in order, so its group is a counter (gq, gpos) advanced by two units per call
    const int spg = p.group_size >> 5;  // units per group
    // (G is read back with readfirstlane where it is used: hipcc keeps the counter on the vector unit -- the division is expanded there --
    //  and a scalar offset held in a VGPR turns every load into a waterfall loop)
    int gq = (2 * KT0 + unit) / spg, gpos = (2 * KT0 + unit) - gq * spg;
    auto load_b = [&](int kt, BSet &bs) {
      const int ktc = KT0 + min(kt, KT - 1);
      const int so = ktc * ktile_bytes + so_unit;
#pragma unroll
      for (int r = 0; r < BITS; ++r) bs.w[r] = __builtin_amdgcn_raw_buffer_load_b32(rs_w, voff_w, so + r * wrow_bytes, 0);
      const int G = __builtin_amdgcn_readfirstlane(min(gq, Gn - 1));  // (past the block's last tile: a later group's, or the layer's last; the tile is never consumed)
      bs.sraw = __builtin_amdgcn_raw_buffer_load_b16(rs_s, voff_s, G * (N * 2), 0);
      bs.z = __builtin_amdgcn_raw_buffer_load_b32(rs_z, voff_z0, G * zrow, 0);
      bs.z2 = __builtin_amdgcn_raw_buffer_load_b32(rs_z, voff_z1, G * zrow, 0);
      gpos += 2;  // (scalar; spg >= 1: two steps at most)
      if (gpos >= spg) { gpos -= spg; ++gq; }
      if (gpos >= spg) { gpos -= spg; ++gq; }
    };
    auto store_b = [&](int stage, const BSet &bs) {
      half_t *Bb = Bs + stage * kBTile;
      const uint32_t zfield = __builtin_amdgcn_alignbit(bs.z2, bs.z, zsh);  // (z2 == z only when the field ends inside its word)
      const half_t zp = (half_t)(float)((zfield + (uint32_t)p.add_zero_bias) & ((1u << BITS) - 1u));
      const half_t zf = __builtin_bit_cast(half_t, (uint16_t)((nB & 1) ? (bs.z >> 16) : (bs.z & 0xffffu)));
      const half_t sc = __builtin_bit_cast(half_t, (uint16_t)bs.sraw);
      const ColConst cc = make_col_const(sc, (zk == ZK_PACKED) ? zp : ((zk == ZK_F16) ? zf : (half_t)(float)(1 << (BITS - 1))));
      *(half8_t *)(Bb + tile_off(bcol, brow + 0)) = unit_row<BITS, 0>(bs.w, cc);
      *(half8_t *)(Bb + tile_off(bcol, brow + 1)) = unit_row<BITS, 1>(bs.w, cc);
      *(half8_t *)(Bb + tile_off(bcol, brow + 2)) = unit_row<BITS, 2>(bs.w, cc);
      *(half8_t *)(Bb + tile_off(bcol, brow + 3)) = unit_row<BITS, 3>(bs.w, cc);
    };

    // Order of one iteration: [write B tile kt+1 from its register set] barrier [request tile kt+3 into that set].  A set is
    // requested right after the barrier that frees it and consumed two barriers later (~1.5 k-tiles of flight), and the only
    // vmcnt wait in the loop is the counted one in front of the stores (the younger set's loads stay in flight).  Nothing is
    // conditional around a load: past the last tile the loads re-read it and the stores fill a stage nobody reads again.
    load_b(0, bset[0]);
    load_b(1, bset[1]);
    __builtin_amdgcn_sched_barrier(0);
    store_b(0, bset[0]);
    __builtin_amdgcn_sched_barrier(0);
    load_b(2, bset[0]);
    __syncthreads();  // prologue barrier: B stage 0 holds tile 0
    for (int kt = 0; kt + 1 < KT; kt += 2) {  // two k-tiles per trip: the register sets alternate by name, no branch between them
      store_b(1, bset[1]);
      __syncthreads();  // barrier #kt
      load_b(kt + 3, bset[1]);
      __builtin_amdgcn_sched_barrier(0);
      store_b(0, bset[0]);
      __syncthreads();  // barrier #kt+1
      load_b(kt + 4, bset[0]);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (KT & 1) __syncthreads();  // odd number of k-tiles: barrier #KT-1 (the tile it would publish does not exist)
    __syncthreads();  // matches the matrix waves' barrier in front of their epilogue
    if (S > 1) {          // ... and the two around the split-K ticket
      __syncthreads();
      __syncthreads();
    }
    return;
  }

  // =================================================== matrix waves ===================================================
  const int wm = wave >> 1, wn = wave & 1;   // 4 (M) x 2 (N): rows wm*64.., columns wn*64..
  const int fr = lane & 31, fs = lane >> 5;  // fragment row (A: m, B: n) and k half of the 16-wide sub-step
  float16_t acc[AM][2];
#pragma unroll
  for (int a = 0; a < AM; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

  half8_t fa0[AM], fb0[2], fa1[AM], fb1[2];
  auto read_frags = [&](int sa, int sb, int ks, half8_t (&fa)[AM], half8_t (&fb)[2]) {
    const half_t *Ab = As + sa * kATile, *Bb = Bs + sb * kBTile;
#pragma unroll
    for (int b = 0; b < 2; ++b) fb[b] = *(const half8_t *)(Bb + tile_off(wn * 64 + b * 32 + fr, ks * 2 + fs));
#pragma unroll
    for (int a = 0; a < AM; ++a) fa[a] = *(const half8_t *)(Ab + tile_off(wm * WROWS + a * 32 + fr, ks * 2 + fs));
  };
  // ---- activation tile by LDS-DMA: this wave owns rows wave*32 .. +31 of the 256-row tile = 4 pieces of 8 rows x 128 B.
  // Piece q: lane l -> LDS row r = wave*32 + 8q + l/8, physical slot l%8, which holds logical 16-byte chunk (l%8) ^ swizzle(r).
  // Per-lane byte offsets into x are loop constants; the k-tile advance (128 B) is the scalar offset.
  const auto rs_x = __builtin_amdgcn_make_buffer_rsrc((void *)p.x, 0, (int)min((size_t)p.M * p.K * 2, (size_t)0x7fffffff), 0x00020000);
  int voff_x[NP];
#pragma unroll
  for (int q = 0; q < NP; ++q) {
    const int r = wave * (8 * NP) + 8 * q + (lane >> 3);
    const int grow = min(m0 + r, p.M - 1);  // rows past M re-read the last row; their outputs are never stored
    voff_x[q] = grow * p.K * 2 + (((lane & 7) ^ lds_row_swizzle(r)) << 4);
  }
  // one DMA piece (8 rows x 128 B of this wave's 32 rows) of k-tile kt into ring slot `slot`
  // (the builtin's operands are first copied into plain locals: called with template-dependent expressions, the HOST pass of
  //  hipcc silently fails to instantiate the whole kernel)
  const int rows_per_wave = 8 * NP;
  auto dma_piece = [&](int kt, int slot, int q) {
    const int so = (KT0 + min(kt, KT - 1)) * (BK * 2);
    const int vo = voff_x[q];
    lds_void_t *dst = (lds_void_t *)(As + slot * kATile + (wave * rows_per_wave + q * 8) * BK);
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs_x, dst, 16, vo, so, 0, 0);
  };
  // half of a sub-step's MFMAs: row tile h
  auto mfma_half = [&](const half8_t (&fa)[AM], const half8_t (&fb)[2], int h) {
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[h][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[h], fb[b], acc[h][b], 0, 0, 0);
  };

  __builtin_amdgcn_s_setprio(2);  // the matrix wave outranks its SIMD's dequant wave for issue slots
#pragma unroll
  for (int q = 0; q < NP; ++q) dma_piece(0, 0, q);
#pragma unroll
  for (int q = 0; q < NP; ++q) dma_piece(1, 1, q);
  asm volatile("s_waitcnt vmcnt(4)" ::: "memory");  // tile 0's pieces have landed (tile 1's still in flight)
  __builtin_amdgcn_s_barrier();                      // prologue barrier (the dequant waves' __syncthreads)
  dma_piece(2, 2, 0);
  read_frags(0, 0, 0, fa0, fb0);
  // The issue order is pinned (sched_barrier), as in gemm3.hip: left alone, hipcc sinks every fragment read to just above its first
  // use.  Between barrier #kt-1 and barrier #kt the wave requests the 4 pieces of tile kt+2 (slot (kt+2)%3, freed by barrier #kt-1):
  // piece 0 beside sub-step 3 of tile kt-1, pieces 1..3 beside sub-steps 0..2 of tile kt, each BETWEEN the two halves of the
  // sub-step's MFMAs.  At barrier #kt the pieces of tile kt+1 are older than those 4: vmcnt(4) retires exactly them.
#define BG_SB() __builtin_amdgcn_sched_barrier(0)
  int sa = 0;  // A ring slot of tile kt (kt % 3)
  for (int kt = 0; kt < KT; ++kt) {
    const int sb = kt & 1;
    const int sa1 = (sa == 2) ? 0 : sa + 1, sa2 = (sa == 0) ? 2 : sa - 1;  // slots of tiles kt+1, kt+2
    read_frags(sa, sb, 1, fa1, fb1);
    BG_SB();
    mfma_half(fa0, fb0, 0); BG_SB();
    dma_piece(kt + 2, sa2, 1); BG_SB();
    mfma_half(fa0, fb0, 1); BG_SB();  // sub-step 0
    read_frags(sa, sb, 2, fa0, fb0);
    BG_SB();
    mfma_half(fa1, fb1, 0); BG_SB();
    dma_piece(kt + 2, sa2, 2); BG_SB();
    mfma_half(fa1, fb1, 1); BG_SB();  // sub-step 1
    read_frags(sa, sb, 3, fa1, fb1);
    BG_SB();
    mfma_half(fa0, fb0, 0); BG_SB();
    dma_piece(kt + 2, sa2, 3); BG_SB();
    mfma_half(fa0, fb0, 1); BG_SB();  // sub-step 2
    // barrier #kt: my fragment reads of tile kt are complete (lgkmcnt(0)) and my DMA pieces of tile kt+1 have landed
    // (vmcnt(4): only tile kt+2's are still in flight).  After it: B stage sb and A slot sa are free, tile kt+1 is complete.
    asm volatile("s_waitcnt vmcnt(4) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    BG_SB();
    read_frags(sa1, sb ^ 1, 0, fa0, fb0);  // past the last tile: stages nobody uses
    BG_SB();
    mfma_half(fa1, fb1, 0); BG_SB();
    dma_piece(kt + 3, sa, 0); BG_SB();
    mfma_half(fa1, fb1, 1); BG_SB();  // sub-step 3
    sa = sa1;
  }
#undef BG_SB
  // (ragged last column tile: matrix waves whose 64 columns are all past N run the loop too -- their DMA pieces feed the other
  //  waves' rows -- and leave before the epilogue)
  const bool live = n0 + wn * 64 < N;
  __builtin_amdgcn_s_setprio(0);
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // stray DMA pieces past the last tile: land before the LDS is reused
  __builtin_amdgcn_s_barrier();                                // (matched by the dequant waves' final barrier)

  // ---- split-K: publish the fp32 partial tile; the last block to arrive sums the S partials in fixed order (deterministic).
  // Write-through (sc1) stores, every storing wave drains them, one relaxed agent-scope ticket per block, the last arriver reads
  // with sc1 loads and re-arms the counter.  Slab element (tile, split, wave, register, lane): 256 contiguous bytes per instruction.
  if (S > 1) {
    int &s_ticket = *(int *)(smem + 24 * 1024);  // past the epilogue's wave-private regions (8 x 4.5 KB)
    constexpr int WREGS = AM * 2 * 16;
    float *slab = p.slabs + ((size_t)tile_id * S + ksplit) * (size_t)(BM * BN) + (size_t)wave * (WREGS * 64) + lane;
#pragma unroll
    for (int a = 0; a < AM; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) st_sc1(slab + ((a * 2 + b) * 16 + r) * 64, acc[a][b][r]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(p.counters + tile_id, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != S - 1) return;
#pragma unroll
    for (int a = 0; a < AM; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;
    for (int sp = 0; sp < S; ++sp) {
      const float *src = p.slabs + ((size_t)tile_id * S + sp) * (size_t)(BM * BN) + (size_t)wave * (WREGS * 64) + lane;
#pragma unroll
      for (int a = 0; a < AM; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[a][b][r] += ld_sc1(src + ((a * 2 + b) * 16 + r) * 64);
    }
    if (tid == 0) __hip_atomic_store(p.counters + tile_id, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!live) return;  // (columns past N: no bias, no store; the block's last barrier is behind it)

  // ---- epilogue: + bias, round once, transpose through wave-private LDS, 16-byte row-contiguous stores ---------------------
  // C/D layout of 32x32 tiles: col = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  (All fragment reads that
  // matter completed before the last barrier; the stray ones above only fill registers.)
  half_t *ep = smem + wave * (32 * 72);  // 32 rows x 64 cols, row stride 72 halves (144 B)
  float bv[2];
#pragma unroll
  for (int b = 0; b < 2; ++b) bv[b] = p.bias ? (float)p.bias[min(n0 + wn * 64 + b * 32 + fr, N - 1)] : 0.f;
#pragma unroll
  for (int a = 0; a < AM; ++a) {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * fs;
        const float v = acc[a][b][r] + bv[b];
        // bf16 output (x was converted to fp16 by the caller): rounded to fp16 and then to bf16, as gemm3 and the reference's shim do
        if (p.out_bf16) ((uint16_t *)ep)[row * 72 + b * 32 + fr] = f32_to_bf16((float)(half_t)v);
        else ep[row * 72 + b * 32 + fr] = (half_t)v;
      }
    // 32 rows x 128 B = 256 chunks of 16 B: 4 per lane (wave-private region: no barrier, the wave's own LDS ops are ordered)
#pragma unroll
    for (int h = 0; h < 4; ++h) {
      const int c = lane + 64 * h, row = c >> 3, ch = c & 7;
      const uint4_t v = *(const uint4_t *)(ep + row * 72 + ch * 8);
      const int m = m0 + wm * WROWS + a * 32 + row;
      const int n = n0 + wn * 64 + ch * 8;
      if (m < p.M && n < N) *(uint4_t *)((half_t *)p.y + (size_t)m * N + n) = v;
    }
  }
}

template <int BITS>
int launch_b(const BitGemmParams &p, int grid, hipStream_t stream) {
  static DeviceLatch attr_done;  // per (kernel, device): the LDS opt-in is a per-device attribute
  if (int rc = lds_optin(attr_done, (const void *)bitgemm_kernel<BITS>)) return rc;
  const size_t lds = (size_t)(3 * kATile + 2 * kBTile) * sizeof(half_t);  // 128 KB
  hipLaunchKernelGGL((bitgemm_kernel<BITS>), dim3(grid), dim3((kMW + 4) * 64), lds, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace

// what the kernel takes apart from the row count, x and y: NULL, or why not
const char *bitgemm_refusal(const qllm_weight_t &w) {
  if (w.layout != QLLM_LAYOUT_GPTQ && w.layout != QLLM_LAYOUT_HQQ) return "the layout must be GPTQ or HQQ (row-stream words in place)";
  if (w.bits < 2 || w.bits > 8) return "bits must be 2..8";
  if (w.K % 64 != 0) return "K must be a multiple of 64";
  if (w.group_size % 32 != 0) return "group_size must be a multiple of 32";
  if (w.N % 8 != 0) return "N must be a multiple of 8";
  if ((uintptr_t)w.qweight % 4 || (uintptr_t)w.scales % 2 || (uintptr_t)w.qzeros % 4 || (uintptr_t)w.bias % 2) return "qweight / qzeros must be 4-byte, scales / bias 2-byte aligned";
  if ((double)w.K * w.N * w.bits / 8 >= 2147483648.0) return "the packed words must be below 2 GiB";
  return nullptr;
}

// ONE function for the launch and for qllm_bitgemm_describe / qllm_bitgemm_workspace_bytes.  `ws_bytes`: bytes of a usable workspace
// (0: none -> no split).  The factor is gemm2_split_k's rule: the largest S <= 8 (a power of two) with tiles * S <= CUs and at least
// 8 k-tiles per block; the blocks' k-tile counts may differ by one.
BitGemmGeom bitgemm_geometry(const qllm_weight_t &w, int M, size_t ws_bytes) {
  BitGemmGeom g;
  g.tiles = ((M + BM - 1) / BM) * ((w.N + BN - 1) / BN);
  const int kt = w.K / BK;
  int s = 1;
  while (s < 8 && (long long)g.tiles * (s * 2) <= compute_units() && kt / (s * 2) >= 8) s *= 2;
  g.split_k = s;
  g.slab_bytes = s > 1 ? (size_t)g.tiles * s * BM * BN * sizeof(float) : 0;
  if (s > 1 && (ws_bytes < 16384 + g.slab_bytes || g.tiles > 4096)) {  // (16384: the counter page every route shares, one counter per tile)
    g.split_k = 1;
    g.slab_bytes = 0;
  }
  g.grid = g.tiles * g.split_k;
  return g;
}

int launch_bitgemm(const BitGemmParams &p, const BitGemmGeom &g, hipStream_t stream) {
  switch (p.bits) {
    case 2: return launch_b<2>(p, g.grid, stream);
    case 3: return launch_b<3>(p, g.grid, stream);
    case 4: return launch_b<4>(p, g.grid, stream);
    case 5: return launch_b<5>(p, g.grid, stream);
    case 6: return launch_b<6>(p, g.grid, stream);
    case 7: return launch_b<7>(p, g.grid, stream);
    case 8: return launch_b<8>(p, g.grid, stream);
  }
  return set_error(QLLM_ERR_UNSUPPORTED, "bitgemm: bits must be 2..8 (got %d)", p.bits);
}

}  // namespace qllm
