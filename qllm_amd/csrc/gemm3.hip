// Prefill GEMM v3: y[M,N] = x[M,K] . dequant(W4), 256x128x64 block tile, WAVE-SPECIALISED: 4 matrix waves + 4 dequant waves.
//
// Why: gemm2's eight waves all run the same body -- dequantise, stage, read fragments, MFMA -- and the two waves that share
// a SIMD move through those phases in lockstep between barriers, so the VALU / LDS-store work of one never hides under the
// MFMAs of the other; the matrix pipe is ~40 % busy (profiles/r01_prefill_summary.md).  Here the roles are split per SIMD
// (waves w and w+4 share one):
//   * waves 0-3, "matrix": each owns a 128x64 output tile = 4x2 tiles of v_mfma_f32_32x32x16_f16 (128 accumulator
//     registers).  Instruction stream: ds_read_b128 + MFMA (6 fragment reads per 8 MFMAs; fragments double-buffered one k16
//     sub-step ahead; the k-tile barrier sits in front of the LAST sub-step's MFMAs so the next tile's first fragment reads
//     are covered too) plus the ACTIVATION tile, which needs no arithmetic: 8 LDS-DMA pieces per wave and k-tile
//     (buffer_load_dwordx4 ... lds: 1 KB = 8 rows x 128 B each, no registers, no ds_write), one behind every four MFMAs,
//     requested two k-tiles ahead into a 3-deep ring and retired with a counted vmcnt(8) in front of the barrier.  These waves issue no other vector
//     memory operation, so the hand-placed vmcnt counts exactly the DMA pieces.
//   * waves 4-7, "dequant": packed weight words + raw scale/zero words through buffer loads (per-lane offsets fixed, the
//     k-tile advance is a scalar offset: no address VALU), two register sets requested ~1.5 k-tiles ahead, the bit-exact
//     3-op fp16 dequant (common.hpp) and ds_write_b128 into the other B stage.  (First version: these waves also staged the
//     activations through registers -- 12 ds_write_b128 + ~130 VALU per k-tile in ONE wave per SIMD -- and were the
//     bottleneck: 748 TFLOP/s against gemm2's 846 on 2048x4096x4096.)
//   * LDS: A 3 x 32 KB + B 2 x 16 KB = 128 KB, one workgroup barrier per k-tile:
//         dequant, iteration t:  [write B tile t+1 -> stage (t+1)%2]                                      barrier #t
//         matrix,  iteration t:  sub-steps 0..2 of tile t, fragments of 3 in registers, vmcnt(8)          barrier #t
//                                [request A tile t+3 -> ring slot t%3] [read tile t+1's first fragments] [MFMAs of sub-step 3]
//     after barrier #t nobody reads B stage t%2 / A slot t%3 any more, and B stage (t+1)%2 / A slot (t+1)%3 are complete
//     (every matrix wave waited for its own DMA pieces of tile t+1 before arriving).  The matrix waves use the raw
//     s_barrier with explicit lgkmcnt(0) / vmcnt(8): __syncthreads() would drain the DMA ring (vmcnt(0)).
//   * LDS rows are 64 halves (128 B) with the eight 16-byte slots XORed by lds_row_swizzle(row) (common.hpp; the plain
//     (row >> 1) & 7 of the first version left the staging waves' ds_write_b128 2-way conflicted: 8 consecutive rows hit only 4
//     slots -- 2.2 M of 15.3 M LDS cycles per launch): conflict-free for the 32x32x16
//     fragment reads (lane l -> row l % 32, slot 2*ks + l / 32: each 16-lane service group of ds_read_b128 sees 8 even and
//     8 odd rows with 8 distinct row>>1 values mod 8) and for the GPTQ weight stores (8 consecutive rows at one slot).  An
//     LDS-DMA piece lands lane-linear (lane l -> row l / 8, physical slot l % 8), so the swizzle is applied to the SOURCE:
//     lane l fetches logical chunk (l % 8) ^ lds_row_swizzle(row) of its row (cdna_hip_programming.md rule 21).
//   * epilogue: + bias, one rounding, transposed through wave-private LDS into 16-byte row-contiguous stores.
// Serves what gemm2's 256x128 form serves when no split-K is wanted (M >= 1024 on the Llama shapes); gemm2 keeps the rest.
// Replaces gemm_forward_4bit_cuda_m16n128k32 (/root/reference/csrc/awq_cuda/quantization/gemm_cuda_gen.cu:31-353).
//
// Shared with bitgemm.hip (the same tile, MW = 8, for the widths and the N this unit does not take): tile256.hpp holds the tile
// constants, tile_off and xcd_run; tile256_body.inc holds the staging waves' schedule, the matrix waves, the split-K hand-off and the
// epilogue, and is included into gemm3_kernel below.  What is this unit's own: the block-to-tile map (tail split, grouped launches,
// raster) and the staging waves' load_b / store_b for the three 4- / 3-bit layouts.
#include <stdlib.h>

#include "kernels.hpp"
#include "tile256.hpp"

namespace qllm {

// LAYOUT 0 = GPTQ/HQQ row stream (4 bits), 1 = AWQ GEMM, 2 = GPTQ/HQQ row stream with 3-bit weights (bit stream: the 32 k of
// a half k-tile are 3 consecutive word rows of the column).  p.sm (LAYOUT 0 / 2): the same words stored strip-major (the native
// layout, include/qllm_mi355x.h): only the loop-constant per-lane offsets and the row strides change -- a thread's four words are
// 4 x 64 B apart inside its strip instead of 4 x 4N B apart.  fp16 activations.  Requires K % 64 == 0, N % 128 == 0, power-of-two group size >= 32, no g_idx.
// Round 7, half-wide last tile (single strip-major 4-bit layers with N % 128 == 64: Falcon-7B's 4544 / 4672): the layer has ceil(N / 128)
// column tiles and the last one holds 64 live columns.  Its staging waves for columns >= N (waves MW+1, MW+3: bcol 64..127) read column
// N - 1's words / scale / zero point again instead (never past the layer's buffers) and fill B columns nobody consumes; its matrix waves
// with wn = 1 run the k-loop as usual (their DMA pieces feed wn = 0's rows) and leave before the epilogue: no bias read, no store.
// MW: matrix waves, 4 (one per SIMD, 128x64 each) or 8 (two per SIMD, 64x64 each: 8 fragment reads per 8 MFMAs instead of 6,
// but the two waves cover each other's LDS / barrier waits); always 4 dequant waves behind them.
// BF (round 6, LAYOUT 0 only): NATIVE bf16 -- the activation tiles are the caller's bf16 rows as they are (LDS-DMA moves bytes), the
// staging waves dequantise to bf16 (q as fp32 via v_cvt_f32_ubyte, one v_pk_fma_f32 per pair: W = bf16(s q - s z), ONE rounding;
// v_cvt_pk_bf16_f32), the matrix waves run v_mfma_f32_32x32x16_bf16 and the epilogue rounds the fp32 sums to bf16 once.  No conversion
// pre-pass, no fp16 overflow for |x| > 65504 (the reference's shim casts x to fp16: quant_linear_awq.py:29-36).
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));

template <int LAYOUT, int MW, bool PRIO = true, bool BF = false>
__global__ __launch_bounds__((MW + 4) * 64) void gemm3_kernel(const GemmParams p) {
  static_assert(!BF || LAYOUT == 0, "native bf16: row-stream / strip-major 4-bit layers");
  using namespace tile256;
  constexpr int AM = 8 / MW * 2;       // 32-row MFMA tiles per matrix wave along M: 4 or 2
  constexpr int WROWS = AM * 32;       // rows per matrix wave: 128 or 64
  constexpr int NP = 32 / MW;          // activation DMA pieces (8 rows x 128 B) per matrix wave and k-tile: 8 or 4
  constexpr bool N_ENDS_IN_TILE = false;  // a column tile ends at 128 columns, or at 64 (the half-wide last tile): whole matrix waves
  extern __shared__ __attribute__((aligned(16))) half_t smem[];
  half_t *As = smem;               // [3][256][64]  (LDS-DMA ring)
  half_t *Bs = smem + 3 * kATile;  // [2][128 n][64 k]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  // Round 6, grouped launches (p.n_prob > 1: layers sharing x -- q/k/v, gate/up -- in ONE grid): the tiles of layer 0 come first, then
  // layer 1's ...; a block looks its layer up from its tile id and takes that layer's pointers and width (P* below).  The rounds of
  // tiles are counted over the whole group: gate/up of Llama-2-7B are 1376 tiles = 5.4 rounds instead of 2 x 2.7 -> 2 x 3.
  const int tiles_m = (p.M + BM - 1) / BM;
  const int tiles_all = p.n_prob > 1 ? p.total_tiles : tiles_m * ((p.N + BN - 1) / BN);  // (a half-wide last column tile counts as one)
  // split-K (p.split_k > 1: fewer tiles than CUs): S consecutive block ids share an output tile and own consecutive K ranges;
  // each publishes its fp32 partial tile to a slab, the last to arrive sums them in fixed order (the protocol of gemm2.hip)
  // Round 6, tail split (p.tail_split > 1, tiles > CUs): the tiles of the whole rounds run unsplit; the tiles of the ragged last round
  // are shared by tail_split blocks each -- two segments of block ids, each walked XCD-contiguously.
  int S, ksplit, tile_id, slab_tile;
  if (p.tail_split > 1) {
    const int F = p.tail_from, bid = blockIdx.x;
    if (bid < F) {
      S = 1;
      ksplit = 0;
      tile_id = slab_tile = xcd_run(bid, F);
    } else {
      const int u = xcd_run(bid - F, (tiles_all - F) * p.tail_split);
      S = p.tail_split;
      ksplit = u % S;
      slab_tile = u / S;
      tile_id = F + slab_tile;
    }
  } else {
    S = p.split_k;
    const int bid = xcd_run(blockIdx.x, tiles_all * S);
    ksplit = bid % S;
    tile_id = slab_tile = bid / S;
  }
  S = __builtin_amdgcn_readfirstlane(S);
  const uint32_t *Pqweight = p.qweight;
  const half_t *Pscales = p.scales, *Pbias = p.bias;
  const void *Pqzeros = p.qzeros;
  void *Py = p.y;
  int PN = p.N, Pzk = p.zero_kind, bid = tile_id;
  if (p.n_prob > 1) {
    int pi = 0;
#pragma unroll
    for (int i = 1; i < kGemm3MaxProb; ++i) pi += (i < p.n_prob && tile_id >= p.prob[i].tile_begin) ? 1 : 0;
    const GemmProb &q = p.prob[pi];
    Pqweight = q.qweight; Pscales = q.scales; Pbias = q.bias; Pqzeros = q.qzeros; Py = q.y;
    PN = q.N; Pzk = q.zero_kind; bid = tile_id - q.tile_begin;
  }
  const int tiles_n = (PN + BN - 1) / BN;
  // p.raster 1: n fastest (an XCD's run shares activation rows, which stay in its L2 while the small packed weights stream)
  const int tm = p.raster ? (bid / tiles_n) : (bid % tiles_m);
  const int tn = p.raster ? (bid % tiles_n) : (bid / tiles_m);
  const int m0 = tm * BM, n0 = tn * BN;
  // this block's k-tiles [KT0, KT0 + KT): the S blocks of a tile own k-tile counts that differ by one at most (the planner splits only
  // where every block keeps >= 8; layers of N % 128 == 0 only where K / 64 is a multiple of S, i.e. equal counts)
  const int KT0 = p.K / BK * ksplit / S;
  const int KT = p.K / BK * (ksplit + 1) / S - KT0;

  if (wave >= MW) {
    // ================================================= dequant waves ==================================================
    const int t = tid - MW * 64;  // 0..255
    // ---- B -------------------------------------------------------------------------------------------------------------
    // GPTQ: thread = column t % 128, word rows 4 (t / 128) .. +3 of the 8 in a k-tile -> 4 x b128 stores
    //       (3 bits: word rows 3 (t / 128) .. +2 of the 6 in a k-tile = the same 32 k -> the same 4 stores)
    // AWQ : thread = word column t % 16 (8 columns), k rows 4 (t / 16) .. +3 -> per column one 8-byte store of 4 k
    constexpr bool ROWS = LAYOUT != 1;   // row-stream layouts
    constexpr int WPT = (LAYOUT == 2) ? 3 : 4;  // packed words per thread and k-tile
    const int bcol = ROWS ? (t & 127) : 8 * (t & 15);
    const int brow = ROWS ? 4 * (t >> 7) : 4 * (t >> 4);
    const int nB = min(n0 + bcol, PN - 1);  // (half-wide last tile: columns >= N re-read column N - 1; their B columns are never consumed)
    const uint32_t nibmask = nib_mask_vgpr();
    uint32_t himask;
    asm volatile("v_mov_b32 %0, 0x00f000f0" : "=v"(himask));  // (held in a VGPR for the same reason as nibmask: one v_and_or_b32)
    const int zk = Pzk;
    const uint32_t *zbase = (zk == ZK_SYM) ? (const uint32_t *)Pscales : (const uint32_t *)Pqzeros;
    // zero points: words per group row (zmul), this column's word inside the row (zoff), and -- strip-major storage (p.sm, row-stream
    // layouts only) -- the word offset of the column's strip (zstrip; group rows then hold the strip's 16 columns only: 2 or 8 words)
    const int Gn = (p.K + (1 << p.gs_shift) - 1) >> p.gs_shift;
    const bool sm = ROWS && p.sm;
    const int ncs = sm ? (nB & 15) : nB;  // column index inside a row of the scale / zero tables
    const int zmul_all = (zk == ZK_PACKED) ? (LAYOUT == 2 ? (PN * 3) >> 5 : (PN >> 3)) : (PN >> 1);  // words per group over all columns
    const int zmul = sm ? ((zk == ZK_PACKED) ? 2 : 8) : zmul_all;
    const int zoff = ((zk == ZK_PACKED) ? (LAYOUT == 2 ? (ncs * 3) >> 5 : (ncs >> 3)) : (ncs >> 1)) + (sm ? (nB >> 4) * Gn * zmul : 0);
    const int zoff2 = (LAYOUT == 2 && zk == ZK_PACKED && (sm ? ((ncs * 3) >> 5) == 0 : zoff + 1 < zmul)) ? 1 : 0;  // packed 3-bit zero points may straddle two words
    struct BSet {
      uint32_t w[4];
      half8_t s8;     // AWQ: the 8 columns' scales
      uint32_t sraw;  // GPTQ: the column's scale, raw 16 bits
      uint32_t z, z2;
    };
    BSet bset[2];
    // buffer loads: per-lane byte offsets are loop constants, the k-tile / group advance is a scalar offset (SALU only)
    const auto rs_w = __builtin_amdgcn_make_buffer_rsrc((void *)Pqweight, 0, (int)((size_t)p.K * PN / 2), 0x00020000);
    const auto rs_s = __builtin_amdgcn_make_buffer_rsrc((void *)Pscales, 0, Gn * PN * 2, 0x00020000);
    // (strip-major: every strip has whole words of its own -- 3-bit zero points take 2 words per 16 columns, not 1.5)
    const auto rs_z = __builtin_amdgcn_make_buffer_rsrc((void *)zbase, 0, (sm ? (PN >> 4) * Gn * zmul : Gn * zmul_all) * 4, 0x00020000);
    const int wrow_bytes = sm ? 64 : (ROWS ? PN * 4 : (PN >> 3) * 4);     // bytes per packed row (strip-major: the strip's 16 words)
    const int ktile_bytes = (LAYOUT == 0 ? 8 : (LAYOUT == 2 ? 6 : BK)) * wrow_bytes;  // packed rows per k-tile: 8 / 6 (3 bits) / 64 (AWQ)
    const int strip_rows = (LAYOUT == 2) ? (p.K * 3) >> 5 : (p.K >> 3);      // word rows of one strip
    const int voff_w = (LAYOUT == 2 ? 3 * (t >> 7) : brow) * wrow_bytes +
                       (sm ? (nB >> 4) * strip_rows * 64 + ncs * 4 : (ROWS ? nB * 4 : (nB >> 3) * 4));
    const int srow_bytes = sm ? 32 : PN * 2;                                // bytes per group row of the scale table
    const int voff_s = sm ? (nB >> 4) * Gn * 32 + ncs * 2 : nB * 2, voff_z = zoff * 4;
    const int krow0 = ROWS ? 8 * brow : brow;                               // this thread's first k inside a k-tile
    auto load_b = [&](int kt, BSet &bs) {
      const int ktc = KT0 + min(kt, KT - 1);
      const int so = ktc * ktile_bytes;
#pragma unroll
      for (int r = 0; r < WPT; ++r) bs.w[r] = __builtin_amdgcn_raw_buffer_load_b32(rs_w, voff_w + r * wrow_bytes, so, 0);
      // one group per thread per k-tile (group_size >= 32); krow0 is per-lane only through brow (0 or 32 k for GPTQ)
      const int G0 = (ktc * BK) >> p.gs_shift, G1 = (ktc * BK + 32) >> p.gs_shift;
      const int G = ROWS ? ((krow0 >= 32) ? G1 : G0) : ((ktc * BK + krow0) >> p.gs_shift);
      if constexpr (ROWS)
        bs.sraw = __builtin_amdgcn_raw_buffer_load_b16(rs_s, voff_s + G * srow_bytes, 0, 0);
      else
        bs.s8 = __builtin_bit_cast(half8_t, __builtin_amdgcn_raw_buffer_load_b128(rs_s, voff_s + G * srow_bytes, 0, 0));
      bs.z = __builtin_amdgcn_raw_buffer_load_b32(rs_z, voff_z + G * zmul * 4, 0, 0);
      if constexpr (LAYOUT == 2) bs.z2 = __builtin_amdgcn_raw_buffer_load_b32(rs_z, voff_z + zoff2 * 4 + G * zmul * 4, 0, 0);
    };
    auto store_b = [&](int stage, const BSet &bs) {
      half_t *Bb = Bs + stage * kBTile;
      if constexpr (LAYOUT == 2) {
        // 32 k = 96 bits of the column's bit stream in w[0..2]: four 24-bit fields of 8 values each, natural k order
        const uint32_t zfield = (uint32_t)(((((uint64_t)bs.z2) << 32) | bs.z) >> ((3 * ncs) & 31));
        const half_t zp = (half_t)(float)((zfield + (uint32_t)p.add_zero_bias) & 7u);
        const half_t zf = __builtin_bit_cast(half_t, (uint16_t)((nB & 1) ? (bs.z >> 16) : (bs.z & 0xffffu)));
        const half_t sc = __builtin_bit_cast(half_t, (uint16_t)bs.sraw);
        const ColConst cc = make_col_const(sc, (zk == ZK_PACKED) ? zp : ((zk == ZK_F16) ? zf : (half_t)4.f));
        const uint32_t f[4] = {bs.w[0] & 0xffffffu, __builtin_amdgcn_alignbit(bs.w[1], bs.w[0], 24) & 0xffffffu,
                               __builtin_amdgcn_alignbit(bs.w[2], bs.w[1], 16) & 0xffffffu, bs.w[2] >> 8};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          half2_t b[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t lo = (f[r] >> (6 * j)) & 7u, hi = (f[r] >> (6 * j + 3)) & 7u;
            b[j] = deq_pair(lo | (hi << 16) | kMagic, cc);
          }
          *(half8_t *)(Bb + tile_off(bcol, brow + r)) = half8_t{b[0].x, b[0].y, b[1].x, b[1].y, b[2].x, b[2].y, b[3].x, b[3].y};
        }
      } else if constexpr (LAYOUT == 0) {
        const half_t zp = (half_t)(float)(((bs.z >> (4 * (nB & 7))) + (uint32_t)p.add_zero_bias) & 15u);
        const half_t zf = __builtin_bit_cast(half_t, (uint16_t)((nB & 1) ? (bs.z >> 16) : (bs.z & 0xffffu)));
        const half_t sc = __builtin_bit_cast(half_t, (uint16_t)bs.sraw);
        if constexpr (BF) {
          // bf16 W: even / odd nibbles as bytes (k = 2 i / 2 i + 1 in byte i), q -> fp32, (q_a, q_b) s - z s in one packed fma, one
          // rounding to bf16; pairs come out in natural k order.  (The empty asm keeps hipcc from splitting the two masks back into
          // one shift + and per nibble.)
          const float sf = (float)sc, zf32 = (zk == ZK_PACKED) ? (float)zp : ((zk == ZK_F16) ? (float)zf : 8.f);
          const float2_t s2 = {sf, sf}, nzs2 = {-(zf32 * sf), -(zf32 * sf)};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            uint32_t e = bs.w[r] & 0x0f0f0f0fu, o = (bs.w[r] >> 4) & 0x0f0f0f0fu;
            asm volatile("" : "+v"(e), "+v"(o));
            uint32_t out[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float2_t q = {(float)((e >> (8 * i)) & 0xffu), (float)((o >> (8 * i)) & 0xffu)};
              out[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(__builtin_elementwise_fma(q, s2, nzs2), bf16x2_t));
            }
            *(uint4_t *)(Bb + tile_off(bcol, brow + r)) = uint4_t{out[0], out[1], out[2], out[3]};
          }
        } else {
          const ColConst cc = make_col_const(sc, (zk == ZK_PACKED) ? zp : ((zk == ZK_F16) ? zf : (half_t)8.f));
          // Round 6: the odd nibbles are taken where they sit (bits 4..7 of each half) under the pattern 0x5400 = 64.0 -- an fp16 in
          // [64, 128) has ulp 1/16, so mantissa bits 4..7 weigh exactly 1, 2, 4, 8: r = 64 + q -- and fma(r, s, -64 s) is q s rounded
          // once, like fma(1024 + q, s, -1024 s) for the even ones: the same three-rounding W bit for bit, one shift per word instead
          // of three (13 VALU per 8 weights instead of 15: the staging waves' issue slots are what the matrix waves wait for).
          const half2_t c64 = splat2((half_t)(-64.0f) * sc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const uint32_t w0 = bs.w[r], w8 = bs.w[r] >> 8;
            const half2_t b0 = deq_pair(and_or(w0, nibmask, kMagic), cc);                                                   // (k0, k4)
            const half2_t b1 = __builtin_elementwise_fma(as_h2(and_or(w0, himask, 0x54005400u)), cc.s2, c64) - cc.zs2;     // (k1, k5)
            const half2_t b2 = deq_pair(and_or(w8, nibmask, kMagic), cc);                                                   // (k2, k6)
            const half2_t b3 = __builtin_elementwise_fma(as_h2(and_or(w8, himask, 0x54005400u)), cc.s2, c64) - cc.zs2;     // (k3, k7)
            *(half8_t *)(Bb + tile_off(bcol, brow + r)) = half8_t{b0.x, b1.x, b2.x, b3.x, b0.y, b1.y, b2.y, b3.y};
          }
        }
      } else {
        // rows brow..brow+3 of 8 interleaved columns: column c of the word sits at nibble awq_nibble_of_col(c).  Two
        // v_perm build, per column pair, the (k0,k1) and (k2,k3) nibble-bearing 16-bit halves side by side.
        const uint32_t P01 = __builtin_amdgcn_perm(bs.w[1], bs.w[0], 0x05040100u), Q01 = __builtin_amdgcn_perm(bs.w[1], bs.w[0], 0x07060302u);
        const uint32_t P23 = __builtin_amdgcn_perm(bs.w[3], bs.w[2], 0x05040100u), Q23 = __builtin_amdgcn_perm(bs.w[3], bs.w[2], 0x07060302u);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
          const int sh = 4 * (c >> 1);
          const half_t z = (half_t)(float)((bs.z >> (4 * awq_nibble_of_col(c))) & 15u);
          const ColConst cc = make_col_const(bs.s8[c], z);
          const half2_t b01 = deq_pair(and_or(((c & 1) ? Q01 : P01) >> sh, nibmask, kMagic), cc);
          const half2_t b23 = deq_pair(and_or(((c & 1) ? Q23 : P23) >> sh, nibmask, kMagic), cc);
          *(uint2_t *)(Bb + tile_off(bcol + c, brow >> 3) + (brow & 7)) = uint2_t{as_u32(b01), as_u32(b23)};
        }
      }
    };

#define TILE256_STAGING  // the schedule of load_b / store_b / barriers
#include "tile256_body.inc"
  }

#include "tile256_body.inc"  // matrix waves, split-K hand-off, epilogue
}

// round 7: single strip-major 4-bit layers whose last 128-column tile is half wide (N % 128 == 64: Falcon-7B); the 4-bit row-stream
// layouts in place keep the 128x128 kernel, 3-bit and AWQ layers their N % 128 == 0 rule
bool gemm3_n_tail(const GemmParams &p, int layout) { return p.N % 128 == 64 && p.sm && layout == QLLM_LAYOUT_GPTQ && p.n_prob <= 1; }

bool gemm3_ok(const GemmParams &p, int layout) {
  const int on = knob("QLLM_GEMM3", 1);
  // 4 bits: from M = 1024 (below it gemm2's split-K form was the measured choice; QLLM_GEMM3_MIN_M moves the line);
  // 3 bits: every prefill size -- the alternative there is the dequant kernel + a dense GEMM
  // round 3 (profiles/r03_mid_m.md, tools/lab/gbench): with split-K this kernel passes gemm2 from M = 384 on the 11008-wide shapes
  // (59 vs 64 us at M = 384 / 512, 110 vs 130 and 89 vs 93 at 768) and from 768 on 4096 x 4096 (41 vs 43; 34.5 vs 33 below)
  const int min_m_env = knob("QLLM_GEMM3_MIN_M", 0);
  const int min_m = min_m_env ? min_m_env : (((size_t)p.K * p.N > (size_t)4096 * 4096) ? 384 : 768);
  const int min_m3 = knob("QLLM_GEMM3_MIN_M_3BIT", 33);  // (33..64: native-layout layers whose strips stop at two row tiles)
  // round 7: a half-wide last column tile has no gemm2 form to fall back on -- gemm3 (split-K below min_m) from gemm2's 33 rows
  const bool tail = gemm3_n_tail(p, layout);
  if (!on || p.g_idx || p.K % 64 != 0 || (p.N % 128 != 0 && !tail)) return false;
  if (p.M < (layout == kGemm3Rows3Bit ? min_m3 : (tail ? 33 : min_m))) return false;
  // fp16 activations only: the activation tile goes to LDS by DMA, which cannot convert bf16 on the way (callers convert x with
  // launch_bf16_to_f16 first and set out_bf16, or use gemm2); 32-bit byte offsets into x and the packed weights
  if (p.act_bf16 || (size_t)p.M * p.K * 2 >= 0x7fffffffull || (size_t)p.K * p.N / 2 >= 0x7fffffffull) return false;
  return p.group_size % 32 == 0 && p.gs_shift >= 5;
}

// bf16 activations served natively (no conversion pre-pass): the 4-bit row-stream / strip-major layouts (the modules' native copies)
bool gemm3_bf16_native(int layout) { return knob("QLLM_GEMM3_BF16", 1) && layout == QLLM_LAYOUT_GPTQ; }

__global__ __launch_bounds__(256) void bf16_to_f16_kernel(const uint4_t *__restrict__ src, uint4_t *__restrict__ dst, size_t n8) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n8) dst[i] = __builtin_bit_cast(uint4_t, bf16x8_to_h8(src[i]));
}

int launch_bf16_to_f16(const void *src, void *dst, size_t n, hipStream_t stream) {
  const size_t n8 = n / 8;  // callers pass M * K with K % 64 == 0
  hipLaunchKernelGGL(bf16_to_f16_kernel, dim3((unsigned)((n8 + 255) / 256)), dim3(256), 0, stream, (const uint4_t *)src, (uint4_t *)dst, n8);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

template <int LAYOUT, int MW, bool PRIO = true, bool BF = false>
static int launch_gemm3_b(const GemmParams &p, hipStream_t stream) {
  using namespace tile256;
  static DeviceLatch attr_done;
  if (int rc = lds_optin(attr_done, (const void *)gemm3_kernel<LAYOUT, MW, PRIO, BF>)) return rc;
  const int tiles_all = p.n_prob > 1 ? p.total_tiles : ((p.M + BM - 1) / BM) * ((p.N + BN - 1) / BN);
  const int tiles = p.tail_split > 1 ? p.tail_from + (tiles_all - p.tail_from) * p.tail_split : tiles_all * p.split_k;
  hipLaunchKernelGGL((gemm3_kernel<LAYOUT, MW, PRIO, BF>), dim3(tiles), dim3((MW + 4) * 64), kLdsBytes, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// split-K factor for gemm3: gemm2's rule (largest S <= 8 with tiles * S <= CUs and >= 8 k-tiles per block), reduced until every
// block owns the same number of k-tiles.  Round 7, N % 128 == 64: the half-wide last tile counts as a tile, and the blocks' k-tile counts
// may differ by one (Falcon-7B's K = 4544 is 71 k-tiles: a whole-count rule would never split it)
int gemm3_split_k(int M, int N, int K) {
  const bool tail = N % 128 != 0;
  int s = gemm2_split_k(M, gemm3_tile_cols(N), K);
  while (s > 1 && (K / 64) % s != 0 && !tail) s /= 2;
  return s;
}

// Round 6: K-split of the ragged last round.  More tiles than CUs and a last round that fills at most half of them (profiles/
// r06_shape_table.md: Llama-2-13B's 5120-wide layers are 320 tiles = 1.25 rounds and ran at 767 TFLOP/s where the 256-tile layers
// of Llama-2-7B run at 970-1070): the r = tiles mod CUs tiles of that round are shared by TS blocks each -- the largest power of two with
// r * TS <= CUs, whole k-tile counts and >= 16 k-tiles per block (the fix-up moves 2 x 128 KB per block: below that it eats the gain).
// Returns TS (1: none) and the number of unsplit tiles in *tail_from.
// (round 7, N % 128 == 64: the half-wide last tile counts as a tile; k-tile counts may differ by one, as for gemm3_split_k)
int gemm3_tail_split(int M, int N, int K, int *tail_from) {
  return gemm3_tail_split_tiles(((M + 255) / 256) * (gemm3_tile_cols(N) / 128), K, tail_from, N % 128 != 0);
}
int gemm3_tail_split_tiles(int tiles, int K, int *tail_from, bool uneven) {
  const int cus = compute_units(), kt = K / 64;
  *tail_from = tiles;
  if (!knob("QLLM_GEMM3_TAIL", 1) || tiles <= cus || tiles % cus == 0) return 1;
  const int r = tiles % cus;
  int ts = 1;
  while (ts < 8 && r * ts * 2 <= cus && (uneven || kt % (ts * 2) == 0) && kt / (ts * 2) >= 16) ts *= 2;
  if (ts > 1) *tail_from = tiles - r;
  return ts;
}

int launch_gemm3(const GemmParams &p_in, int layout, hipStream_t stream) {
  GemmParams p = p_in;
  if (p.split_k < 1 || !p.slabs || !p.counters) p.split_k = 1;
  if (p.tail_split < 2 || !p.slabs || !p.counters || p.split_k != 1) p.tail_split = 0;
  const int raster = knob("QLLM_GEMM2_RASTER", 1);
  p.raster = raster;
#ifdef QLLM_LAB
  if (const int g4 = knob("QLLM_GEMM4", -1); g4 >= 0) return launch_gemm4(p, layout, g4, stream);  // (lab) tools/lab/gemm4.hip variants
  // (lab) tools/lab/gemm5.hip: every wave a matrix wave, B fragments dequantised in registers; QLLM_GEMM5 = waves along M
  if (const int g5 = knob("QLLM_GEMM5", 0); g5 > 0 && gemm5_ok(p, layout)) return launch_gemm5(p, g5, stream);
#endif
  const int mw = knob("QLLM_GEMM3_MW", 8);  // measured (profiles/r02_prefill_summary.md): 8 matrix waves 908 / 923 / 1004 TFLOP/s, 4: 873 / 915 / 1003
  const int prio = knob("QLLM_GEMM3_PRIO", 1);
  if (p.native_bf16) {
    if (layout != QLLM_LAYOUT_GPTQ) return set_error(QLLM_ERR_INVALID, "internal: native bf16 serves the row-stream / strip-major 4-bit layouts");
    return launch_gemm3_b<0, 8, true, true>(p, stream);
  }
  if (layout == kGemm3Rows3Bit) return launch_gemm3_b<2, 8>(p, stream);
  if (mw == 4 && !prio) return layout == QLLM_LAYOUT_AWQ_GEMM ? launch_gemm3_b<1, 4, false>(p, stream) : launch_gemm3_b<0, 4, false>(p, stream);
  if (mw == 8) return layout == QLLM_LAYOUT_AWQ_GEMM ? launch_gemm3_b<1, 8>(p, stream) : launch_gemm3_b<0, 8>(p, stream);
  return layout == QLLM_LAYOUT_AWQ_GEMM ? launch_gemm3_b<1, 4>(p, stream) : launch_gemm3_b<0, 4>(p, stream);
}

}  // namespace qllm
