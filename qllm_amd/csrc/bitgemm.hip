// bitgemm: fused dequant + prefill GEMM (M >= 129) on the reference's row-stream layouts READ IN PLACE (GPTQ / HQQ qweight i32
// [K / 32 * bits][N]) at every width from 2 to 8 bits: the widths gemm3.hip does not take (2, 5, 6, 7, 8) and the 3- / 4-bit layers
// gemm3_ok refuses (N % 128 != 0).  Above bitpanel's rows such a call used to write the whole fp16 W with qllm_dequant (2 K N bytes),
// read it back in a dense GEMM and pay two launches, on every forward call.  Reached through qllm_linear_forward_bitgemm only: the
// planner, its routes and qllm_plan_describe do not know it.
//
// The tile is gemm3.hip's, at MW = 8: block tile 256 x 128 x 64, twelve waves.  The two units share their text: tile256.hpp holds the
// tile constants, tile_off and xcd_run; tile256_body.inc holds the staging waves' schedule, the matrix waves, the split-K hand-off and
// the epilogue, and is included into bitgemm_kernel below with MW = 8, PRIO = true, BF = false and N_ENDS_IN_TILE = true.  This unit's
// own: the block-to-tile map and the dequant waves' load_b / store_b.
//   * waves 0-7, "matrix" (tile256_body.inc): 64 x 64 each = 2 x 2 tiles of v_mfma_f32_32x32x16_f16.  The x tile arrives by LDS-DMA
//     into a 3-deep ring, 4 pieces per wave and k-tile, one between the two halves of every sub-step's MFMAs; a counted vmcnt(4) sits
//     in front of the raw s_barrier.  Rows past M re-read row M - 1 and are never stored;
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
//   * epilogue (tile256_body.inc, N_ENDS_IN_TILE): + bias (clamped read), one rounding, transposed through wave-private LDS, 16-byte
//     row-contiguous stores; a chunk is stored only if its first column is < N (N % 8 == 0: a chunk is inside N or outside it) and
//     its row is < M;
//   * split-K (tile256_body.inc): fp32 partial tiles to slabs with write-through stores, one relaxed agent-scope ticket per tile in
//     the shared counter page, the last arriver sums in split order and re-arms the counter.  The blocks' k-tile counts may differ by
//     one (KT0 = K / 64 * ksplit / S).  Block ids run through xcd_run;
//   * numerics: gemm3's fp16 contract.  The B tile holds fp16(q s) - fp16(z s), bit for bit what qllm_dequant produces; fp32 sums; y
//     rounded once (bf16 output: fp32 -> fp16 -> bf16, as gemm3); deterministic with and without a split.
// K % 64 == 0, N % 8 == 0, group_size % 32 == 0, fp16 x (bf16 callers convert first and ask for a bf16 y).
#include "kernels.hpp"
#include "planner.hpp"
#include "tile256.hpp"

namespace qllm {

using namespace tile256;

namespace {

constexpr int kMW = 8;  // matrix waves; four dequant waves behind them

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
  constexpr bool PRIO = true, BF = false;
  constexpr bool N_ENDS_IN_TILE = true;  // N % 8 == 0 is all this unit asks: the last column tile ends at any multiple of 8
  extern __shared__ __attribute__((aligned(16))) half_t smem[];
  half_t *As = smem;               // [3][256][64]  (LDS-DMA ring)
  half_t *Bs = smem + 3 * kATile;  // [2][128 n][64 k]

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  const int N = p.N;
  const int tiles_n = (N + BN - 1) / BN;
  const int tiles_all = ((p.M + BM - 1) / BM) * tiles_n;  // (a ragged last column tile counts as one)
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

#define TILE256_STAGING  // the schedule of load_b / store_b / barriers
#include "tile256_body.inc"
  }

  // (one layer per launch, no tail split: the layer's width, bias and y are p's, and a tile's slab and counter index is its id)
  const int slab_tile = tile_id, PN = N;
  const half_t *Pbias = p.bias;
  void *Py = p.y;
#include "tile256_body.inc"  // matrix waves, split-K hand-off, epilogue
}

template <int BITS>
int launch_b(const BitGemmParams &p, int grid, hipStream_t stream) {
  static DeviceLatch attr_done;  // per (kernel, device): the LDS opt-in is a per-device attribute
  if (int rc = lds_optin(attr_done, (const void *)bitgemm_kernel<BITS>)) return rc;
  hipLaunchKernelGGL((bitgemm_kernel<BITS>), dim3(grid), dim3((kMW + 4) * 64), kLdsBytes, stream, p);
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
  if (s > 1 && (ws_bytes < kCounterBytes + g.slab_bytes || g.tiles > (int)(kCounterBytes / sizeof(int)))) {  // (the counter page every route shares: one counter per tile)
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
