// attn_chunk.hip's call -- a FEW query rows per sequence (S >= 2, G * S <= 128) behind a long cache, all rows of a kv head in one block,
// the key positions split over the device -- against a QUANTIZED cache: 8- or 4-bit codes with one scale (and at 4 bits one zero) per group
// of 32 elements (kv_quant.hpp has the format).  The cache is read in place and never written; no dequantised row ever reaches memory.
// The caller has already put the S new rows in (kv_quantize), and kv_len counts them.
//
// The kernel is attn_chunk_body.inc, the text attn_chunk_kernel is made of: the rows a block holds, the 64-key tile, S^T = K Q^T and
// O^T = V^T P^T on mfma_f32_32x32x16 with V read transposed out of LDS, the fp32 online softmax, P rounded once, the hand-off, the ticket
// and the combine in split order by the last block to arrive, attn_chunk_geom's grid and workspace, a launch that never depends on the
// length.  What differs is how a tile reaches LDS (the two functions of attn_quant_tile.hpp, which attn_prefill_quant.hip stages its
// tiles with too; the body calls them where attn_chunk_kernel moves 16-byte chunks of act rows):
//
// Ownership.  The format's lane convention: a thread owns runs of 8 consecutive elements of a row, run c = tid + 256 u of the tile is
// chunk c % (D / 8) of row c / (D / 8) -- the act kernel's chunks, so the LDS image has the same addresses -- and the 4 neighbouring
// threads of a DPP quad own one group of 32.  64 * D / 8 / 256 runs of K and as many of V per thread and tile: 4 at D = 128, 2 at D = 64.
// Loads.  Per run the codes of K and of V: one 8-byte load each at 8 bits, one 4-byte load each at 4 bits, contiguous across the threads
// of a row.  The params: ONE 2-byte load per run fetches one of the group's K / V params, by the lane's place in the quad -- at 8 bits
// lanes 0 / 2 the K scale and lanes 1 / 3 the V scale, at 4 bits K scale, K zero, V scale, V zero -- and the other lanes read it with a
// quad_perm DPP (kvq_quad_lane) when the run is stored.  Against every thread loading its own 2 bytes of each param this is 1 load
// instead of 2 (8 bits) or 4 (4 bits) per run pair, with their 64-bit address arithmetic, for 2 or 4 DPP moves, and one register in
// flight instead of 2 or 4: fewer instructions and fewer registers, so this form is the one built (profiles/attn_chunk_quant.md has the
// counts of both).
// In flight for tile t + 1 are CODES AND PARAMS, not act values: 5 dwords per run pair at 8 bits and 3 at 4 bits, where the act kernel
// holds 8.
// Store.  A run is dequantised when it goes to LDS, by kv_dequantize_kernel's arithmetic to the letter (kvq_decode: the codes as fp32,
// s * code at 8 bits, fma(code, s, z) at 4, in fp32, one rounding to act) and written as the same 16-byte store at row * LROW + 8 * chunk.
// A position at or beyond the length is never loaded: its codes and params stay zero, which decode to zeros (s * 0 and fma(0, 0, 0)).
// So the MFMAs consume, bit for bit, what kv_dequantize would have written and attn_chunk_kernel would have staged.
//
// More than 128 rows per kv head (prompts, long chunks) over codes: attn_prefill_quant.hip.
// Not built: the append inside this kernel, quantized ring / sliding layers, fp8, int8 MFMA on the codes.
#include "attn_quant_tile.hpp"

namespace qllm {

namespace {

// attn_chunk_kernel's blocks per compute unit: two, but one at head_dim 128 with an additive mask
template <bool BF16, int D, int BITS, int MK>  // MK: the mask kind
__global__ __launch_bounds__(256, (D == 128 && MK == 2) ? 1 : 2) void attn_chunk_quant_kernel(const AttnChunkQuantParams p) {
  constexpr int QBITS = BITS;
#include "attn_chunk_body.inc"
}

template <bool BF16, int D, int BITS>
int launch_acq(const AttnChunkQuantParams &p, hipStream_t stream) {
  const dim3 grid((unsigned)p.splits, (unsigned)p.kv_heads, (unsigned)p.batch);
  switch (p.mask_kind) {
    case 0: hipLaunchKernelGGL((attn_chunk_quant_kernel<BF16, D, BITS, 0>), grid, dim3(256), 0, stream, p); break;
    case 1: hipLaunchKernelGGL((attn_chunk_quant_kernel<BF16, D, BITS, 1>), grid, dim3(256), 0, stream, p); break;
    default: hipLaunchKernelGGL((attn_chunk_quant_kernel<BF16, D, BITS, 2>), grid, dim3(256), 0, stream, p); break;
  }
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

template <bool BF16, int D>
int launch_acq_bits(const AttnChunkQuantParams &p, int bits, hipStream_t stream) {
  return bits == 8 ? launch_acq<BF16, D, 8>(p, stream) : launch_acq<BF16, D, 4>(p, stream);
}

}  // namespace

// shapes, bits, strides and alignment checked by the entry (capi.hip); p.splits / p.chunk from attn_chunk_geom
int launch_attn_chunk_quant(const AttnChunkQuantParams &p, int head_dim, int bits, int act_bf16, hipStream_t stream) {
  if (head_dim == 128) return act_bf16 ? launch_acq_bits<true, 128>(p, bits, stream) : launch_acq_bits<false, 128>(p, bits, stream);
  return act_bf16 ? launch_acq_bits<true, 64>(p, bits, stream) : launch_acq_bits<false, 64>(p, bits, stream);
}

}  // namespace qllm
