// Batch-1 decode kernel of the native strip-major layout (round 5): y[1, N] = x . dequant(W) for 4-bit layers with 128-wide groups.
// The same decomposition as strip_kernel.hpp's lds-slab form -- one block = one 16-column strip for ALL of K, its NW waves split K,
// every wave issues all of its loads before its first wait, no cross-block reduction -- rebuilt around what a launch costs BESIDES
// its bytes (profiles/r05_decode_bisect.md: the production kernel ran 1.2-1.5 us per launch above a read + reduce + store skeleton of
// the same launch shape):
//
//   * ONE batch of scalar loads.  The problem (layer) of a grouped launch is blockIdx.y, so the problem record's address depends on
//     nothing that has to be loaded first: header and record leave together (strip_kernel: n_prob -> block_begin8[1..] -> prob[pi]
//     -> late header words: 2 dependent round trips on single launches, 3 on gate/up, 4 on q/k/v).  Groups whose layers differ in
//     width launch max(n_strips) columns of blocks; the surplus blocks leave at once.
//   * ONE scale and ONE zero-point load per lane.  Lane (g, i) fetches group G0 + g of column i (strip_kernel: every lane all four
//     groups of its column) and finishes exactly that group:
//   * one accumulator for all groups.  The A operand's 16 rows are free at batch 1 (one real row): rows 4j..4j+3 carry x on the
//     k-steps of the wave's group j and zeros elsewhere (the lane's ds_read address is chosen per group, once: no instruction in the
//     loop), so after the wave's 16 (24) MFMAs lane (g, i) holds  sum_{k in group g} x_k (1024 + q_k)  of column i in its own
//     accumulator rows -- no accumulator reset per group, no select, and the per-group correction
//         y_g = s_g (acc_g - (z_g Sx_g + 1024 Sx'_g))
//     is ONE fma per lane after the last MFMA: s_g and c_g = s_g (z_g Sx_g + 1024 Sx'_g) are computed while the weights are still
//     in flight (Sx_g / Sx'_g are already in the lane: the 16-lane DPP row reduce of the staging pass leaves group g's sums in
//     every lane of row g, so they never go through LDS).  strip_kernel did the four groups one after the other on 16 lanes
//     behind the last MFMA (~100 instructions and a scalar load in the tail).
//   * chains: the MFMAs alternate between NCH accumulators (k-step s -> chain s % NCH) so that the last k-steps to arrive do not
//     queue behind one dependent chain.
//   * the cross-wave and cross-group sum is one pass: every lane stores its value to red[column][wave][g] and the first 16 lanes
//     of wave 0 read their column's NW x 4 values as float4s.
//
// Arithmetic contract: strip_kernel.hpp's (x . s(q - z) for the unrounded W, fp32): raw 0x6400 | nibble patterns as B fragments, the
// x16 of the odd nibbles undone by staging x / 16 in those A slots, one fp32 correction per group.
//
// LVL (lab builds only; the library instantiates LVL = 4): the bisect of tools/lab/dbisect.hip -- 0: loads + xor + reduce + store
// (the memlab2 skeleton behind this kernel's prologue), 1: + scale / zero loads, 2: + x staged through LDS (permute, Sx / Sx' DPP
// sums) and the A fragments read back, 3: + pattern build and MFMAs, 4: + corrections = the kernel.
//
// Replaces gemv<half> (/root/reference/csrc/ort_cuda/dq_gemv.cu:41-150).
#pragma once
#include "strip1_forms.hpp"

namespace qllm {

template <int CTRL>
__device__ __forceinline__ float dpp_add1(float v) {
  return v + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// bytes of LDS per block: red[16 columns][36 floats >= NW * 4] | per wave: staged x (XL KB) + 256 zero bytes
// floats per column of the reduction buffer: NW x 4 values, rows 16-byte aligned and never a multiple of 32 floats apart (7 and 15
// waves would otherwise put all 16 columns on the same banks)
constexpr int strip1_rs(int nw) { return nw * 4 + 4 + (((nw * 4 + 4) % 32 == 0) ? 4 : 0); }

template <int NW, int MAXS, int MR = 1>
constexpr int strip1_lds_bytes() {
  constexpr int XL = (MAXS * 4 + 63) / 64;
  static_assert(NW * 4 <= 64, "at most 16 waves");
  return 16 * MR * strip1_rs(NW) * 4 + NW * (MR * XL * 1024 + 256);
}

// SWIGLU (the fused down-projection entry, strip1_swiglu.hip): one 32-bit pair of the gate and of the up vector -> act(gate) * up as the
// eager act_fn(g) * u rounds it: silu in fp32, rounded to the activation type, the product in fp32, rounded again.
__device__ __forceinline__ float silu_f32(float g) { return g / (1.f + expf(-g)); }
template <bool BF16>
__device__ __forceinline__ uint32_t swiglu_pair(uint32_t g2, uint32_t u2) {
  if constexpr (BF16) {
    const float g0 = __builtin_bit_cast(float, g2 << 16), g1 = __builtin_bit_cast(float, g2 & 0xffff0000u);
    const float u0 = __builtin_bit_cast(float, u2 << 16), u1 = __builtin_bit_cast(float, u2 & 0xffff0000u);
    const float s0 = __builtin_bit_cast(float, (uint32_t)f32_to_bf16(silu_f32(g0)) << 16);
    const float s1 = __builtin_bit_cast(float, (uint32_t)f32_to_bf16(silu_f32(g1)) << 16);
    return (uint32_t)f32_to_bf16(s0 * u0) | ((uint32_t)f32_to_bf16(s1 * u1) << 16);
  } else {
    const half2_t g = as_h2(g2), u = as_h2(u2);
    const half_t s0 = (half_t)silu_f32((float)g.x), s1 = (half_t)silu_f32((float)g.y);
    return as_u32(half2_t{(half_t)((float)s0 * (float)u.x), (half_t)((float)s1 * (float)u.y)});
  }
}
template <bool BF16>
__device__ __forceinline__ uint4_t swiglu_chunk(uint4_t g, uint4_t u) {
  return uint4_t{swiglu_pair<BF16>(g.x, u.x), swiglu_pair<BF16>(g.y, u.y), swiglu_pair<BF16>(g.z, u.z), swiglu_pair<BF16>(g.w, u.w)};
}

// NORM (the fused RMSNorm entry, strip1_norm.hip): the sum of the fp32 squares of one chunk's eight elements, in element order (an fp16 /
// bf16 square is exact in fp32), and one 32-bit pair of the row and of the norm's weight -> weight * round(x * rstd) as the eager
// LlamaRMSNorm rounds it: x * rstd in fp32, rounded to the activation type, the product with the weight in fp32, rounded again.
template <bool BF16>
__device__ __forceinline__ float sumsq_chunk(uint4_t x) {
  const uint32_t wds[4] = {x.x, x.y, x.z, x.w};
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float lo, hi;
    if constexpr (BF16) {
      lo = __builtin_bit_cast(float, wds[j] << 16);
      hi = __builtin_bit_cast(float, wds[j] & 0xffff0000u);
    } else {
      const half2_t h = as_h2(wds[j]);
      lo = (float)h.x;
      hi = (float)h.y;
    }
    s += lo * lo;
    s += hi * hi;
  }
  return s;
}
template <bool BF16>
__device__ __forceinline__ uint32_t norm_pair(uint32_t x2, uint32_t w2, float rstd) {
  if constexpr (BF16) {
    const float x0 = __builtin_bit_cast(float, x2 << 16), x1 = __builtin_bit_cast(float, x2 & 0xffff0000u);
    const float w0 = __builtin_bit_cast(float, w2 << 16), w1 = __builtin_bit_cast(float, w2 & 0xffff0000u);
    const float h0 = __builtin_bit_cast(float, (uint32_t)f32_to_bf16(x0 * rstd) << 16);
    const float h1 = __builtin_bit_cast(float, (uint32_t)f32_to_bf16(x1 * rstd) << 16);
    return (uint32_t)f32_to_bf16(w0 * h0) | ((uint32_t)f32_to_bf16(w1 * h1) << 16);
  } else {
    const half2_t x = as_h2(x2), w = as_h2(w2);
    const half_t h0 = (half_t)((float)x.x * rstd), h1 = (half_t)((float)x.y * rstd);
    return as_u32(half2_t{(half_t)((float)w.x * (float)h0), (half_t)((float)w.y * (float)h1)});
  }
}
template <bool BF16>
__device__ __forceinline__ uint4_t norm_chunk(uint4_t x, uint4_t w, float rstd) {
  return uint4_t{norm_pair<BF16>(x.x, w.x, rstd), norm_pair<BF16>(x.y, w.y, rstd), norm_pair<BF16>(x.z, w.z, rstd), norm_pair<BF16>(x.w, w.w, rstd)};
}
// rstd of a row from the sum of its squares (both RMSNorm kernels): the eager rsqrt(mean + eps), in fp32
__device__ __forceinline__ float rms_rstd(float sumsq, int K, float eps) { return rsqrtf(sumsq / (float)K + eps); }
// bytes of LDS the NORM forms add behind strip1_lds_bytes: one partial sum of squares per wave (NW <= 16 floats)
constexpr int kStrip1NormLdsBytes = 64;

// NW waves x MAXS k-steps cover T (host: NW * MAXS >= T >= MAXS; EXACT: NW * MAXS == T, no masking of a shifted window)
// AR: the row-parallel form (one layer per launch, p.ar_* set): instead of storing y the block pushes its 16 partial outputs, rounded to
//     the activation type like the unfused path's y, into slot [parity][rank] of EVERY peer's staging buffer (comm.hip's layout and
//     protocol) and takes a ticket; the rank's last block publishes the world's flags, waits for the peers' and writes the sum of the
//     slots in rank order -- the o_proj / down_proj launch and its all-reduce are ONE launch (160 kernel boundaries per Llama-2-70B token).
// G64 (round 6): 64-wide groups (HQQ's default; the batch-1 kernel took 128-wide groups only and a g64 layer fell back to the general strip
//     kernel: 35.5 us per Llama-2-7B decoder layer against 26.3).  A group is then TWO k-steps, a pass of 16 k-steps holds EIGHT groups:
//     A rows 2 j, 2 j + 1 carry x on the k-steps of group j, so lane (g, i) finds group 2 g of the pass in accumulator registers 0 / 1
//     and group 2 g + 1 in registers 2 / 3 -- two scales, two zero points, two corrections per lane and pass; the staging pass sums x
//     over the 8 lanes of a group and fetches the neighbouring group's sums with one more DPP move.
// MR = 4 (round 6): batches 2..4 at the price of batch 1.  With 128-wide groups the A operand's rows 4 j .. 4 j + 3 all belong to group j of
//     the pass -- at batch 1 they carry four copies of x.  Here row 4 j + m carries batch row m (rows past M: zeros), so accumulator
//     register m of lane (g, i) is batch row m of column i for group g: the same weight stream, the same MFMAs, four times the staging
//     and four corrections per lane.  (Until then batches 2..4 took strip_dma.hpp: ~1.5 x a batch-1 launch.)
// B3 (round 6): 3-bit layers (configs[3] mixes 3- and 4-bit HQQ layers; at batch 1 the 3-bit ones ran on the general strip kernel: 43 us per
//     Llama-2-7B decoder layer against 28.6 for the 4-bit ones).  The recipe of strip_kernel.hpp inside this kernel's skeleton: a k-step is
//     three word rows of the strip; lane (g, i) needs bits [24 g, 24 g + 24) of column i's 96: two word loads (rows {0,0,1,2}[g] and
//     {0,1,2,2}[g]) + one v_alignbit; fragment slots (k0,k5 | k1,k6 | k2,k7 | k3,k4) taken where the fields sit, their weights
//     (2,1 | 16,8 | 128,64 | 1,1) divided out of the staged activations (exact: powers of two).
// SWIGLU: the activation is act(gate) * up of TWO vectors (p.x = gate, p.x2 = up: same shape and row stride).  Every chunk of x is
//     joined by the matching chunk of x2 in the same batch of loads (same window, same clamp, same row rule) and the staging pass forms
//     silu(g) * u with the two roundings of the eager expression (swiglu_pair) before anything else looks at the chunk: from there on the
//     kernel is the plain form's code, so a SWIGLU launch returns bit for bit what the plain launch returns on x = act(g) * u.  The SWIGLU
//     forms are kernels of their own (strip1_swiglu_kernel below, instantiated in strip1_swiglu.hip) around the same body: the body is
//     strip1_body.inc, included by both kernels with SWIGLU a constant of the enclosing function, so that strip1_kernel's template
//     parameters -- and with them the names and the code of every instantiation strip1.hip builds -- stay what they were.
// NORM: the activation is RMSNorm(x) of the un-normed row p.x with the norm's weight p.norm_w ([K], the activation type) and p.norm_eps;
//     batch 1 only (M = 2..4 -- the four-row forms -- is not built: it would double the instantiations, and the modules send one row).  The
//     weight's chunks are loaded with the x chunks (same window, same clamp).  Once its x chunks have arrived a wave sums the fp32 squares of
//     the elements it KEEPS (xkeep: the windows of non-EXACT forms overlap, and a shifted last window re-reads k-steps of its neighbour --
//     every k-step is owned by exactly one wave, so every element is counted once), reduces over its lanes (DPP over the 16-lane rows,
//     then the four rows in order) and writes ONE partial to LDS of its own behind the staging areas (kStrip1NormLdsBytes; the reduction
//     buffer at the start of `lds` is written by fast waves at the end of the kernel, possibly before a slow wave has read the partials).
//     One __syncthreads() -- behind the surplus-block test, which a whole block passes or leaves together -- then every wave sums the NW
//     partials in index order: the order depends on (NW, MAXS, T) only, so every block of the launch, whichever sibling it serves, forms
//     the same rstd bit for bit; block 0 of problem 0 reports it (p.rstd_out).  Each chunk is then rewritten in registers as
//     weight * round(x * rstd) (norm_pair: the two roundings of the eager expression, in the activation type, before the bf16 -> fp16
//     conversion), and from there on the kernel is the plain form's code: a NORM launch returns bit for bit what the plain grouped launch
//     returns on xn = weight * (x.float() * rstd).to(dtype).  Kernels of their own (strip1_norm_kernel below, strip1_norm.hip), as for SWIGLU.
// RESID: y = residual + linear(..) in the launch (p.residual: one row [N] in the activation type): the 16 threads that store the block's
//     outputs round their value to the activation type as the plain form does, add their element of the residual in fp32 and round
//     again -- the eager `residual + linear(x)`, rounding for rounding, so a RESID launch returns bit for bit what the plain (SWIGLU)
//     launch followed by torch's add returns.  The element is loaded with the prologue's loads and waits in one register -- except in
//     the ten SWIGLU forms at their register bound (RESID_LATE, strip1_body.inc: plain rounds of 24, rounds of 56 and 64), which load it
//     behind their last MFMA.  Batch 1 only,
//     no AR; kernels of their own around the same body (strip1_resid_kernel, strip1_swiglu_resid_kernel below; strip1_resid.hip,
//     strip1_swiglu_resid.hip), as for SWIGLU.  y may be the residual row itself: element n is read and written by the same thread.
template <int NW, int MAXS, bool EXACT, int NCH = 2, int LVL = 4, bool DBG = false, bool AR = false, bool G64 = false, int MR = 1, bool B3 = false>
// (second launch bound = minimum waves per SIMD: 64 registers up to rounds of 24 k-steps -- a CU full of waves -- 128 above)
__global__ __launch_bounds__(NW * 64, strip1_min_waves(MAXS, G64, MR, B3)) void strip1_kernel(const Strip1Params p) {
  constexpr bool SWIGLU = false, NORM = false, NORM_PARK = false;
  constexpr bool RESID = false;
#include "strip1_body.inc"
}

// the SWIGLU forms (strip1_swiglu.hip; WAVES: the second launch bound -- strip1_min_waves, the plain twin's)
template <int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3, int WAVES>
__global__ __launch_bounds__(NW * 64, WAVES) void strip1_swiglu_kernel(const Strip1Params p) {
  constexpr bool SWIGLU = true, NORM = false, NORM_PARK = false, DBG = false, AR = false;
  constexpr bool RESID = false;
  constexpr int NCH = 2, LVL = 4;
#include "strip1_body.inc"
}

// the NORM forms (grouped launch: blockIdx.y is the sibling; WAVES as above -- strip1_norm.hip)
template <int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3, int WAVES>
__global__ __launch_bounds__(NW * 64, WAVES) void strip1_norm_kernel(const Strip1Params p) {
  constexpr bool SWIGLU = false, NORM = true, DBG = false, AR = false;
  constexpr bool RESID = false;
  constexpr bool NORM_PARK = MAXS >= 64 || (MAXS == 24 && !G64 && !B3);   // (the forms whose twins sit next to their register bound)
  constexpr int NCH = 2, LVL = 4;
#include "strip1_body.inc"
}

// the RESID forms: the plain input (strip1_resid.hip) and act(gate) * up (strip1_swiglu_resid.hip); WAVES as above, the twin form's
template <int NW, int MAXS, bool EXACT, bool G64, bool B3, int WAVES>
__global__ __launch_bounds__(NW * 64, WAVES) void strip1_resid_kernel(const Strip1Params p) {
  constexpr bool SWIGLU = false, NORM = false, NORM_PARK = false, DBG = false, AR = false;
  constexpr bool RESID = true;
  constexpr int NCH = 2, LVL = 4, MR = 1;
#include "strip1_body.inc"
}

template <int NW, int MAXS, bool EXACT, bool G64, bool B3, int WAVES>
__global__ __launch_bounds__(NW * 64, WAVES) void strip1_swiglu_resid_kernel(const Strip1Params p) {
  constexpr bool SWIGLU = true, NORM = false, NORM_PARK = false, DBG = false, AR = false;
  constexpr bool RESID = true;
  constexpr int NCH = 2, LVL = 4, MR = 1;
#include "strip1_body.inc"
}

}  // namespace qllm
