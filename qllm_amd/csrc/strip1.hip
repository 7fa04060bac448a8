// Host side of the batch-1 native-layout decode kernel (strip1_kernel.hpp): the shape table, and the plain, the fused all-reduce and the
// diagnostics families of strip1_forms.hpp's form table -- which says what a family is and picks and launches the instantiation.
#include "strip1_forms.hpp"
#include "strip1_kernel.hpp"

namespace qllm {

// (waves per block, k-steps per wave) for T = K / 32 k-steps, or false: not served (the general strip kernel takes the call).
// One round per wave: NW * MAXS >= T >= MAXS.  Measured choices: profiles/r05_decode_bisect.md.
// `blocks`: 16-column strips of the launch (all layers); `cus`: compute units.
// Round 7, `odd64` (4-bit layers with 64-wide groups only): K % 128 == 64 too, i.e. T % 4 == 2 (Falcon-7B: K = 4544, T = 142).  No such T
// is a whole number of rounds (MAXS % 4 == 0), so these shapes always take the non-EXACT forms, whose last live wave shifts its window
// back to [T - MAXS, T): no load for a k-step >= T, and T - MAXS is even, so the window still starts on a 64-wide group (G0 = tb / 2).
bool strip1_shape(int K, int blocks, int cus, int *nw, int *maxs, bool odd64) {
  if (K % 128 != 0 && !(odd64 && K % 128 == 64)) return false;  // (whole 16-byte windows of x per four k-steps; 64-wide groups: the same table)
  const int T = K / 32;
  if (T < 8) return false;
  int w, m;
  if (T <= 32) { w = 4; m = 8; }
  else if (T <= 64) { w = 4; m = 16; }
  // one block per CU at most (o_proj): four waves x 32 k-steps, one per SIMD -- 3.54 vs 3.78 us (profiles/r05_decode_bisect.md); wider
  // launches lose with it (gate/up 9.89 vs 9.57)
  else if (T <= 128 && blocks <= cus && knob("QLLM_S1_NW4", 1)) { w = 4; m = 32; }
  else if (T <= 128) { w = 8; m = 16; }
  else if (T <= 192) { w = 8; m = 24; }
  else if (T <= 256) { if (knob("QLLM_S1_T256_NW16", 0)) { w = 16; m = 16; } else { w = 8; m = 32; } }
  else if (T <= 384) { w = 16; m = 24; }
  else if (T <= 512) { w = 16; m = 32; }
  // round 6 (profiles/r06_shape_table.md: Qwen2-7B's down_proj, K = 18944, sat on the general strip kernel at 0.33 of 8 TB/s): rounds of
  // 40 .. 64 k-steps, three / four accumulator sets -- K up to 32768 (Llama-2-70B's unsharded down_proj is K = 28672)
  else if (T <= 640) { w = 16; m = 40; }
  else if (T <= 768) { w = 16; m = 48; }
  else if (T <= 896) { w = 16; m = 56; }
  else if (T <= 1024) { w = 16; m = 64; }
  else return false;
  // No dead waves where an odd wave count is built: K = 11008 is 344 k-steps = 14 1/3 rounds of 24 -- the sixteenth wave of a 16 x 24
  // block owns nothing (it re-reads its neighbour's words and multiplies zeros); K = 3584 (a Llama-2-70B TP = 8 down_proj shard) is
  // exactly 7 x 16.  The cross-wave sum is a pairwise tree over NW values: the dead wave contributed an exact zero, same bits.
  const int need = (T + m - 1) / m;
  if (need < w && knob("QLLM_S1_ODD", 1) && ((need == 7 && m == 16) || (need == 15 && m == 24))) w = need;
  *nw = w;
  *maxs = m;
  return true;
}

// <NCH = 2, LVL = 4, DBG, AR>: the plain forms; the diagnostics forms (timeline stamps); the row-parallel layer fused with its one-shot
// all-reduce -- the forms of the Llama-class row-parallel shards (K / world per rank up to 16384: Llama-2-70B's down_proj at TP = 2)
template <bool DBG, bool AR>
struct Strip1Family {
  static constexpr const char *kWhat = AR ? "fused all-reduce" : "internal";
  static constexpr int kLdsExtra = 0, kMaxRound = AR ? 32 : 64;
  static constexpr bool kRows4 = !AR, kG64B3 = !AR;
  template <int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3>
  static Strip1Kernel kernel() { return strip1_kernel<NW, MAXS, EXACT, 2, 4, DBG, AR, G64, MR, B3>; }
};

int launch_strip1_allreduce(const Strip1Params &p, int nw, int maxs, int n_strips, hipStream_t stream) {
  return strip1_launch<Strip1Family<false, true>>(p, nw, maxs, dim3(n_strips, 1), stream);
}

int launch_strip1(const Strip1Params &p, int nw, int maxs, int n_prob, int max_strips, hipStream_t stream) {
  const dim3 grid(max_strips, n_prob);
  if (p.dbg && !p.group64 && p.M == 1 && !p.bits3) {  // the two diagnostics instantiations: Llama-2-7B's forms
    if (nw == 8 && maxs == 16 && p.T == 128) return strip1_enqueue(strip1_form<Strip1Family<true, false>, 8, 16, true, false, 1, false>(), p, grid, nw, stream);
    if (nw == 15 && maxs == 24 && p.T < 360) return strip1_enqueue(strip1_form<Strip1Family<true, false>, 15, 24, false, false, 1, false>(), p, grid, nw, stream);
  }
  return strip1_launch<Strip1Family<false, false>>(p, nw, maxs, grid, stream);
}

}  // namespace qllm
