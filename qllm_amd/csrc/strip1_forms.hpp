// The forms of the batch-1 native-layout decode kernel (strip1_kernel.hpp), written once: which (waves, round) pairs are built, which
// forms of a pair, each form's second launch bound, and the one place that picks and launches an instantiation.  strip1_kernel.hpp
// includes this file (the launch bound); planner.hip includes it alone (the caps on the round).  A kernel family -- strip1.hip (plain,
// fused all-reduce), strip1_swiglu.hip, strip1_norm.hip, strip1_resid.hip, strip1_swiglu_resid.hip -- is a struct with
//   kWhat       the prefix of its refusal ("<kWhat>: no batch-1 instantiation for nw=.. round=..")
//   kLdsExtra   bytes of LDS behind strip1_lds_bytes
//   kRows4      whether it builds the four-row forms (M = 2..4)
//   kG64B3      whether it builds the 64-wide-group and the 3-bit forms
//   kMaxRound   its longest round
//   kernel<NW, MAXS, EXACT, G64, MR, B3>()   the __global__ function of one form
// and a launcher of its own that calls strip1_launch<Family>.  A new family writes that struct and nothing else.
#pragma once
#include "kernels.hpp"

namespace qllm {

// every (NW, MAXS) pair strip1_shape (strip1.hip) can answer
#define QLLM_STRIP1_PAIRS(X) \
  X(4, 8) X(4, 16) X(4, 32) X(8, 16) X(7, 16) X(8, 24) X(8, 32) X(16, 16) X(16, 24) X(15, 24) X(16, 32) X(16, 40) X(16, 48) X(16, 56) X(16, 64)

// Second launch bound (minimum waves per SIMD) of a form, of every family: 64 registers (8 waves per SIMD, a CU full of waves) for the
// plain forms up to rounds of 24 k-steps, 128 (4: what a 16-wave block needs anyway) for the rest.  Every fused form fits its plain
// twin's bound without scratch (-Rpass-analysis=kernel-resource-usage; DESIGN 3.10 .. 3.12 have the tables).
constexpr int strip1_min_waves(int maxs, bool g64, int mr, bool b3) { return (maxs <= 24 && !g64 && mr == 1 && !b3) ? 8 : 4; }

// Longest round (k-steps per wave) a form is built for: 3-bit forms (two word loads per k-step) and four-row forms (LDS: four staged
// rows per wave) 32, 64-wide groups 48 (56 spills a register with sixteen group addresses more), plain forms 64.  With strip1_shape's
// table a round of at most 32 is K <= 16384, of at most 48 K <= 24576.
constexpr int strip1_max_round(bool g64, int mr, bool b3) { return (b3 || mr > 1) ? 32 : (g64 ? 48 : 64); }

template <int NW, int MAXS, int MR>
constexpr int strip1_lds_bytes();   // strip1_kernel.hpp (the kernel's LDS layout)

using Strip1Kernel = void (*)(const Strip1Params);
struct Strip1Form {
  Strip1Kernel kernel;
  int lds_bytes;
  DeviceLatch *optin;   // the form's LDS opt-in (per kernel and device), or null: up to 64 KB
};

// One form of a family.  The template arguments ARE the form: nothing else says which kernel this is.
template <class F, int NW, int MAXS, bool EXACT, bool G64, int MR, bool B3>
Strip1Form strip1_form() {
  constexpr int lds_bytes = strip1_lds_bytes<NW, MAXS, MR>() + F::kLdsExtra;
  static_assert(lds_bytes <= 160 * 1024, "LDS of one CU");
  static DeviceLatch optin;   // (rounds of 56 / 64 k-steps x 16 waves, or four batch rows: the staged activations)
  return Strip1Form{F::template kernel<NW, MAXS, EXACT, G64, MR, B3>(), lds_bytes, lds_bytes > 64 * 1024 ? &optin : nullptr};
}

// the LDS opt-in, the launch and the check, for every form of every family
inline int strip1_enqueue(const Strip1Form &f, const Strip1Params &p, dim3 grid, int nw, hipStream_t stream) {
  if (f.optin)
    if (int rc = lds_optin(*f.optin, (const void *)f.kernel)) return rc;
  hipLaunchKernelGGL(f.kernel, grid, dim3(nw * 64), f.lds_bytes, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// (G64, MR, B3) of one pair -> the EXACT or the shifted-window form, where the family builds it (else *f stays empty).
// EXACT: NW * MAXS == p.T -- decided here and nowhere else.
template <class F, int NW, int MAXS, bool G64, int MR, bool B3>
void strip1_pick_exact(const Strip1Params &p, Strip1Form *f) {
  if constexpr (MAXS <= F::kMaxRound && MAXS <= strip1_max_round(G64, MR, B3) && (F::kRows4 || MR == 1) && (F::kG64B3 || (!G64 && !B3)))
    *f = (NW * MAXS == p.T) ? strip1_form<F, NW, MAXS, true, G64, MR, B3>() : strip1_form<F, NW, MAXS, false, G64, MR, B3>();
}

// 3-bit layers: batch 1, 64- and 128-wide groups; batches 2..4: the four-row forms, 128-wide groups; batch 1: 64- or 128-wide groups
template <class F, int NW, int MAXS>
void strip1_pick(const Strip1Params &p, Strip1Form *f) {
  if (p.bits3 && p.group64) strip1_pick_exact<F, NW, MAXS, true, 1, true>(p, f);
  else if (p.bits3) strip1_pick_exact<F, NW, MAXS, false, 1, true>(p, f);
  else if (p.M > 1) strip1_pick_exact<F, NW, MAXS, false, 4, false>(p, f);
  else if (p.group64) strip1_pick_exact<F, NW, MAXS, true, 1, false>(p, f);
  else strip1_pick_exact<F, NW, MAXS, false, 1, false>(p, f);
}

template <class F>
int strip1_launch(const Strip1Params &p, int nw, int maxs, dim3 grid, hipStream_t stream) {
  Strip1Form f{};
#define X(NW, MAXS) \
  if (nw == NW && maxs == MAXS) strip1_pick<F, NW, MAXS>(p, &f);
  QLLM_STRIP1_PAIRS(X)
#undef X
  if (!f.kernel) return set_error(QLLM_ERR_UNSUPPORTED, "%s: no batch-1 instantiation for nw=%d round=%d", F::kWhat, nw, maxs);
  return strip1_enqueue(f, p, grid, nw, stream);
}

}  // namespace qllm
