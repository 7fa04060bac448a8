// The preloading twins of the plain batch-1 forms (strip1_kernel.hpp): the same body, strip1_body.inc, behind another way to
// its hot words.  strip1_kernel's only argument is Strip1Params by value, a ~600-byte aggregate the compiler passes by reference: every
// wave of every launch starts with a batch of scalar loads from the kernel-argument segment -- through a scalar cache that is cold at a
// launch boundary -- and forms the address of its first vector load only when they are back.  gfx950 can hand a kernel its leading
// arguments in user SGPRs instead (kernel-argument preload; this unit alone is compiled with -mllvm -amdgpu-kernarg-preload-count, see
// the Makefile): 16 user SGPRs, 2 of them the kernel-argument pointer, so 14 words.  The twin spends them on everything a block of
// problem 0 reads, the cold words (bias, y) included:
//
//   x (2) | T (1) | word (1): n_strips << 8 | zero_kind << 2 | add_zero_bias << 1 | act_bf16 | qweight, scales, qzeros, bias, y (2 each)
//
// n_groups is not among them: these are the forms of 128-wide groups, where it is T / 4 (the launcher checks).  A block of problem 0 --
// every block of the o_proj and down_proj launches, a third of q/k/v, half of gate/up -- executes no scalar load at all.  The blocks of a
// later sibling issue their x chunks first (they need x and T only) and then read p.prob[blockIdx.y] in ONE batch of scalar loads, chosen
// by a scalar branch on blockIdx.y: one round trip as in the plain kernel, but behind the x loads instead of in front of them.  The
// surplus-block test follows the record (n_strips is part of it); x is [K] for every sibling, so the surplus block's loads are in bounds.
// The unchanged Strip1Params comes last (the record of the later siblings, dbg).
//
// Lab define QLLM_PRELOAD_XONLY: every block, problem 0 too, takes its record from the scalar loads behind the x chunks -- the "x only
// ahead of the wait" variant of profiles/strip1_preload.md.
#include "strip1_forms.hpp"
#include "strip1_kernel.hpp"

namespace qllm {

#ifdef QLLM_PRELOAD_XONLY
#define STRIP1_PRE_FROM_RECORD true
#else
#define STRIP1_PRE_FROM_RECORD (blockIdx.y != 0)
#endif

#define STRIP1_HOT_WORDS                                                                                                    \
  const void *const hw_x = a_x;                                                                                             \
  const int hw_T = a_T, hw_n_groups = a_T >> 2;                                                                             \
  const uint32_t *hw_qweight = a_qweight;                                                                                   \
  const half_t *hw_scales = (const half_t *)a_scales, *hw_bias = (const half_t *)a_bias;                                    \
  const void *hw_qzeros = a_qzeros;                                                                                         \
  void *hw_y = a_y;                                                                                                         \
  int hw_n_strips = (int)(a_word >> 8), hw_zero_kind = (int)((a_word >> 2) & 3u);                                           \
  int add_zero_bias = (int)((a_word >> 1) & 1u), act_bf16 = (int)(a_word & 1u);                                             \
  asm volatile("" : "+s"(add_zero_bias), "+s"(act_bf16));
// (the empty asm: one batch, as in QLLM_STRIP1_HOT_WORDS_KERNARG)
#define STRIP1_LATE_PROBLEM                                                                                                          \
  if (STRIP1_PRE_FROM_RECORD) {                                                                                                      \
    const Strip1Problem pr = p.prob[blockIdx.y];                                                                                     \
    asm volatile("" ::"s"(pr.qweight), "s"(pr.scales), "s"(pr.qzeros), "s"(pr.bias), "s"(pr.y), "s"(pr.n_strips), "s"(pr.zero_kind)); \
    hw_qweight = pr.qweight, hw_scales = pr.scales, hw_qzeros = pr.qzeros, hw_bias = pr.bias, hw_y = pr.y;                          \
    hw_n_strips = pr.n_strips, hw_zero_kind = pr.zero_kind;                                                                          \
  }

// <NW, MAXS, EXACT, DBG>: the plain form <NW, MAXS, EXACT, 2, 4, DBG> of strip1_kernel, same launch bounds.  (The fp16 pointers are
// void pointers in the signature: profilers' demanglers leave a name with _Float16 in it mangled, and the benchmark's counter pass
// selects dispatches by the demangled qllm::strip1_kernel...)
template <int NW, int MAXS, bool EXACT, bool DBG>
__global__ __launch_bounds__(NW * 64, strip1_min_waves(MAXS, false, 1, false)) void strip1_kernel_pre(
    const void *a_x, int a_T, uint32_t a_word, const uint32_t *a_qweight, const void *a_scales, const void *a_qzeros, const void *a_bias,
    void *a_y, const Strip1Params p) {
  constexpr bool SWIGLU = false, NORM = false, NORM_PARK = false, RESID = false, AR = false, G64 = false, B3 = false, PRELOAD = true;
  constexpr int NCH = 2, LVL = 4, MR = 1;
#include "strip1_body.inc"
}

#undef STRIP1_HOT_WORDS
#undef STRIP1_LATE_PROBLEM

using Strip1PreKernel = void (*)(const void *, int, uint32_t, const uint32_t *, const void *, const void *, const void *, void *, const Strip1Params);
struct Strip1PreForm {
  Strip1PreKernel kernel;
  int lds_bytes;
  DeviceLatch *optin;   // (as Strip1Form's: rounds of 56 / 64 k-steps x 16 waves)
};

template <int NW, int MAXS, bool EXACT, bool DBG>
static Strip1PreForm strip1_pre_form() {
  constexpr int lds_bytes = strip1_lds_bytes<NW, MAXS, 1>();
  static_assert(lds_bytes <= 160 * 1024, "LDS of one CU");
  static DeviceLatch optin;
  return Strip1PreForm{strip1_kernel_pre<NW, MAXS, EXACT, DBG>, lds_bytes, lds_bytes > 64 * 1024 ? &optin : nullptr};
}

// the launches the twins serve: the forms of strip1_pre_forms (a batch-1 launch is 3 or 4 bits, 64- or 128-wide groups), n_groups == T / 4
// (the word the twin derives), and the zero-point kind and the strip count of problem 0 inside their fields of the packed word.  A
// diagnostics launch (p.dbg) of a form without a DBG twin runs the form's plain twin and leaves its slots unwritten, as launch_strip1 does
bool strip1_pre_serves(const Strip1Params &p) {
  return strip1_pre_forms(p.M, p.bits3 ? 3 : 4, p.group64 ? 64 : 128) && p.T == 4 * p.n_groups && (unsigned)p.prob[0].zero_kind < 4u &&
         (unsigned)p.prob[0].n_strips < (1u << 24);
}

int launch_strip1_pre(const Strip1Params &p, int nw, int maxs, int n_prob, int max_strips, hipStream_t stream) {
  if (!strip1_pre_serves(p)) return set_error(QLLM_ERR_UNSUPPORTED, "strip1 preload: not a plain 4-bit batch-1 launch of 128-wide groups");
  Strip1PreForm f{};
  if (p.dbg && nw == 8 && maxs == 16 && p.T == 128) f = strip1_pre_form<8, 16, true, true>();   // (the two diagnostics forms of launch_strip1)
  else if (p.dbg && nw == 15 && maxs == 24 && p.T < 360) f = strip1_pre_form<15, 24, false, true>();
#define X(NW, MAXS) \
  else if (nw == NW && maxs == MAXS) f = (NW * MAXS == p.T) ? strip1_pre_form<NW, MAXS, true, false>() : strip1_pre_form<NW, MAXS, false, false>();
  QLLM_STRIP1_PAIRS(X)
#undef X
  if (!f.kernel) return set_error(QLLM_ERR_UNSUPPORTED, "strip1 preload: no batch-1 instantiation for nw=%d round=%d", nw, maxs);
  if (f.optin)
    if (int rc = lds_optin(*f.optin, (const void *)f.kernel)) return rc;
  const Strip1Problem &q = p.prob[0];
  const uint32_t word = ((uint32_t)q.n_strips << 8) | ((uint32_t)q.zero_kind << 2) | (p.add_zero_bias ? 2u : 0u) | (p.act_bf16 ? 1u : 0u);
  hipLaunchKernelGGL(f.kernel, dim3(max_strips, n_prob), dim3(nw * 64), f.lds_bytes, stream, p.x, p.T, word, q.qweight, (const void *)q.scales, q.qzeros, (const void *)q.bias, q.y, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
