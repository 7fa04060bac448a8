// The forward planner: the knob table, the predicates of every kernel family, the strip planner, the workspace-dependent splits,
// decide_single / decide_group and their text form.  Pure host code: no weight pointer is dereferenced and no kernel is launched here
// (capi.hip fills the parameter blocks and launches what is decided).  No global mutable state beyond the knob table.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "planner.hpp"
#include "strip1_forms.hpp"

namespace qllm {

// ---- tuning knobs: the measured defaults, qllm_set_knob() overrides, and -- lab builds only -- the environment (common.hpp) ---------
static int env_int(const char *name, int dflt) {
  const char *v = getenv(name);
  return (v && *v) ? atoi(v) : dflt;
}
// the planner thresholds a caller may move in a RELEASE build, with the range every built kernel instantiation covers
static Settable kSettable[] = {
    {"QLLM_STRIP1_3BIT", 0, 1, 0, 0},          // 0: 3-bit layers at batch 1 on the general strip kernel
    {"QLLM_STRIP1_MAX_M", 1, 4, 0, 0},         // 1: batches 2..4 on strip_dma instead of the batch-1 kernel's four-row forms
    {"QLLM_STRIP1", 0, 2, 0, 0},               // 0: batch-1 calls on the general strip kernel (the round-4 path); 2: only 128-wide groups on the batch-1 kernel
    {"QLLM_PANEL", 0, 1, 0, 0},                // 0: no panel kernel (strips to 32 rows, the 256-row tiles above)
    {"QLLM_PANEL_MIN_M", 17, 129, 0, 0},       // single layers: rows from which the panel kernel serves (no form below 17 rows)
    {"QLLM_PANEL_GROUP_MIN_M", 17, 129, 0, 0}, // sibling groups: rows from which ONE panel launch serves the group
    {"QLLM_GEMM2", 0, 1, 0, 0},                // 0: no 256-row register-staged tiles (the 128 x 128 kernel instead)
    {"QLLM_GEMM3", 0, 1, 0, 0},                // 0: no wave-specialised prefill kernel
    {"QLLM_GEMM2_MIN_M", 33, 1 << 30, 0, 0},   // rows from which the 256-row tiles serve what the strips leave alone
    {"QLLM_GEMM3_MIN_M", 0, 1 << 30, 0, 0},    // rows from which gemm3 takes over from gemm2 (0: the measured line, 384 / 768)
    {"QLLM_GEMM2_SPLITK", 0, 1, 0, 0},         // 0: never split K over blocks in the tile GEMMs
    {"QLLM_GEMM3_TAIL", 0, 1, 0, 0},           // 0: no K-split of the ragged last round of tiles (gemm3.hip, round 6)
    {"QLLM_GEMM3_GROUP", 0, 1, 0, 0},          // 0: no grouped launches of the prefill kernel (q/k/v, gate/up run layer by layer from 129 rows)
    {"QLLM_GEMM3_BF16", 0, 1, 0, 0},           // 0: bf16 prefill through the fp16 conversion pre-pass (the reference's shim) instead of bf16 MFMA
    {"QLLM_SKINNY_MAX_M", 0, 64, 0, 0},        // rows up to which the split-K decode kernel serves the reference layouts in place
    {"QLLM_STRIP_MIN", 0, 1 << 20, 0, 0},      // fewest 16-column strips the full-K strip kernels take (0: never)
    {"QLLM_S1_T256_NW16", 0, 1, 0, 0},         // 1: the batch-1 kernel takes K = 6272..8192 with 16 waves x 16 k-steps instead of 8 x 32 (every form table builds both)
    {"QLLM_BITGEMV", 0, 1, 0, 0},              // 0: 2 / 5 / 6 / 7 / 8-bit decode calls refused (callers then dequantise + GEMM: the reference's branch)
    // (no route: the two knobs of qllm_linear_forward_bitpanel, bitpanel.hip)
    {"QLLM_BITPANEL", 0, 1, 0, 0},             // 0: the mid-batch entry refuses every call
    {"QLLM_BITPANEL_LDS", 0, 1, 0, 0},         // 1: that kernel stages the packed words through LDS (the ingest that lost the A/B: profiles/bitpanel.md)
    {"QLLM_BITPANEL_MAX_M", 17, 512, 0, 0},    // read by callers that route by rows (the Python modules): the most rows they send to that entry
    // (no route: the two knobs of qllm_linear_forward_bitgroup, bitgemv_group.hip)
    {"QLLM_BITGROUP", 0, 1, 0, 0},             // 0: the grouped bit-stream entry refuses every call
    {"QLLM_BITGROUP_MAX_M", 0, 16, 0, 0},      // read by callers that route by rows (the Python modules): the most rows they send to that entry (0: never)
    // (no route: the two knobs of qllm_linear_forward_bitgemm, bitgemm.hip)
    {"QLLM_BITGEMM", 0, 1, 0, 0},              // 0: the 2..8-bit prefill entry refuses every call
    {"QLLM_BITGEMM_MIN_M", 129, 65536, 0, 0},  // read by callers that route by rows (the Python modules): the fewest rows they send to that entry
    // (no route: qllm_gather_columns, gather.hip)
    {"QLLM_GATHER_ROWS", 0, 1, 0, 0},          // 0: every row count on the row-at-a-time gather (no several-rows-per-step kernel from 64 rows)
};
int g_knob_overrides = 0;
Settable *find_knob(const char *name) {
  for (Settable &k : kSettable)
    if (strcmp(k.name, name) == 0) return &k;
  return nullptr;
}
void reset_knobs() {
  for (Settable &k : kSettable) k.set = 0;
  __atomic_store_n(&g_knob_overrides, 0, __ATOMIC_RELAXED);
}
int knob_override(const char *name, int dflt) {
  for (const Settable &k : kSettable)
    if (k.set && strcmp(k.name, name) == 0) return k.value;
  return dflt;
}
#ifdef QLLM_LAB
int knob(const char *name, int dflt) { return g_knob_overrides ? knob_override(name, env_int(name, dflt)) : env_int(name, dflt); }
#endif
// CUs of the current device (launch heuristics only); 256 (MI355X) when no device is reachable, so that the pure-host
// planners (qllm_plan_describe, qllm_workspace_bytes) stay deterministic without a GPU.  QLLM_NUM_CU overrides.
int compute_units() {
  static int v = [] {
    int e = env_int("QLLM_NUM_CU", 0);
    if (e > 0) return e;
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) return n;
    (void)hipGetLastError();
    return kNumCU;
  }();
  return v;
}
static int skinny_target_waves() { return knob("QLLM_SKINNY_WAVES", 2048); }
static int skinny_awq_w(int M) { return (M <= 16 && knob("QLLM_SKINNY_AWQ_W", 1) == 2) ? 2 : 1; }
static int skinny_max_m() { return std::min(knob("QLLM_SKINNY_MAX_M", 64), 64); }
static int strip_min_strips() {
  // measured (profiles/r02_narrow_shapes.md): even 8-80 strips beat the split-K kernel's three dependent round trips
  // (K=8192, N=1024+128+128: 15.2 -> 9.8 us; K=4096, N=1024: 11.7 -> 4.8 us)
  return knob("QLLM_STRIP_MIN", 8);
}

// ---- per-layer predicates --------------------------------------------------------------------------------------------------------------
// the buffers every fused kernel reads with 16-byte (packed zero points: 8-byte) loads
static bool ptrs_aligned(const qllm_weight_t &w) {
  return (uintptr_t)w.qweight % 16 == 0 && (uintptr_t)w.scales % 16 == 0 && (!w.qzeros || (uintptr_t)w.qzeros % 8 == 0);
}
static bool fused_common_ok(const qllm_weight_t &w) {
  return !is_native(w) && w.bits == 4 && w.N % 8 == 0 && w.group_size % 8 == 0 && ptrs_aligned(w);
}
static bool skinny_ok(const qllm_weight_t &w, int M) {
  return M <= skinny_max_m() && fused_common_ok(w) && w.K % 32 == 0 && w.g_idx == nullptr;
}
static bool gemm_ok(const qllm_weight_t &w) {
  if (!fused_common_ok(w) || w.K % 64 != 0) return false;
  if (w.layout == QLLM_LAYOUT_AWQ_GEMM) return w.group_size % 4 == 0;
  if (w.g_idx) {
    const int groups = (w.K + w.group_size - 1) / w.group_size;
    return (size_t)groups * 128 * 4 + 65536 <= 160 * 1024;
  }
  return true;
}
// layouts that may share a grouped launch: reference row-stream (GPTQ / HQQ), AWQ, native
static int layout_family(const qllm_weight_t &w) { return is_native(w) ? 2 : (w.layout == QLLM_LAYOUT_AWQ_GEMM ? 1 : 0); }

void fill_gemm_params(GemmParams &p, const qllm_weight_t *w, const void *x, void *y, int M, int act_dtype) {
  fill_call(p, *w, x, M, act_dtype);
  fill_layer(p, *w, y);
  p.g_idx = w->g_idx;
  p.K = w->K;
  p.N = w->N;
  p.group_size = w->group_size;
  p.gs_shift = ((w->group_size & (w->group_size - 1)) == 0) ? __builtin_ctz((unsigned)w->group_size) : -1;
  p.n_groups = (w->K + w->group_size - 1) / w->group_size;
  p.sm = is_native(*w) ? 1 : 0;
  p.split_k = 1;
}

// ---- the panel kernel's share ------------------------------------------------------------------------------------------------------------
// the mid-batch panel kernel (panel.hip): single native layers from QLLM_PANEL_MIN_M (17) rows to 128.  us per linear, strips -> panel
// (profiles/r04_mid_m.md): M = 32: 23.8 -> 15.9 (4096 x 11008), 20.8 -> 16.0 (11008 x 4096).
// Round 5 (profiles/r05_batch16.md, tools/rounds5/g13_down_sweep.sh), after the strips' scale / zero tables moved to LDS:
//   * 9..16 rows where K >= 2 N (down_proj) went BACK to the strips: 15.0 -> 12.6-14.4 us (HQQ g64 4 bits), 16.5 -> 14.1-15.0 (3 bits),
//     13.5 -> 11.9-13.1 (g128): the split-K fix-up of the panel costs more than the one-strip blocks' x traffic now;
//   * 17..32 rows on layers of up to 4096 x 4096 (o_proj) stay on the two-row-tile strips: 9.1-9.7 -> 7.7-8.9 us (3 bits 10.3 -> 8.2-9.9).
static bool panel_rows_ok(int M, int K, int N) {
  if (M < knob("QLLM_PANEL_MIN_M", 17)) return false;  // (lab builds only: below 17 rows the release library has no panel form)
  if (M <= 32 && K <= 4096 && N <= 4096 && !knob("QLLM_PANEL_SMALL", 0)) return false;
  return true;
}
// prefill-sized calls (M > 64) on native-layout layers: the same tile GEMMs, their staging waves reading the strip-major words
// every layer of the launch: native strip-major, 4 bits, no act-order, whole 64-column panels; the group: one K / group size
static bool panel_layers_ok(const qllm_weight_t *w, int n, int M) {
  if (!knob("QLLM_PANEL", 1) || n < 1 || n > kMaxProblems) return false;
  for (int i = 0; i < n; ++i) {
    if ((w[i].bits != 4 && w[i].bits != 3) || w[i].bits != w[0].bits || !is_native(w[i]) || w[i].g_idx || w[i].K != w[0].K || w[i].group_size != w[0].group_size) return false;
    if (!panel_shape_ok(M, w[i].K, w[i].N, w[i].group_size, w[i].bits)) return false;
    // (one launch decodes every layer's zero points the same way: fp16 zero points and packed / symmetric ones do not mix -- such a
    //  group goes to the strips, which decide per layer, or runs layer by layer)
    if ((zero_kind_of(w[i]) == ZK_F16) != (zero_kind_of(w[0]) == ZK_F16)) return false;
    if (!ptrs_aligned(w[i])) return false;
  }
  return true;
}
// 65..128 rows (eight row tiles, one K half per block): only where it pays whatever the activation type -- us per linear, fp16 / bf16,
// against gemm2's 28 / 40 / 41 (+1-2 for bf16): 4096 x 4096 19 / 25; 4096 x 11008 36-38 / 50; 11008 x 4096 35 / 44 -> layers of up to
// 2^25 weights; groups (three launches become one: q/k/v 41 against 84) of up to 16384 columns.  profiles/r04_mid_m.md
static bool panel_serves(const qllm_weight_t *w, int M) {
  if (M > 64 && (double)w->K * w->N > 33554432.0) return false;
  return panel_rows_ok(M, w->K, w->N) && panel_layers_ok(w, 1, M);
}
// grouped launches (q/k/v, gate/up): from 17 rows -- the strips keep the smaller batches (BASELINE configs[3] is tuned there)
static bool panel_group_serves(const qllm_weight_t *w, int n, int M) {
  if (n <= 1 || M < knob("QLLM_PANEL_GROUP_MIN_M", 17) || !panel_layers_ok(w, n, M)) return false;
  if (M > 64) {
    int cols = 0;
    for (int i = 0; i < n; ++i) cols += w[i].N;
    if (cols > 16384) return false;
  }
  return true;
}
static int panels_of(const qllm_weight_t *w, int n) {
  int t = 0;
  for (int i = 0; i < n; ++i) t += w[i].N / 64;
  return t;
}

// ---- the strip planner: strip_plan tries the sub-planners below in order; each either leaves the call alone or writes a whole StripPlan ---
// the rows the strips serve at all, by shape
static int strip_row_limit(const qllm_weight_t *w, int n) {
  // measured (graph replay, us; split-K kernel -> strips with 2 / 4 row tiles): M=32: 4096x4096 28.3 -> 13.4, 4096x11008 54.9 -> 36.3,
  // 11008x4096 50.1 -> 30.3; M=64: 33.8 -> 22.6, 52.5 -> 61.5, 48.1 -> 53.9 -- four row tiles only pay on the small shape
  // M = 33..64 (four row tiles), us per linear, split-K kernel -> strips (profiles/r02_mid_m.md): 4096x4096 26.8/31.4/33.5 ->
  // 17.6/19.8/22.6 at M = 33/48/64; on the 11008-wide shapes the strips lose at M >= 48 (43.9 -> 55.1, 41.2 -> 49.8): small shape only
  const int max_m = knob("QLLM_STRIP_MAX_M", 0);
  int cols_all = 0;
  for (int i = 0; i < n; ++i) cols_all += w[i].N;
  // (native layout, round 3, profiles/r03_mid_m.md: four row tiles 17-21 us vs gemm2 27-28 on 4096 x 4096; 46-59 and 43-54 vs
  //  40 on the 11008-wide shapes: the same line as for the reference layouts)
  return max_m ? max_m : ((w[0].K <= 4096 && cols_all <= 4096 && !(is_native(w[0]) && w[0].bits == 3)) ? 64 : 32);
}
// a call within the strips' rows that the panel kernel serves goes there (the panel kernel's own conditions decide: a group it will NOT
// take -- e.g. fp16 and packed zero points mixed -- stays on the strips, which decode zero points per layer)
static bool panel_takes_instead(const qllm_weight_t *w, int n, int M) {
  // (single native 4-bit layers: the panel kernel takes over where it is served -- panel.hip; grouped launches stay here)
  if (n == 1) return panel_rows_ok(M, w[0].K, w[0].N) && panel_layers_ok(w, 1, M);  // (M <= 64 here)
  // (groups from 17 rows: ONE grouped launch of the panel kernel -- q/k/v 21.8-23.2 us on the two-row-tile strips, 25.2 layer by layer;
  //  gate/up 40-43.5 / 29.4.  profiles/r04_mid_m.md)
  return panel_group_serves(w, n, M);
}
// the layers can share one strip launch; their columns in total, and whether every layer is a multiple of 64 / 32 wide
struct StripCols {
  int cols;
  bool m64, m32;
};
static bool strip_layers_ok(const qllm_weight_t *w, int n, int M, StripCols *c) {
  if (M > 64 || strip_min_strips() <= 0) return false;
  const int bits = w[0].bits;
  const bool sm = is_native(w[0]);
  if (bits != 4 && bits != 3) return false;
  if (!strip_group_ok(w[0].group_size, sm, bits)) return false;
  c->cols = 0;
  c->m64 = c->m32 = true;
  for (int i = 0; i < n; ++i) {
    if (w[i].bits != bits || w[i].K % 32 != 0 || w[i].g_idx || is_native(w[i]) != sm) return false;
    // 3-bit: fp16 (HQQ), symmetric, or packed zero points (a column's field may straddle two words of the N*3/32-word row)
    if (bits == 3 && !sm && !(w[i].layout == QLLM_LAYOUT_HQQ || w[i].layout == QLLM_LAYOUT_GPTQ)) return false;
    if (bits == 3 && w[i].layout == QLLM_LAYOUT_GPTQ && w[i].qzeros && w[i].N % 32 != 0) return false;
    if (!ptrs_aligned(w[i])) return false;
    if (w[i].layout == QLLM_LAYOUT_AWQ_GEMM || w[i].N % 16 != 0) return false;
    c->cols += w[i].N;
    c->m64 = c->m64 && (w[i].N % 64 == 0);
    c->m32 = c->m32 && (w[i].N % 32 == 0);
  }
  return true;
}
// 1: the register-A form by row count
static int strip_ra_base(int M) {
  // rows from which the activation slab in LDS (staged once per block: M*K/8 chunk operations) loses to per-lane
  // fragment loads + two bookkeeping MFMAs per k-step (strip_kernel.hpp, RA)
  // measured (graph replay, us; slab -> RA): 4096x4096 M=4 5.3 -> 6.2, M=8 9.6 -> 7.1, M=16 9.9 -> 8.5; 4096x11008 M=4 9.8 -> 9.3,
  // M=8 10.0 -> 9.7, M=16 25.7 -> 11.9; 11008x4096 M=4 13.6 -> 13.0, M=8 20.2 -> 14.6, M=16 26.4 (split-K fallback) -> 18.9
  const int ra_min = knob("QLLM_STRIP_RA_MIN", 5);
  return (M >= ra_min) ? 1 : 0;
}
static bool strip_longk(const qllm_weight_t &w) {
  // long K with 64-wide groups or 3 bits: the one-round slab variant (24 loads + 12 scale/zero pairs per lane) spills
  // 17-21 registers in a 16-wave block; the register-A variant (rounds of 8) does not
  const int ra_longk = knob("QLLM_STRIP_RA_LONGK", 1);
  return ra_longk && (w.group_size <= 64 || w.bits == 3) && strip_spw(w.K, w.group_size, 16) > 8;
}
static bool take(StripPlan *plan, int cpl, int nw, int spw, int ra, int sm) {
  *plan = StripPlan{cpl, nw, spw, ra, sm, plan->one_nw, plan->one_maxs};
  return true;
}

// Round 6: batches 2..4 on the batch-1 kernel's four-row forms (128-wide groups, as far as their rounds go): the A rows that carry four copies of x
// at batch 1 carry four batch rows -- the weight stream and the MFMAs of a batch-1 launch.  QLLM_STRIP1_MAX_M = 1 keeps them on strip_dma.
static bool plan_strip1_rows4(const qllm_weight_t *w, int M, int strips, StripPlan *plan) {
  if (!(M >= 2 && M <= 4 && M <= knob("QLLM_STRIP1_MAX_M", 4) && w[0].bits == 4 && w[0].group_size == 128 && knob("QLLM_STRIP1", 1))) return false;
  int nw1 = 0, maxs1 = 0;
  if (!strip1_shape(w[0].K, strips, compute_units(), &nw1, &maxs1) || maxs1 > strip1_max_round(false, 4, false)) return false;
  plan->one_nw = nw1;
  plan->one_maxs = maxs1;
  return take(plan, 1, nw1, maxs1, 0, 1);
}

// strip_dma.hpp (M = 5..32, K a multiple of 64): the activations go through LDS by DMA.  A block pulls the activations of its
// k range through the CU's memory pipe once, a CU ingests ~55 GB/s here, so the launch costs about (rounds of blocks on the
// CUs) x (a block's fixed life + the bytes it pulls): blocks of cpl strips share one activation stream -- pick the cpl that minimises that product
// (profiles/r03_batch16.md).  One strip per block: 16 waves; several: 8 waves (registers).  The last block of a layer may be ragged.
static bool strip_dma_applies(const qllm_weight_t *w, int n, int M) {
  const int ra_xd = knob("QLLM_RA_XD", 1);
  // From batch 2: the lds-slab forms stage M x K / 8 chunks per block and run one-strip blocks in several rounds on wide launches
  // (4 bits g128 at M = 4: q/k/v 14.3 -> 10.5 us, gate/up 24.7 -> 14.1; 64-wide groups had only the register-A form there: gate/up
  // 25 -> 18; 3 bits: q/k/v 26.6 -> 13.5, gate/up 49 -> 24).  Batch 1 never: the one-round slab forms win (profiles/r03_batch16.md).
  const int dma_min_m = knob("QLLM_DMA_MIN_M", 2);
  const int dma_from = dma_min_m < 2 ? 2 : dma_min_m;
  bool small_enough = true;  // (the kernel's byte offsets are 32-bit)
  for (int i = 0; i < n; ++i) small_enough = small_enough && (double)w[i].K * w[i].N * w[0].bits / 8 < 2147483648.0;
  return ra_xd && small_enough && M >= dma_from && M >= 2 && M <= 32 && w[0].K % 64 == 0;
}
static bool plan_strip_dma(const qllm_weight_t *w, int n, int M, StripPlan *plan) {
  const int K = w[0].K, gs = w[0].group_size, bits = w[0].bits, cus = compute_units();
  const bool g32 = gs == 32;  // (native layout, 4 bits: one strip per block, lds-slab at batch 1, register-A above)
  const int dma_cpl = knob("QLLM_DMA_CPL", 0);
  // (round 5: three strips -- q/k/v's 768 strips are 256 blocks of three, every CU busy, instead of 192 of four; six 3-bit strips where
  //  the ring fits the registers: 64-wide groups with fp16 zero points, HQQ -- gate/up's 1376 strips in ONE round of 230 blocks
  //  instead of 344 blocks of four in two.  profiles/r05_batch16.md)
  static const int cands[] = {1, 2, 3, 4, 6};
  bool all_f16z = gs == 64;
  for (int i = 0; i < n; ++i) all_f16z = all_f16z && w[i].layout == QLLM_LAYOUT_NATIVE_F16Z && w[i].qzeros;
  const int n_cands = (M > 16) ? 1 : (g32 ? 2 : (bits == 4 ? 5 : (all_f16z ? 5 : 4)));  // (two row tiles: one strip per block; 3 bits: four strips unless fp16 zeros at g64; 32-wide groups: two)
  const double x_bytes = (double)M * K * 2, strip_bytes = (double)K * bits * 2 + (double)(K / gs) * 64;
  int best = 0;
  double best_cost = 0;
  // a candidate must fit the LDS: the waves' rings + (round 5) their scale / zero-point tables, which grow with K and the width
  auto dma_fits = [&](int c) {
    const int nw_c = (c == 1 && M <= 16) ? 16 : 8;
    const int spw_c = (strip_spw(K, gs, nw_c) + 1) & ~1;
    return strip_lds_bytes(M, spw_c, nw_c, c, gs, 2, 1) <= 156 * 1024;
  };
  for (int ci = 0; ci < n_cands; ++ci) {
    const int c = cands[ci];
    if (!dma_fits(c)) continue;
    int blocks = 0;
    for (int i = 0; i < n; ++i) blocks += (w[i].N / 16 + c - 1) / c;
    // (+ 96 KB per round: the ~1.8 us a block lives before and after its stream, at the CU's ingest rate)
    const double cost = (double)((blocks + cus - 1) / cus) * (96.0 * 1024 + x_bytes + c * strip_bytes);
    if (best == 0 || cost < best_cost * 0.97) { best = c; best_cost = cost; }  // (wider only for a clear gain)
    if (c == dma_cpl) { best = c; break; }                                    // (experiments: QLLM_DMA_CPL forces a width)
  }
  const int cpl = best ? best : 1;
  // (32-wide groups, one strip per block, short K, few rows: the register-A form's 8-k-step rounds beat the three-slot ring --
  //  4096 x 4096 at M = 4: 6.2 vs 7.7 us, M = 16: 7.8 both; tools/g32_bench.py, profiles/logs/r04r_g32_bench.log)
  const bool g32_ra = g32 && cpl == 1 && M <= 8 && K <= 4096;
  const int nw = (cpl == 1 && M <= 16) ? 16 : 8;
  const int spw = (strip_spw(K, gs, nw) + 1) & ~1;  // (the ring's slots are pairs of k-steps; only 32-wide groups can give an odd chunk)
  if (g32_ra || strip_lds_bytes(M, spw, nw, cpl, gs, 2, 1) > 156 * 1024) return false;  // (does not fit: the register-A form below)
  return take(plan, cpl, nw, spw, 2, 1);
}

// batch 1, 4 bits, 128-wide groups: the specialised kernel (round 5; profiles/r05_decode_bisect.md) in place of the general form planned
static void upgrade_to_strip1(const qllm_weight_t &w, int M, int strips, StripPlan *plan) {
  int nw1 = 0, maxs1 = 0;
  // (round 6: 64-wide groups too -- HQQ's default; QLLM_STRIP1 = 2 keeps them on the general kernel)
  const int s1 = knob("QLLM_STRIP1", 1);
  // (round 6: 3-bit layers too -- batch 1; QLLM_STRIP1_3BIT = 0 keeps them on the general kernel)
  const bool w4 = w.bits == 4 && (w.group_size == 128 || (w.group_size == 64 && s1 != 2));
  const bool w3 = w.bits == 3 && (w.group_size == 128 || w.group_size == 64) && knob("QLLM_STRIP1_3BIT", 1);
  // (round 7: K % 128 == 64 -- Falcon-7B's 4544 -- on the 4-bit 64-wide-group forms: strip1_shape)
  // (as far as the form's rounds go, strip1_forms.hpp: 3 bits K <= 16384, 64-wide groups K <= 24576)
  if (M == 1 && (w4 || w3) && s1 && strip1_shape(w.K, strips, compute_units(), &nw1, &maxs1, w4 && w.group_size == 64) &&
      maxs1 <= strip1_max_round(w.group_size == 64, 1, w.bits == 3)) {
    plan->one_nw = nw1;
    plan->one_maxs = maxs1;
  }
}
// the native layout's lds-slab and register-A forms.  `after_dma`: strip_dma was asked first and its ring did not fit
static bool plan_strip_native(const qllm_weight_t *w, int M, const StripCols &c, bool after_dma, StripPlan *plan) {
  const int K = w[0].K, gs = w[0].group_size, bits = w[0].bits;
  const bool g32 = gs == 32;  // (native layout, 4 bits: one strip per block, lds-slab at batch 1, register-A above)
  const bool longk = strip_longk(w[0]);
  const int slab_nw = strip_ra_base(M) ? 0 : strip_sm_nw(K, M, gs, bits);  // 0: no slab form for this shape
  // register-A form at M = 5..16, 4 bits, every layer a multiple of 64 wide and enough of them: blocks of four adjacent strips
  // (a register-A block re-reads all of x from L2; 64 columns share it instead of 16)
  const int sm_ra_cpl4 = knob("QLLM_SM_RA_CPL4", 1);
  // (3 bits: two strips -- four need more than 256 registers)
  const int cpl = (!after_dma && sm_ra_cpl4 && !g32 && slab_nw == 0 && M >= 5 && M <= 16 && c.m64 && c.cols / 64 >= compute_units() / 2) ? (bits == 3 ? 2 : 4) : 1;
  int nw = after_dma ? (M > 16 ? 8 : 16) : ((M > 16 || cpl > 1) ? 8 : (slab_nw ? slab_nw : 16));
  for (int tries = 0; tries < 2; ++tries) {
    const int spw = strip_spw(K, gs, nw);
    const int ra = (slab_nw == 0 || (longk && nw == 16)) ? 1 : 0;
    if (!ra && K / 32 < strip_maxs(nw, spw, 1, 0, 1)) return false;  // a round's window must fit into the strip
    if ((ra || strip_x_ok(M, spw, nw, 1, 1)) && strip_lds_bytes(M, spw, nw, cpl, gs, ra, 1) <= 156 * 1024) {
      upgrade_to_strip1(w[0], M, c.cols / 16, plan);
      return take(plan, cpl, nw, spw, ra, 1);
    }
    if (nw == 16 || M > 16 || cpl > 1) break;
    nw = 16;  // shorter per-wave chunks
  }
  return false;
}

// the reference row-stream layouts (GPTQ / HQQ in place)
static bool plan_strip_rowstream(const qllm_weight_t *w, int M, const StripCols &c, StripPlan *plan) {
  const int K = w[0].K, gs = w[0].group_size, bits = w[0].bits, cus = compute_units();
  const int ra_base = strip_ra_base(M);
  const bool longk = strip_longk(w[0]);
  int force_cpl = knob("QLLM_STRIP_CPL", 0);
  int first = (bits == 3 || M > 16) ? 1 : strip_cpl(c.cols, c.m64, c.m32 && M <= 4, cus);
  if (M > 16) force_cpl = 1;  // several row tiles per block: 16-column strips, 8-wave blocks, register-A
  if (force_cpl == 4 && c.m64 && bits == 4) first = 4;
  if (force_cpl == 2 && c.m32 && bits == 4) first = 2;
  if (force_cpl == 1) first = 1;
  // candidates: the measured-best strip width first; if its activation slab does not fit in LDS (many rows), narrower
  // strips with 16 waves (each wave stages a shorter K chunk)
  const int cand_cpl[2] = {first, 1};
  for (int ci = 0; ci < 2; ++ci) {
    const int cpl = cand_cpl[ci];
    if (ci >= 1 && cpl == cand_cpl[ci - 1]) continue;
    const int strips = c.cols / (16 * cpl);
    if (cpl == 1 && strips < strip_min_strips()) continue;
    // 64-column strips use 128 VGPRs -> 16 waves per CU: 8-wave blocks keep two strips co-resident per CU (one
    // round) instead of 16-wave blocks in two rounds (gate/up 15.6 -> 13.8 us, q/k/v 8.5 -> 8.3 us)
    int nw = cpl == 4 ? 8 : ((cpl == 2 || bits == 3) ? 16 : strip_nw(K, strips, cus));
    if (M > 16) nw = 8;
    for (int tries = 0; tries < 2; ++tries) {
      const int spw = strip_spw(K, gs, nw);
      const int ra = (ra_base || (longk && cpl == 1 && nw == 16)) ? 1 : 0;
      if ((ra || strip_x_ok(M, spw, nw, cpl, 0)) && strip_lds_bytes(M, spw, nw, cpl, gs, ra, 0) <= 156 * 1024) return take(plan, cpl, nw, spw, ra, 0);
      if (nw == 16 || M > 16 || cpl == 4) break;  // (64-column strips exist as 8-wave blocks only)
      nw = 16;  // shorter per-wave chunks
    }
  }
  return false;
}

bool strip_plan(const qllm_weight_t *w, int n, int M, StripPlan *plan) {
  *plan = StripPlan{};
  StripCols c;
  if (M > strip_row_limit(w, n) || panel_takes_instead(w, n, M) || !strip_layers_ok(w, n, M, &c)) return false;
  if (!is_native(w[0])) return plan_strip_rowstream(w, M, c, plan);
  // strip-major: 16-column strips only (every wave-load is 256 contiguous bytes whatever the width; narrow strips balance best)
  if (plan_strip1_rows4(w, M, c.cols / 16, plan)) return true;
  const bool dma = strip_dma_applies(w, n, M);
  if (dma && plan_strip_dma(w, n, M, plan)) return true;
  return plan_strip_native(w, M, c, dma, plan);
}

SkinnyPlan plan_skinny(const qllm_weight_t *w, int n, int M) {
  SkinnyPlan s;
  s.awq_w = skinny_awq_w(M);
  s.tile_cols = skinny_tile_cols(w[0].layout, s.awq_w);
  s.tiles_total = 0;
  for (int i = 0; i < n; ++i) s.tiles_total += (w[i].N + s.tile_cols - 1) / s.tile_cols;
  skinny_plan(w[0].K, M, s.tiles_total, skinny_target_waves(), &s.S, &s.spw);
  return s;
}

// ---- sub-decisions that depend on the caller's workspace (planner.hpp) ----------------------------------------------------------------
// the workspace holds the partial results behind its counters, and the counters cover every tile that is split
static bool split_fits(size_t ws_bytes, size_t slab_bytes, int counters) {
  return ws_bytes >= kCounterBytes + slab_bytes && counters <= (int)(kCounterBytes / sizeof(int));
}
// gemm3 over K-split blocks when the 256x128 tiling leaves CUs idle and the workspace can hold the partial tiles: the split, or 1
// (round 7: a half-wide last column tile is a tile -- and a 256x128 slab -- of its own: gemm3_tile_cols)
int gemm3_split_for(int M, int N, int K, size_t ws_bytes) {
  const int S = gemm3_split_k(M, N, K);
  if (S <= 1 || !split_fits(ws_bytes, gemm2_slab_bytes(M, gemm3_tile_cols(N), S), tiles_256x128(M, gemm3_tile_cols(N)))) return 1;
  return S;
}
static int gemm2_split_for(int M, int N, int K, size_t ws_bytes) {
  const int S = gemm2_split_k(M, N, K);
  if (S <= 1 || !split_fits(ws_bytes, gemm2_slab_bytes(M, N, S), tiles_256x128(M, N))) return 1;
  return S;
}
int panel_split_for(int M, int n_panels, int K, size_t ws_bytes) {
  const int S = panel_split_k(M, n_panels, K);
  if (S <= 1 || !split_fits(ws_bytes, panel_slab_bytes(M, n_panels, S), n_panels)) return 1;
  return S;
}
int bitgemv_split_for(int M, int K, int N, size_t ws_bytes) {
  const int S = bitgemv_split(M, K, N);
  if (S <= 1 || !split_fits(ws_bytes, (size_t)S * M * N * sizeof(float), (N + 15) / 16)) return 1;
  return S;
}
// gemm3's K-split of the ragged last round (gemm3.hip, round 6): the factor (1: none) and the first split tile
static size_t gemm3_tail_slab_bytes(int tail_tiles, int TS) { return TS > 1 ? (size_t)tail_tiles * TS * 256 * 128 * sizeof(float) : 0; }
static int tail_that_fits(int TS, int tiles, size_t ws_bytes, int *tail_from) {
  if (TS > 1 && split_fits(ws_bytes, gemm3_tail_slab_bytes(tiles - *tail_from, TS), tiles - *tail_from)) return TS;
  *tail_from = tiles;
  return 1;
}
static int gemm3_tail_for(int M, int N, int K, size_t ws_bytes, int *tail_from) {
  return tail_that_fits(gemm3_tail_split(M, N, K, tail_from), tiles_256x128(M, gemm3_tile_cols(N)), ws_bytes, tail_from);
}
static int group_tiles(const qllm_weight_t *w, int n, int M) {
  int t = 0;
  for (int i = 0; i < n; ++i) t += tiles_256x128(M, w[i].N);
  return t;
}
int tile_group_tail_for(const qllm_weight_t *w, int n, int M, size_t ws_bytes, int *tail_from) {
  const int tiles = group_tiles(w, n, M);
  return tail_that_fits(gemm3_tail_split_tiles(tiles, w[0].K, tail_from), tiles, ws_bytes, tail_from);
}

// bytes of the fp16 copy of bf16 activations gemm3 reads (0 for fp16 activations), and where it sits in the workspace
static size_t bf16_copy_bytes(int M, int K, int act_bf16) { return act_bf16 ? align_up((size_t)M * K * 2, 256) : 0; }

// large M: the wave-specialised 256x128 kernel (no split-K needed: every CU has at least one tile), also where it can split K; gemm2
// below.  bf16 activations: gemm3's activation tiles travel by LDS-DMA, which cannot convert, so x is converted to fp16 once into the
// workspace (the reference's own shim does the same cast, quant_linear_awq.py:29-36) and the epilogue rounds the fp16 result to bf16 --
// which needs room for the copy, else gemm2 (which converts in registers)
TileChoice choose_tile(const GemmParams &p, int layout, size_t ws_bytes) {
  GemmParams q = p;
  q.act_bf16 = 0;
  if (gemm3_ok(q, layout)) {
    const int S3 = gemm3_split_for(p.M, p.N, p.K, ws_bytes);
    if (gemm2_split_k(p.M, p.N, p.K) == 1 || S3 > 1) {
      const int native = p.act_bf16 && gemm3_bf16_native(layout);
      const size_t copy = native ? 0 : bf16_copy_bytes(p.M, p.K, p.act_bf16);
      const int tiles = tiles_256x128(p.M, gemm3_tile_cols(p.N));
      int tail_from = tiles;
      // (the slabs of the tail split and the fp16 copy of bf16 activations share the workspace: the copy comes first)
      const int TS = S3 > 1 ? 1 : gemm3_tail_for(p.M, p.N, p.K, ws_bytes > copy ? ws_bytes - copy : 0, &tail_from);
      const size_t used = kCounterBytes + (S3 > 1 ? align_up(gemm2_slab_bytes(p.M, gemm3_tile_cols(p.N), S3), 256) : align_up(gemm3_tail_slab_bytes(tiles - tail_from, TS), 256));
      if (!copy || ws_bytes >= used + copy) return TileChoice{3, S3, used, tail_from, TS, native};
    }
  }
  return TileChoice{2, gemm2_split_for(p.M, p.N, p.K, ws_bytes), 0, 0, 0, 0};
}

static bool native_prefill_ok(const qllm_weight_t *w, GemmParams &p) {
  if (!ptrs_aligned(*w)) return false;
  if (panel_serves(w, p.M)) return true;
  if (w->bits == 3) return gemm3_ok(p, kGemm3Rows3Bit);
  if (w->bits != 4) return false;
  if (gemm2_ok(p, QLLM_LAYOUT_GPTQ)) return true;
  // round 7: N % 128 == 64 (Falcon-7B's 4544 / 4672) -- gemm3's half-wide last tile, whatever the activation type (choose_tile decides
  // how gemm3 takes bf16)
  GemmParams q = p;
  q.act_bf16 = 0;
  return gemm3_n_tail(q, QLLM_LAYOUT_GPTQ) && gemm3_ok(q, QLLM_LAYOUT_GPTQ);
}

// ---- the decision ------------------------------------------------------------------------------------------------------------------------
static Decision routed(Route r, int layout = 0) {
  Decision d;
  memset(&d, 0, sizeof(d));
  d.route = r;
  d.layout = layout;
  return d;
}
static Decision refused(int rc) {
  Decision d = routed(ROUTE_NONE);
  d.rc = rc;
  return d;
}

Decision decide_single(const qllm_weight_t *w, int M, int act_dtype) {
  Decision d = routed(ROUTE_STRIP);
  GemmParams p;
  fill_gemm_params(p, w, nullptr, nullptr, M, act_dtype);
  if ((w->bits == 3 || is_native(*w)) && strip_plan(w, 1, M, &d.strip)) return d;
  if (is_native(*w)) {
    // prefill-sized calls (M > 64, and what the strips leave alone) on native-layout layers: the panel kernel, or the tile GEMMs with
    // their staging waves reading the strip-major words
    if (!native_prefill_ok(w, p))
      return refused(set_error(QLLM_ERR_UNSUPPORTED, "native-layout layer: no fused kernel for M=%d K=%d N=%d g=%d bits=%d (decode sizes, and M > 64 with "
                               "K %% 64 == 0, N %% 128 == 0 and a power-of-two group size, are served)", M, w->K, w->N, w->group_size, w->bits));
    if (panel_serves(w, M)) return routed(ROUTE_PANEL);
    if (w->bits == 3) return routed(ROUTE_ROWS3, kGemm3Rows3Bit);
    return routed(ROUTE_TILE, QLLM_LAYOUT_GPTQ);
  }
  if (skinny_ok(*w, M)) {
    if (strip_plan(w, 1, M, &d.strip)) return d;
    // 33..64 rows the strips leave alone (wide shapes): the 256-row-tile GEMM beats split-K here
    if (M > 32 && gemm_ok(*w) && gemm2_ok(p, w->layout)) return routed(ROUTE_TILE, w->layout);
    return routed(ROUTE_SKINNY);
  }
  if (w->bits == 3 && M > 64 && w->layout != QLLM_LAYOUT_AWQ_GEMM && !w->g_idx && ptrs_aligned(*w) && gemm3_ok(p, kGemm3Rows3Bit))
    return routed(ROUTE_ROWS3, kGemm3Rows3Bit);  // 3-bit row-stream layers at prefill sizes: gemm3 with 3-bit staging waves (LAYOUT 2)
  if (gemm_ok(*w)) return routed(gemm2_ok(p, w->layout) ? ROUTE_TILE : ROUTE_GEMM, w->layout);
  // 2 / 5 / 6 / 7 / 8 bits (and 3 / 4-bit layers nothing above takes) at decode sizes: the bit-stream matvec (bitgemv.hip, round 6)
  if (knob("QLLM_BITGEMV", 1) && bitgemv_ok(*w, M)) return routed(ROUTE_BITGEMV);
  return refused(set_error(QLLM_ERR_UNSUPPORTED, "no fused kernel for bits=%d K=%d N=%d g=%d layout=%d act_order=%d; use qllm_dequant + GEMM",
                           w->bits, w->K, w->N, w->group_size, w->layout, w->g_idx != nullptr));
}

// prefill-sized groups (round 6): q/k/v, gate/up as ONE launch of the 256x128 kernel -- its grid carries the tiles of up to 4 layers, so
// the rounds of CUs are counted over the group (Llama-2-7B gate/up: 1376 tiles = 5.4 rounds, with the last one K-split, instead of
// 2 x 2.7 -> 2 x 3) and the group costs one launch boundary.  4-bit row-stream / strip-major layers of one storage kind, whole tiles,
// at least one tile per CU (no split-K inside a group); bf16 only where the kernel takes it natively.
static bool tile_group_serves(const qllm_weight_t *w, int n, int M, int act_dtype) {
  if (!knob("QLLM_GEMM3_GROUP", 1) || !knob("QLLM_GEMM3", 1) || n < 2 || n > kGemm3MaxProb || M < 384) return false;
  const int gs = w[0].group_size;
  if (w[0].bits != 4 || w[0].K % 64 != 0 || gs < 32 || (gs & (gs - 1)) != 0) return false;
  if (act_dtype == QLLM_BF16 && !gemm3_bf16_native(QLLM_LAYOUT_GPTQ)) return false;
  for (int i = 0; i < n; ++i) {
    if (w[i].layout == QLLM_LAYOUT_AWQ_GEMM || w[i].g_idx || w[i].N % 128 != 0 || is_native(w[i]) != is_native(w[0])) return false;
    if (!ptrs_aligned(w[i])) return false;
    if ((size_t)M * w[i].K * 2 >= 0x7fffffffull || (size_t)w[i].K * w[i].N / 2 >= 0x7fffffffull) return false;
  }
  return group_tiles(w, n, M) >= compute_units();
}

// INVALID when the layers cannot share a launch at all, UNSUPPORTED when no grouped kernel takes them
Decision decide_group(const qllm_weight_t *w, int n, int M, int act_dtype) {
  for (int i = 0; i < n; ++i) {
    if (w[i].K != w[0].K || w[i].group_size != w[0].group_size || w[i].bits != w[0].bits || layout_family(w[0]) != layout_family(w[i]) ||
        w[i].add_zero_bias != w[0].add_zero_bias)
      return refused(set_error(QLLM_ERR_INVALID, "grouped weights must agree on K, group_size, bits, layout family and add_zero_bias"));
  }
  if (tile_group_serves(w, n, M, act_dtype)) return routed(ROUTE_TILE_GROUP, QLLM_LAYOUT_GPTQ);  // (prefill sizes: M >= 384)
  for (int i = 0; i < n; ++i) {
    if (w[i].bits == 3 || is_native(w[i])) continue;  // decided as a group by strip_plan below
    if (!skinny_ok(w[i], M))
      return refused(set_error(QLLM_ERR_UNSUPPORTED, "grouped forward needs the decode kernel (4-bit, M<=%d, K%%32==0, no act-order)", skinny_max_m()));
  }
  Decision d = routed(ROUTE_STRIP);
  if (strip_plan(w, n, M, &d.strip)) return d;
  if (panel_group_serves(w, n, M)) return routed(ROUTE_PANEL);
  if (is_native(w[0]))
    return refused(set_error(QLLM_ERR_UNSUPPORTED, "grouped forward: native-layout layers are served for M <= 32 (4 bits: <= 128) with group size 64 / 128 (4 bits: also 32), and 4-bit groups of at least one 256x128 tile per CU from 384 rows (M=%d g=%d)", M, w[0].group_size));
  if (w[0].bits != 4) return refused(set_error(QLLM_ERR_UNSUPPORTED, "grouped forward: no fused kernel for %d-bit weights in this shape", w[0].bits));
  return routed(ROUTE_SKINNY);
}

// The fused SwiGLU down-projection (strip1_swiglu.hip): exactly the calls the plain entry runs on the batch-1 kernel, with the same
// waves x round, so that the fused launch is the plain launch's arithmetic on act(gate) * up.  Everything else keeps today's path
// (the elementwise kernel, then qllm_linear_forward).
int decide_swiglu(const qllm_weight_t *w, int M, int act, StripPlan *plan) {
  *plan = StripPlan{};
  if (act != QLLM_ACT_SILU) return set_error(QLLM_ERR_UNSUPPORTED, "fused SwiGLU: act=%d is not served (QLLM_ACT_SILU only)", act);
  if (!is_native(*w) || !strip_plan(w, 1, M, plan) || !plan->one_nw)
    return set_error(QLLM_ERR_UNSUPPORTED, "fused SwiGLU: calls of the batch-1 kernel on native-layout layers only -- M=1: 4 bits with 128- / 64-wide groups and 3 bits, "
                     "M=2..4: 4 bits with 128-wide groups and K <= 16384 (M=%d bits=%d g=%d K=%d layout=%d); run the activation and qllm_linear_forward",
                     M, w->bits, w->group_size, w->K, w->layout);
  return QLLM_OK;
}

// The fused residual add behind o_proj / down_proj (strip1_resid.hip, strip1_swiglu_resid.hip): one row, and there exactly what
// decide_swiglu serves -- the calls the plain entry runs on the batch-1 kernel for native-layout layers -- with the same waves x round.
// Everything else keeps today's path (the launch, then the elementwise add).
int decide_residual(const qllm_weight_t *w, int M, StripPlan *plan) {
  static const char kInstead[] = "run the launch and add the residual";
  *plan = StripPlan{};
  if (M != 1) return set_error(QLLM_ERR_UNSUPPORTED, "fused residual: one row only (M=%d; the four-row forms are not built); %s", M, kInstead);
  if (decide_swiglu(w, 1, QLLM_ACT_SILU, plan))
    return set_error(QLLM_ERR_UNSUPPORTED, "fused residual: calls of the batch-1 kernel on native-layout layers only -- 4 bits with 128- / 64-wide groups and 3 bits, "
                     "K within its shape table, QLLM_STRIP1 on (bits=%d g=%d K=%d layout=%d); %s", w->bits, w->group_size, w->K, w->layout, kInstead);
  return QLLM_OK;
}

// The fused RMSNorm in front of a sibling group (strip1_norm.hip): exactly the M = 1 calls decide_single / decide_group put on the batch-1
// kernel for native-layout layers, with the same waves x round, so that the fused launch is the plain grouped launch's arithmetic on
// RMSNorm(x).  Everything else keeps qllm_rmsnorm and today's launch.
int decide_rmsnorm(const qllm_weight_t *w, int n, int M, Decision *d) {
  static const char kInstead[] = "run qllm_rmsnorm and qllm_linear_forward_grouped";
  *d = refused(QLLM_ERR_UNSUPPORTED);
  if (M != 1) return set_error(QLLM_ERR_UNSUPPORTED, "fused RMSNorm: one row only (M=%d; the four-row forms are not built); %s", M, kInstead);
  for (int i = 0; i < n; ++i) {
    if (!is_native(w[i]))
      return set_error(QLLM_ERR_UNSUPPORTED, "fused RMSNorm: native-layout layers only (member %d: layout=%d bits=%d); %s", i, w[i].layout, w[i].bits, kInstead);
    if (w[i].K != w[0].K || w[i].group_size != w[0].group_size || w[i].bits != w[0].bits || w[i].add_zero_bias != w[0].add_zero_bias)
      return set_error(QLLM_ERR_UNSUPPORTED, "fused RMSNorm: the members must agree on K, group_size, bits and add_zero_bias (member %d: K=%d g=%d bits=%d against K=%d g=%d bits=%d); %s",
                       i, w[i].K, w[i].group_size, w[i].bits, w[0].K, w[0].group_size, w[0].bits, kInstead);
  }
  const Decision plain = n == 1 ? decide_single(w, 1, QLLM_F16) : decide_group(w, n, 1, QLLM_F16);
  if (plain.route != ROUTE_STRIP || !plain.strip.one_nw)
    return set_error(QLLM_ERR_UNSUPPORTED, "fused RMSNorm: calls of the batch-1 kernel only -- 4 bits with 128- / 64-wide groups and 3 bits, K within its shape table, "
                     "QLLM_STRIP1 on (bits=%d g=%d K=%d layout=%d, %d layers); %s", w[0].bits, w[0].group_size, w[0].K, w[0].layout, n, kInstead);
  *d = plain;
  clear_error();
  return QLLM_OK;
}

void describe(const Decision &d, const qllm_weight_t *w, int n, int M, size_t ws_bytes, char *buf, size_t buflen) {
  const char *sm = is_native(w[0]) ? " layout=strip-major" : "";
  switch (d.route) {
    case ROUTE_STRIP: {
      const StripPlan &pl = d.strip;
      if (pl.one_nw)
        snprintf(buf, buflen, "strip1 nw=%d round=%d%s%s%s grid=strips x %d layout=strip-major", pl.one_nw, pl.one_maxs,
                 pl.one_nw * pl.one_maxs == w[0].K / 32 ? " exact" : "", w[0].group_size == 64 ? (w[0].bits == 3 ? " g64 bits=3" : " g64") : (w[0].bits == 3 ? " bits=3" : ""),
                 M > 1 ? " rows=4" : "", n);
      else
        snprintf(buf, buflen, "strip nw=%d cpl=%d spw=%d form=%s row_tiles=%d%s", pl.nw, pl.cpl, pl.spw,
                 pl.ra == 2 ? "dma-A" : (pl.ra ? "register-A" : "lds-slab"), M > 32 ? 4 : (M > 16 ? 2 : 1), pl.sm ? " layout=strip-major" : "");
      return;
    }
    case ROUTE_PANEL: {
      char layers[24] = "";
      if (n > 1) snprintf(layers, sizeof(layers), " layers=%d", n);
      snprintf(buf, buflen, "panel cols=64 row_tiles=%d k_halves=%d split_k=%d%s%s layout=strip-major", panel_mt(M), panel_kh(M),
               panel_split_for(M, panels_of(w, n), w[0].K, ws_bytes), layers, w[0].bits == 3 ? " bits=3" : "");
      return;
    }
    case ROUTE_ROWS3: {
      const int S = gemm3_split_for(M, w[0].N, w[0].K, ws_bytes);
      if (S > 1) snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4 bits=3 split_k=%d%s", S, sm);
      else snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4 bits=3%s", sm);
      return;
    }
    case ROUTE_TILE: {
      GemmParams p;
      fill_gemm_params(p, &w[0], nullptr, nullptr, M, QLLM_F16);
      const TileChoice c = choose_tile(p, d.layout, ws_bytes);
      const char *nt = w[0].N % 128 ? " n_tail=64" : "";  // (round 7: the half-wide last column tile)
      if (c.kernel == 3 && c.tail_split > 1) snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4 tail_split=%d%s%s", c.tail_split, nt, sm);
      else if (c.kernel == 3 && c.split_k > 1) snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4 split_k=%d%s%s", c.split_k, nt, sm);
      else if (c.kernel == 3) snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4%s%s", nt, sm);
      else snprintf(buf, buflen, "gemm2 tile=256x%d split_k=%d%s", gemm2_tile_n(M, w[0].N, c.split_k), c.split_k, sm);
      return;
    }
    case ROUTE_TILE_GROUP: {
      int tail_from = 0;
      const int TS = tile_group_tail_for(w, n, M, ws_bytes, &tail_from);
      if (TS > 1) snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4 layers=%d tail_split=%d%s", n, TS, sm);
      else snprintf(buf, buflen, "gemm3 tile=256x128 matrix-waves=8 staging-waves=4 layers=%d%s", n, sm);
      return;
    }
    case ROUTE_GEMM: snprintf(buf, buflen, "gemm tile=128x128%s", w[0].g_idx ? " act-order-gather" : ""); return;
    case ROUTE_SKINNY: {
      const SkinnyPlan s = plan_skinny(w, n, M);
      snprintf(buf, buflen, "skinny tile_cols=%d split_k=%d spw=%d", s.tile_cols, s.S, s.spw);
      return;
    }
    case ROUTE_BITGEMV:
      snprintf(buf, buflen, "bitgemv bits=%d cols=%d waves=8 split_k=%d", w[0].bits, bitgemv_cols(), bitgemv_split_for(M, w[0].K, w[0].N, ws_bytes));
      return;
    default: snprintf(buf, buflen, "unsupported (%s)", last_error_text()[0] ? last_error_text() : "dequant + GEMM");
  }
}

size_t workspace_bytes_act(const qllm_weight_t *w, int M, int act_dtype) {
  if (!w || M <= 0) return kCounterBytes;
  size_t tiles = 0;
  if (M > 32) {  // the 256-row-tile GEMMs (every M > 64, and 33..64 rows of the shapes the strips leave alone): fp32 partial
    GemmParams p;  // tiles of the split-K forms + the fp16 copy of bf16 activations where the wave-specialised kernel would
    fill_gemm_params(p, w, nullptr, nullptr, M, QLLM_F16);  // serve a bf16 call
    p.g_idx = nullptr;
    const bool g3 = gemm3_ok(p, w->bits == 3 ? kGemm3Rows3Bit : (w->layout == QLLM_LAYOUT_AWQ_GEMM ? QLLM_LAYOUT_AWQ_GEMM : QLLM_LAYOUT_GPTQ));
    int tail_from = 0;
    const int TS = g3 && w->bits != 3 ? gemm3_tail_split(M, w->N, w->K, &tail_from) : 1;  // (the ragged last round's K-split, gemm3.hip)
    const size_t tail = align_up(gemm3_tail_slab_bytes(tiles_256x128(M, gemm3_tile_cols(w->N)) - tail_from, TS), 256);
    // (round 7: gemm3's own split-K -- the only one a layer with a half-wide last tile has; never more than gemm2's elsewhere)
    const size_t split3 = g3 ? align_up(gemm2_slab_bytes(M, gemm3_tile_cols(w->N), gemm3_split_k(M, w->N, w->K)), 256) : 0;
    tiles = std::max(std::max(align_up(gemm2_slab_bytes(M, w->N, gemm2_split_k(M, w->N, w->K)), 256), split3), tail) +
            (g3 ? bf16_copy_bytes(M, w->K, act_dtype == QLLM_BF16) : 0);
    if (M > 128) return kCounterBytes + tiles;
  }
  // the panel kernel's partial panels (single native 4-bit layers, 9..128 rows)
  if (M >= 9 && M <= 128 && w->N % 64 == 0) tiles = std::max(tiles, align_up(panel_slab_bytes(M, w->N / 64, panel_split_k(M, w->N / 64, w->K)), 256));
  if (M > 64) return kCounterBytes + tiles;
  const size_t slabs = align_up((size_t)skinny_max_split(M) * M * w->N * sizeof(float), 256);
  return kCounterBytes + (tiles > slabs ? tiles : slabs);
}

}  // namespace qllm
