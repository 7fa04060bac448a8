// C-ABI entry points of libqllm_mi355x.so: argument validation (the reference's TORCH_CHECK / invalid_argument
// sites: /root/reference/csrc/ort_cuda/ort_ops.cc:64-73,99-107; csrc/awq_cuda/quantization/gemm_cuda_gen.cu:1128-1135),
// parameter-block fills, workspace carving, launches.  Which kernel runs is decided in planner.hip.  No allocation, no host sync, no
// global mutable state beyond thread-local error text.
// The kernels with an entry of their own (qllm_linear_forward_permuted / _bitpanel / _bitgemm / _bitgroup / _swiglu / _rmsnorm / _residual: the planner
// does not know them) each keep ONE *_check / decide_* that their forward, *_workspace_bytes and *_describe entries all ask.  What those
// entries do around it is written once: check_layer_count + check_layers (an array of layers), check_describe_args, describe_refusal
// (a refusal as text), counters_and_slabs (a workspace size) and fill_bit_params (the bit family's parameter blocks).
// The six launches of the batch-1 kernel (launch_strip1 / _allreduce / _swiglu / _norm / _resid / _swiglu_resid) fill one Strip1Params
// here and share ONE form table and launch site, strip1_forms.hpp: a further fused family is the struct that header describes plus its
// entry here -- no pair table and no launch of its own.
// The attention entries (qllm_attn_decode / _prefill and their _window forms) share check_attn_shape / _served / _call / _layout:
// a rule both kernels have is one text there, and an entry's body holds the calls and the few rules that are its own.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>

#include "planner.hpp"

namespace qllm {

// ---- error plumbing ----------------------------------------------------------------------------------------
static thread_local char g_err[512] = {0};

int set_error(int code, const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}
void clear_error() { g_err[0] = 0; }
const char *last_error_text() { return g_err; }

// ---- validation ----------------------------------------------------------------------------------------------
// shapes the strip-major native layout can hold (include/qllm_mi355x.h)
static int native_shape_ok(int bits, int K, int N, int group_size, bool packed_zeros) {
  if (bits != 4 && bits != 3) return set_error(QLLM_ERR_UNSUPPORTED, "the native layout holds 3- and 4-bit weights (got %d)", bits);
  if (K % 32 != 0 || N % 16 != 0) return set_error(QLLM_ERR_UNSUPPORTED, "the native layout needs K %% 32 == 0 and N %% 16 == 0 (K=%d N=%d)", K, N);
  if (group_size % 32 != 0) return set_error(QLLM_ERR_UNSUPPORTED, "the native layout needs group_size %% 32 == 0 (got %d)", group_size);
  if (bits == 3 && packed_zeros && N % 32 != 0) return set_error(QLLM_ERR_UNSUPPORTED, "3-bit packed zero points need N %% 32 == 0 (N=%d)", N);
  return QLLM_OK;
}

static int validate_weight(const qllm_weight_t *w) {
  if (!w) return set_error(QLLM_ERR_INVALID, "weight descriptor is NULL");
  if (!w->qweight || !w->scales) return set_error(QLLM_ERR_INVALID, "qweight/scales must not be NULL");
  if (w->layout < QLLM_LAYOUT_GPTQ || w->layout > QLLM_LAYOUT_NATIVE_F16Z) return set_error(QLLM_ERR_INVALID, "unknown layout %d", w->layout);
  if (w->bits < 2 || w->bits > 8) return set_error(QLLM_ERR_INVALID, "bits must be >= 2 and <= 8 (got %d)", w->bits);
  if (w->K <= 0 || w->N <= 0) return set_error(QLLM_ERR_INVALID, "in_features/out_features must be >= 1 (K=%d N=%d)", w->K, w->N);
  if (w->group_size < 8) return set_error(QLLM_ERR_INVALID, "groupsize must be >= 8 (got %d)", w->group_size);
  if (w->layout == QLLM_LAYOUT_AWQ_GEMM) {
    if (w->bits != 4) return set_error(QLLM_ERR_INVALID, "AWQ GEMM layout is 4-bit only (got %d)", w->bits);
    if (w->N % 8 != 0) return set_error(QLLM_ERR_INVALID, "OC is not multiple of pack_num = 8 (N=%d)", w->N);
    if (w->K % w->group_size != 0) return set_error(QLLM_ERR_INVALID, "IC is not multiple of group size (K=%d g=%d)", w->K, w->group_size);
    if (!w->qzeros) return set_error(QLLM_ERR_INVALID, "AWQ GEMM layout needs qzeros");
    if (w->g_idx) return set_error(QLLM_ERR_INVALID, "AWQ GEMM layout has no act-order (g_idx must be NULL)");
  } else if (is_native(*w)) {
    if (int rc = native_shape_ok(w->bits, w->K, w->N, w->group_size, w->layout == QLLM_LAYOUT_NATIVE && w->qzeros)) return rc;
    if (w->K % w->group_size != 0) return set_error(QLLM_ERR_INVALID, "the native layout holds whole groups (K=%d g=%d)", w->K, w->group_size);
    if (w->g_idx) return set_error(QLLM_ERR_INVALID, "the native layout has no act-order (g_idx must be NULL: sort the rows by group first)");
    if (w->layout == QLLM_LAYOUT_NATIVE_F16Z && !w->qzeros) return set_error(QLLM_ERR_INVALID, "NATIVE_F16Z layout needs fp16 qzeros");
  } else {
    if ((w->K * w->bits) % 32 != 0) return set_error(QLLM_ERR_INVALID, "in_features*bits must be a multiple of 32 (K=%d bits=%d)", w->K, w->bits);
    if (w->layout == QLLM_LAYOUT_HQQ && !w->qzeros) return set_error(QLLM_ERR_INVALID, "HQQ layout needs fp16 qzeros");
    if (w->layout == QLLM_LAYOUT_HQQ && w->g_idx) return set_error(QLLM_ERR_INVALID, "HQQ layout has no act-order (g_idx must be NULL)");
    if (w->layout == QLLM_LAYOUT_GPTQ && w->qzeros && (w->N * w->bits) % 32 != 0)
      return set_error(QLLM_ERR_INVALID, "out_features*bits must be a multiple of 32 for packed zeros (N=%d bits=%d)", w->N, w->bits);
  }
  if (w->add_zero_bias < 0 || w->add_zero_bias > 1) return set_error(QLLM_ERR_INVALID, "add_zero_bias must be 0 or 1");
  return QLLM_OK;
}

static int check_io(const void *x, const void *y, int M, int act_dtype) {
  if (!x || !y) return set_error(QLLM_ERR_INVALID, "x / y must not be NULL");
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  if (act_dtype != QLLM_F16 && act_dtype != QLLM_BF16) return set_error(QLLM_ERR_INVALID, "act_dtype must be f16 or bf16");
  if ((uintptr_t)x % 16 != 0) return set_error(QLLM_ERR_INVALID, "x must be 16-byte aligned");
  return QLLM_OK;
}

// What every entry that takes an ARRAY of layers checks: the arrays (each entry words its own NULL check: a describe entry names its
// buffer with them), the count against the entry's limit (`entry`: "", or the name its message starts with), then layer by layer the
// descriptor and -- with `each` -- what the entry asks of that layer (its output through check_io, ...).  Two functions because entries
// have checks of their own between the count and the layers, and the order in which checks fire is part of the ABI.
static const char kArraysNull[] = "w / y arrays must not be NULL";
static int check_layer_count(int n, int limit, const char *entry = "") {
  if (n < 1 || n > limit) return set_error(QLLM_ERR_INVALID, "%sn_weights must be 1..%d (got %d)", entry, limit, n);
  return QLLM_OK;
}
template <typename Each>
static int check_layers(const qllm_weight_t *w, int n, Each each) {
  for (int i = 0; i < n; ++i) {
    if (int rc = validate_weight(&w[i])) return rc;
    if (int rc = each(i)) return rc;
  }
  return QLLM_OK;
}
static int check_layers(const qllm_weight_t *w, int n) { return check_layers(w, n, [](int) { return (int)QLLM_OK; }); }

// what qllm_bitpanel_describe and qllm_bitgemm_describe check before the entry's own *_check
static int check_describe_args(const qllm_weight_t *w, int M, const char *buf, size_t buflen) {
  if (!buf || buflen == 0) return set_error(QLLM_ERR_INVALID, "buf must not be NULL");
  if (int rc = validate_weight(w)) return rc;
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  return QLLM_OK;
}

// The tail of a describe entry whose check said no (rc != QLLM_OK).  A call the kernel does not take is an answer, not a failure:
// QLLM_ERR_UNSUPPORTED becomes text in buf through `fmt` (kUnsupported, kRefused) with the error's own words, the error is cleared and
// the entry returns QLLM_OK.  Every other status is returned as it is, its text in qllm_last_error().
static const char kUnsupported[] = "unsupported (%s)", kRefused[] = "refused: %s";
static int describe_refusal(int rc, const char *fmt, char *buf, size_t buflen) {
  if (rc != QLLM_ERR_UNSUPPORTED) return rc;
  snprintf(buf, buflen, fmt, last_error_text());
  clear_error();
  return QLLM_OK;
}

// What the *_workspace_bytes of the bit family answer: the counter page, and behind it the slabs of the geometry the entry would launch
// with a workspace of any size (`geometry`: that call, with SIZE_MAX).  A call the entry refuses needs the page alone, and leaves no error.
template <typename Geometry>
static size_t counters_and_slabs(bool refused, Geometry geometry) {
  if (refused) {
    clear_error();
    return kCounterBytes;
  }
  return kCounterBytes + geometry().slab_bytes;
}

// What the four quantizer entry points check first, alike: the pointers they require (`required` names them, w_nk among them), the
// weight's type and N / K / group_size.  Each entry's own checks follow in the order they have always fired.
static int check_quant_layer(const char *required, bool missing, int32_t w_dtype, int32_t N, int32_t K, int32_t group_size) {
  if (missing) return set_error(QLLM_ERR_INVALID, "%s must not be NULL", required);
  if (w_dtype != QLLM_F16 && w_dtype != QLLM_BF16 && w_dtype != QLLM_F32) return set_error(QLLM_ERR_INVALID, "w_dtype must be QLLM_F16, QLLM_BF16 or QLLM_F32");
  if (N <= 0 || K <= 0 || group_size <= 0) return set_error(QLLM_ERR_INVALID, "bad N/K/group_size (%d/%d/%d)", N, K, group_size);
  return QLLM_OK;
}
static int check_whole_groups(int32_t K, int32_t group_size) {
  if (K % group_size != 0) return set_error(QLLM_ERR_INVALID, "K must be a multiple of group_size (K=%d group_size=%d)", K, group_size);
  return QLLM_OK;
}
static int elem_size(int32_t w_dtype) { return w_dtype == QLLM_F32 ? 4 : 2; }
static const char *const kElemAligned = "every buffer must be aligned to its element size";

static int check_workspace(const char *entry, const void *workspace, size_t workspace_bytes, size_t need) {
  if ((need && !workspace) || workspace_bytes < need || (uintptr_t)workspace % 16)
    return set_error(QLLM_ERR_WORKSPACE, "%s needs a 16-byte aligned workspace of %zu bytes (got %zu)", entry, need, workspace ? workspace_bytes : (size_t)0);
  return QLLM_OK;
}

// ---- parameter-block fills shared by the run_* functions ------------------------------------------------------------------------------
// diagnostics: timeline buffer handed to the native-layout decode launches (24 x u64 per launch), see qllm_debug_timeline()
static uint64_t *g_timeline = nullptr;
static int g_timeline_slots = 0, g_timeline_next = 0;

// the workspace a split may use: non-NULL and 256-byte aligned, else none; its head holds the arrival counters, the partial results follow
static size_t usable_ws(const void *workspace, size_t workspace_bytes) {
  return (workspace && (uintptr_t)workspace % 256 == 0) ? workspace_bytes : 0;
}
static void carve(void *workspace, int **counters, float **slabs) {
  *counters = (int *)workspace;
  *slabs = (float *)((char *)workspace + kCounterBytes);
}
static void set_split(GemmParams &p, int S, void *workspace, int tail_from = 0, int tail_split = 0) {
  p.split_k = S;
  p.tail_from = tail_split > 1 ? tail_from : 0;
  p.tail_split = tail_split > 1 ? tail_split : 0;
  p.counters = nullptr;
  p.slabs = nullptr;
  if (S > 1 || tail_split > 1) carve(workspace, &p.counters, &p.slabs);
}
static void fill_launch_params(GemmParams &p, const qllm_weight_t *w, const void *x, void *y, int M, int act_dtype) {
  fill_gemm_params(p, w, x, y, M, act_dtype);
#ifdef QLLM_LAB
  p.dbg = g_timeline;  // (lab: qllm_debug_timeline(buf, n) before a prefill call hands gemm4 its per-block stamp buffer)
#endif
}

// ---- one run_* per route --------------------------------------------------------------------------------------------------------------
// the batch-1 kernel's block (run_strip1, and qllm_linear_forward_allreduce with one layer); returns the widest layer's strips
static int fill_strip1_params(Strip1Params &p, const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype) {
  fill_call(p, w[0], x, M, act_dtype);
  p.T = w[0].K / 32;
  p.n_groups = w[0].K / w[0].group_size;
  p.group64 = w[0].group_size == 64;
  p.bits3 = w[0].bits == 3;
  int max_strips = 0;
  for (int i = 0; i < n; ++i) {
    fill_layer(p.prob[i], w[i], y[i]);
    p.prob[i].n_strips = w[i].N / 16;
    // the kernel issues its zero-point load whatever the kind (one address form, no select): a symmetric layer reads a scale word
    if (p.prob[i].zero_kind == ZK_SYM) p.prob[i].qzeros = w[i].scales;
    max_strips = std::max(max_strips, p.prob[i].n_strips);
  }
  return max_strips;
}
static int run_strip1(const StripPlan &pl, const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype, hipStream_t stream) {
  Strip1Params p;
  const int max_strips = fill_strip1_params(p, w, y, n, x, M, act_dtype);
  p.dbg = (g_timeline && g_timeline_next < g_timeline_slots) ? g_timeline + 24 * (g_timeline_next++) : nullptr;
  return launch_strip1(p, pl.one_nw, pl.one_maxs, n, max_strips, stream);
}

static int run_strip(const StripPlan &pl, const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype, hipStream_t stream) {
  if (pl.one_nw) return run_strip1(pl, w, y, n, x, M, act_dtype, stream);
  StripParams p;
  fill_call(p, w[0], x, M, act_dtype);
  p.n_prob = n;
  p.K = w[0].K;
  p.T = w[0].K / 32;
  p.cpl = pl.cpl;
  p.bits = w[0].bits;
  p.nw = pl.nw;
  p.spw = pl.spw;
  p.ra = pl.ra;
  p.sm = pl.sm;
  p.n_groups = (w[0].K + w[0].group_size - 1) / w[0].group_size;
  p.group_size = w[0].group_size;
  // diagnostics: only the lds-slab 4-bit g128 native-layout form has a timeline instantiation
  p.dbg = (pl.sm && (!pl.ra || pl.ra == 2) && p.bits == 4 && p.group_size == 128 && g_timeline && g_timeline_next < g_timeline_slots)
              ? g_timeline + 24 * (g_timeline_next++) : nullptr;
  int block = 0;
  for (int i = 0; i < n; ++i) {
    StripProblem &q = p.prob[i];
    fill_layer(q, w[i], y[i]);
    q.N = w[i].N;
    q.n_strips = (w[i].N / 16 + pl.cpl - 1) / pl.cpl;  // (strip_dma.hpp: the last block may be ragged; every other form divides)
    q.block_begin = block;
    p.block_begin8[i] = block;
    block += q.n_strips;
  }
  return launch_strip(p, block, stream);
}

static int run_skinny(const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype, void *workspace,
                      size_t workspace_bytes, hipStream_t stream) {
  const SkinnyPlan s = plan_skinny(w, n, M);
  if (s.tiles_total > (int)(kCounterBytes / sizeof(int))) return set_error(QLLM_ERR_UNSUPPORTED, "too many column tiles (%d)", s.tiles_total);

  SkinnyParams p;
  fill_call(p, w[0], x, M, act_dtype);
  p.n_prob = n;
  p.K = w[0].K;
  p.T = w[0].K / 32;
  p.group_size = w[0].group_size;
  size_t slab_off = kCounterBytes;
  int tile_off = 0, block = 0;
  for (int i = 0; i < n; ++i) {
    SkinnyProblem &q = p.prob[i];
    fill_layer(q, w[i], y[i]);
    q.N = w[i].N;
    q.n_tiles = (w[i].N + s.tile_cols - 1) / s.tile_cols;
    q.S = s.S;
    q.spw = s.spw;
    q.block_begin = block;
    q.counters = (int *)workspace + tile_off;
    q.slabs = (float *)((char *)workspace + slab_off);
    tile_off += q.n_tiles;
    block += q.n_tiles * s.S;
    if (s.S > 1) slab_off += align_up((size_t)s.S * M * w[i].N * sizeof(float), 256);
  }
  if (s.S > 1) {
    if (!workspace) return set_error(QLLM_ERR_WORKSPACE, "split-K needs a workspace (call qllm_workspace_bytes)");
    if (workspace_bytes < slab_off) return set_error(QLLM_ERR_WORKSPACE, "workspace too small: need %zu bytes, have %zu", slab_off, workspace_bytes);
    if ((uintptr_t)workspace % 256 != 0) return set_error(QLLM_ERR_INVALID, "workspace must be 256-byte aligned");
  }
  return launch_skinny(p, w[0].layout, s.awq_w, block, stream);
}

// ROUTE_TILE: gemm3 or gemm2 as choose_tile says.  `bf16_out_only` (QLLM_F16_IN_BF16_OUT): x is fp16 already and y is bf16, which only
// gemm3 writes
static const char kNotPrefillKernel[] = "QLLM_F16_IN_BF16_OUT: M=%d K=%d N=%d is not served by the 256x128 prefill kernel";
static int run_tile_gemm(GemmParams &p, int layout, void *workspace, size_t workspace_bytes, hipStream_t stream, bool bf16_out_only = false) {
  const TileChoice c = choose_tile(p, layout, usable_ws(workspace, workspace_bytes));
  if (bf16_out_only && c.kernel != 3) return set_error(QLLM_ERR_UNSUPPORTED, kNotPrefillKernel, p.M, p.K, p.N);
  set_split(p, c.split_k, workspace, c.tail_from, c.tail_split);
  if (c.kernel == 2 && p.N % 128 != 0)  // (half-wide last tile: gemm2 has no such form; bf16 with QLLM_GEMM3_BF16=0 needs the fp16 copy)
    return set_error(QLLM_ERR_WORKSPACE, "N %% 128 == 64 with bf16 activations converted to fp16: the workspace must hold the copy (call qllm_workspace_bytes_act)");
  if (c.kernel == 2) return launch_gemm2(p, layout, stream);
  if (bf16_out_only) p.out_bf16 = 1;
  if (c.native_bf16) {
    p.native_bf16 = 1;
    p.act_bf16 = 0;  // (gemm3's own flag means "x was converted": not here)
  } else if (p.act_bf16) {
    void *xh = (char *)workspace + c.copy_off;
    if (int rc = launch_bf16_to_f16(p.x, xh, (size_t)p.M * p.K, stream)) return rc;
    p.x = xh;
    p.act_bf16 = 0;
    p.out_bf16 = 1;
  }
  return launch_gemm3(p, layout, stream);
}

static int run_panel(const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype, void *workspace, size_t workspace_bytes,
                     hipStream_t stream) {
  PanelParams p;
  fill_call(p, w[0], x, M, act_dtype);
  p.K = w[0].K;
  p.group_size = w[0].group_size;
  p.bits = w[0].bits;
  p.n_groups = (w[0].K + w[0].group_size - 1) / w[0].group_size;
  p.n_prob = n;
  p.abl = panel_ablation();
  int begin = 0;
  for (int i = 0; i < n; ++i) {
    PanelProblem &q = p.prob[i];
    fill_layer(q, w[i], y[i]);
    q.N = w[i].N;
    q.panel_begin = begin;
    begin += w[i].N / 64;
  }
  p.n_panels = begin;
  // split-K when the panels alone leave CUs idle and the caller's workspace can hold the partial panels (else: no split)
  p.split_k = panel_split_for(M, begin, p.K, usable_ws(workspace, workspace_bytes));
  if (p.split_k > 1) carve(workspace, &p.counters, &p.slabs);
  return launch_panel(p, stream);
}

// what the bit family's parameter blocks (BitGemvParams, BitPanelParams, BitGemmParams) share: the call, the one layer and its shape
template <typename Params>
static void fill_bit_params(Params &p, const qllm_weight_t *w, const void *x, void *y, int M, int act_dtype) {
  fill_call(p, *w, x, M, act_dtype);
  fill_layer(p, *w, y);
  p.K = w->K;
  p.N = w->N;
  p.group_size = w->group_size;
}

// "<name> " + the plan line of the launch `d`: what qllm_swiglu_describe and qllm_rmsnorm_describe answer where their entries serve
static int describe_fused(const char *name, const Decision &d, const qllm_weight_t *w, int n, int M, char *buf, size_t buflen) {
  const int at = snprintf(buf, buflen, "%s ", name);
  describe(d, w, n, M, 0, buf + at, buflen - at);
  clear_error();
  return QLLM_OK;
}

// perm: NULL, or the permutation the kernel applies to x's columns while it stages them (qllm_linear_forward_permuted)
static int run_bitgemv(const qllm_weight_t *w, void *y, const void *x, int M, int act_dtype, void *workspace, size_t workspace_bytes, hipStream_t stream,
                       const int32_t *perm = nullptr) {
  BitGemvParams p;
  fill_bit_params(p, w, x, y, M, act_dtype);
  p.ksplit = bitgemv_split_for(M, w->K, w->N, usable_ws(workspace, workspace_bytes));
  if (p.ksplit > 1) carve(workspace, &p.counters, &p.slabs);
  return perm ? launch_bitgemv_permuted(p, perm, w->bits, stream) : launch_bitgemv(p, w->bits, stream);
}

static int run_tile_group(const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype, void *workspace, size_t workspace_bytes,
                          hipStream_t stream) {
  GemmParams p;
  fill_launch_params(p, &w[0], x, y[0], M, act_dtype);
  p.n_prob = n;
  int begin = 0;
  for (int i = 0; i < n; ++i) {
    fill_layer(p.prob[i], w[i], y[i]);
    p.prob[i].N = w[i].N;
    p.prob[i].tile_begin = begin;
    begin += tiles_256x128(M, w[i].N);
  }
  p.total_tiles = begin;
  int tail_from = begin;
  const int TS = tile_group_tail_for(w, n, M, usable_ws(workspace, workspace_bytes), &tail_from);
  set_split(p, 1, workspace, tail_from, TS);
  if (act_dtype == QLLM_BF16) {
    p.native_bf16 = 1;
    p.act_bf16 = 0;
  }
  return launch_gemm3(p, QLLM_LAYOUT_GPTQ, stream);
}

// the Decision, executed
static int execute(const Decision &d, const qllm_weight_t *w, void *const *y, int n, const void *x, int M, int act_dtype, void *workspace,
                   size_t workspace_bytes, hipStream_t stream) {
  switch (d.route) {
    case ROUTE_STRIP: return run_strip(d.strip, w, y, n, x, M, act_dtype, stream);
    case ROUTE_PANEL: return run_panel(w, y, n, x, M, act_dtype, workspace, workspace_bytes, stream);
    case ROUTE_SKINNY: return run_skinny(w, y, n, x, M, act_dtype, workspace, workspace_bytes, stream);
    case ROUTE_TILE_GROUP: return run_tile_group(w, y, n, x, M, act_dtype, workspace, workspace_bytes, stream);
    case ROUTE_BITGEMV: return run_bitgemv(w, y[0], x, M, act_dtype, workspace, workspace_bytes, stream);
    case ROUTE_ROWS3: case ROUTE_TILE: case ROUTE_GEMM: {
      GemmParams p;
      fill_launch_params(p, w, x, y[0], M, act_dtype);
      if (d.route == ROUTE_GEMM) return launch_gemm(p, d.layout, stream);
      if (d.route == ROUTE_TILE) return run_tile_gemm(p, d.layout, workspace, workspace_bytes, stream);
      p.g_idx = nullptr;
      set_split(p, gemm3_split_for(p.M, p.N, p.K, usable_ws(workspace, workspace_bytes)), workspace);
      return launch_gemm3(p, kGemm3Rows3Bit, stream);
    }
    default: return d.rc ? d.rc : set_error(QLLM_ERR_INVALID, "internal: empty decision");
  }
}

}  // namespace qllm

using namespace qllm;

extern "C" {

int qllm_abi_version(void) { return QLLM_ABI_VERSION; }

int qllm_is_lab_build(void) {
#ifdef QLLM_LAB
  return 1;
#else
  return 0;
#endif
}

const char *qllm_last_error(void) { return g_err; }

int qllm_set_knob(const char *name, int32_t value) {
  clear_error();
  if (!name) return set_error(QLLM_ERR_INVALID, "qllm_set_knob: name is NULL");
  Settable *k = find_knob(name);
  if (!k) return set_error(QLLM_ERR_INVALID, "qllm_set_knob: %s is not a settable planner threshold (see include/qllm_mi355x.h)", name);
  if (value < k->lo || value > k->hi) return set_error(QLLM_ERR_INVALID, "qllm_set_knob: %s takes %d..%d (got %d)", name, k->lo, k->hi, value);
  k->value = value;
  if (!k->set) {
    k->set = 1;
    __atomic_fetch_add(&g_knob_overrides, 1, __ATOMIC_RELAXED);
  }
  return QLLM_OK;
}

int qllm_get_knob(const char *name, int32_t *value, int32_t *is_set) {
  clear_error();
  if (!name || !value) return set_error(QLLM_ERR_INVALID, "qllm_get_knob: name / value is NULL");
  const Settable *k = find_knob(name);
  if (!k) return set_error(QLLM_ERR_INVALID, "qllm_get_knob: %s is not a settable planner threshold", name);
  *value = k->set ? k->value : 0;
  if (is_set) *is_set = k->set;
  return QLLM_OK;
}

void qllm_reset_knobs(void) { reset_knobs(); }

int qllm_device_info(int device, qllm_device_info_t *out) {
  clear_error();
  if (!out) return set_error(QLLM_ERR_INVALID, "out is NULL");
  memset(out, 0, sizeof(*out));
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) {
    (void)hipGetLastError();
    return set_error(QLLM_ERR_DEVICE, "no HIP device %d (count=%d)", device, count);
  }
  hipDeviceProp_t prop;
  QLLM_HIP_CHECK(hipGetDeviceProperties(&prop, device));
  size_t n = 0;
  while (prop.gcnArchName[n] && prop.gcnArchName[n] != ':' && n + 1 < sizeof(out->arch)) {
    out->arch[n] = prop.gcnArchName[n];
    ++n;
  }
  out->compute_units = prop.multiProcessorCount;
  out->wavefront_size = prop.warpSize;
  out->lds_bytes_per_cu = (int32_t)prop.maxSharedMemoryPerMultiProcessor;
  out->clock_khz = prop.clockRate;
  out->hbm_bytes = (int64_t)prop.totalGlobalMem;
  if (strncmp(out->arch, "gfx950", 6) != 0) return set_error(QLLM_ERR_DEVICE, "device %d is %s, this library is gfx950-only", device, out->arch);
  return QLLM_OK;
}

size_t qllm_workspace_bytes(const qllm_weight_t *w, int32_t M) { return qllm_workspace_bytes_act(w, M, QLLM_BF16); }

size_t qllm_workspace_bytes_act(const qllm_weight_t *w, int32_t M, int32_t act_dtype) { return workspace_bytes_act(w, M, act_dtype); }

int qllm_workspace_init(void *workspace, size_t bytes, void *stream) {
  clear_error();
  if (!workspace || bytes < kCounterBytes) return set_error(QLLM_ERR_WORKSPACE, "workspace must be at least %zu bytes", kCounterBytes);
  QLLM_HIP_CHECK(hipMemsetAsync(workspace, 0, kCounterBytes, (hipStream_t)stream));
  return QLLM_OK;
}

int qllm_linear_forward_grouped(const qllm_weight_t *w, void *const *y, int32_t n_weights, const void *x, int32_t M,
                                int32_t act_dtype, void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  if (!w || !y) return set_error(QLLM_ERR_INVALID, kArraysNull);
  if (int rc = check_layer_count(n_weights, kMaxProblems)) return rc;
  if (n_weights == 1) return qllm_linear_forward(&w[0], x, y[0], M, act_dtype, workspace, workspace_bytes, stream);  // (a group of one is a plain call)
  if (int rc = check_layers(w, n_weights, [&](int i) { return check_io(x, y[i], M, act_dtype); })) return rc;
  const Decision d = decide_group(w, n_weights, M, act_dtype);
  return execute(d, w, y, n_weights, x, M, act_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

// the two shape checks qllm_gather_columns and qllm_gather_describe share (the entry has its pointer checks between them)
static int check_gather_shape(int M, int K) {
  if (M < 0 || K <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 0 and K >= 1 (got M=%d K=%d)", M, K);
  return QLLM_OK;
}
static int check_gather_served(int K) {
  if (!gather_columns_ok(K)) return set_error(QLLM_ERR_UNSUPPORTED, "column gather serves K %% 8 == 0, K <= 28672 (got %d)", K);
  return QLLM_OK;
}

int qllm_gather_columns(const void *x, const int32_t *perm, void *out, int32_t M, int32_t K, int32_t act_dtype, void *stream) {
  clear_error();
  if (!x || !perm || !out) return set_error(QLLM_ERR_INVALID, "x / perm / out must not be NULL");
  if (int rc = check_gather_shape(M, K)) return rc;
  if (act_dtype != QLLM_F16 && act_dtype != QLLM_BF16) return set_error(QLLM_ERR_INVALID, "act_dtype must be QLLM_F16 or QLLM_BF16");
  if ((uintptr_t)x % 16 || (uintptr_t)out % 16 || (uintptr_t)perm % 16) return set_error(QLLM_ERR_INVALID, "x / perm / out must be 16-byte aligned");
  if (x == out) return set_error(QLLM_ERR_INVALID, "the gather is not in-place: out must not alias x");
  if (int rc = check_gather_served(K)) return rc;
  if (M == 0) return QLLM_OK;
  return launch_gather_columns(x, perm, out, M, K, (hipStream_t)stream);
}

int qllm_gather_describe(int32_t M, int32_t K, char *buf, size_t buflen) {
  clear_error();
  if (!buf || buflen == 0) return set_error(QLLM_ERR_INVALID, "buf must not be NULL or empty");
  if (int rc = check_gather_shape(M, K)) return rc;
  if (int rc = check_gather_served(K)) return describe_refusal(rc, kUnsupported, buf, buflen);
  if (M == 0) {
    snprintf(buf, buflen, "gather nothing (M=0)");
    return QLLM_OK;
  }
  const GatherForm f = gather_form(M, K);
  if (f.rows)
    snprintf(buf, buflen, "gather rows=%d cpt=%d grid=%d lds=%zu", f.rows, f.cpt, f.grid, f.lds);
  else
    snprintf(buf, buflen, "gather columns chunks=%d parts=%d rows_per_block=%d grid=%dx%d lds=%zu", f.chunks, f.parts, f.rows_per_block, f.grid, f.parts, f.lds);
  return QLLM_OK;
}

int qllm_linear_forward_permuted(const qllm_weight_t *w, const int32_t *perm_k, const void *x, void *y, int32_t M, int32_t act_dtype,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  if (w->g_idx) return set_error(QLLM_ERR_INVALID, "qllm_linear_forward_permuted takes a plain layer (g_idx must be NULL: sort the rows by group, pass the order as perm_k)");
  if (!perm_k || (uintptr_t)perm_k % 16) return set_error(QLLM_ERR_INVALID, "perm_k must not be NULL and must be 16-byte aligned");
  rc = check_io(x, y, M, act_dtype);
  if (rc) return rc;
  static const char kInstead[] = "gather x with qllm_gather_columns and call qllm_linear_forward, or use qllm_dequant + GEMM";
  if (!knob("QLLM_BITGEMV", 1)) return set_error(QLLM_ERR_UNSUPPORTED, "QLLM_BITGEMV is off, and only the bit-stream matvec gathers while it stages x; %s", kInstead);
  if (!bitgemv_ok(*w, M))
    return set_error(QLLM_ERR_UNSUPPORTED, "the gathering matvec serves GPTQ / HQQ row-stream layers of 2..8 bits with K %% 32 == 0, group_size %% 32 == 0 and M <= %d "
                     "(got bits=%d K=%d N=%d g=%d layout=%d M=%d); %s", kBitGemvMaxM, w->bits, w->K, w->N, w->group_size, w->layout, M, kInstead);
  if ((long long)M * w->K >= (1ll << 31)) return set_error(QLLM_ERR_UNSUPPORTED, "the gathering matvec indexes x with 32 bits: M * K must be below 2^31 (M=%d K=%d); %s", M, w->K, kInstead);
  return run_bitgemv(w, y, x, M, act_dtype, workspace, workspace_bytes, (hipStream_t)stream, perm_k);
}

// why qllm_linear_forward_bitpanel does not serve (w, M): the status, with the text in qllm_last_error(); QLLM_OK: served
static int bitpanel_check(const qllm_weight_t *w, int M) {
  static const char kInstead[] = "use qllm_dequant + a GEMM";
  if (w->g_idx) return set_error(QLLM_ERR_INVALID, "qllm_linear_forward_bitpanel takes a plain layer (g_idx must be NULL: sort the rows by group and gather x with qllm_gather_columns)");
  if (!knob("QLLM_BITPANEL", 1)) return set_error(QLLM_ERR_UNSUPPORTED, "QLLM_BITPANEL is off; %s", kInstead);
  if (M < kBitPanelMinM) return set_error(QLLM_ERR_UNSUPPORTED, "the mid-batch kernel serves %d..%d rows (got M=%d); call qllm_linear_forward, or %s", kBitPanelMinM, kBitPanelMaxM, M, kInstead);
  if (M > kBitPanelMaxM) return set_error(QLLM_ERR_UNSUPPORTED, "the mid-batch kernel serves %d..%d rows (got M=%d); %s", kBitPanelMinM, kBitPanelMaxM, M, kInstead);
  if (const char *why = bitpanel_refusal(*w))
    return set_error(QLLM_ERR_UNSUPPORTED, "the mid-batch kernel: %s (got bits=%d K=%d N=%d g=%d layout=%d); %s", why, w->bits, w->K, w->N, w->group_size, w->layout, kInstead);
  return QLLM_OK;
}

int qllm_linear_forward_bitpanel(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *workspace,
                                 size_t workspace_bytes, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  rc = check_io(x, y, M, act_dtype);
  if (rc) return rc;
  rc = bitpanel_check(w, M);
  if (rc) return rc;
  const BitPanelGeom g = bitpanel_geometry(*w, M, usable_ws(workspace, workspace_bytes));
  BitPanelParams p;
  fill_bit_params(p, w, x, y, M, act_dtype);
  p.bits = w->bits;
  p.mt = g.mt;
  p.row_blocks = g.row_blocks;
  p.split_k = g.split_k;
  p.chunk = g.chunk;
  p.n_panels = g.n_panels;
  if (g.split_k > 1) carve(workspace, &p.counters, &p.slabs);
  return launch_bitpanel(p, g, (hipStream_t)stream);
}

size_t qllm_bitpanel_workspace_bytes(const qllm_weight_t *w, int32_t M) {
  // (the rows, the layer and its shape: not the QLLM_BITPANEL knob)
  return counters_and_slabs(!w || validate_weight(w) || M < kBitPanelMinM || M > kBitPanelMaxM || w->g_idx || bitpanel_refusal(*w),
                            [&] { return bitpanel_geometry(*w, M, SIZE_MAX); });
}

int qllm_bitpanel_describe(const qllm_weight_t *w, int32_t M, int32_t have_workspace, char *buf, size_t buflen) {
  clear_error();
  if (int rc = check_describe_args(w, M, buf, buflen)) return rc;
  if (bitpanel_check(w, M)) return describe_refusal(QLLM_ERR_UNSUPPORTED, kUnsupported, buf, buflen);  // (a g_idx too: its text says what to do)
  const BitPanelGeom g = bitpanel_geometry(*w, M, have_workspace ? SIZE_MAX : 0);
  snprintf(buf, buflen, "bitpanel bits=%d cols=64 row_tiles=%d row_blocks=%d split_k=%d", w->bits, g.mt, g.row_blocks, g.split_k);
  return QLLM_OK;
}

// why qllm_linear_forward_bitgemm does not serve (w, M): the status, with the text in qllm_last_error(); QLLM_OK: served
static int bitgemm_check(const qllm_weight_t *w, int M) {
  static const char kInstead[] = "use qllm_dequant + a GEMM";
  if (w->g_idx) return set_error(QLLM_ERR_INVALID, "qllm_linear_forward_bitgemm takes a plain layer (g_idx must be NULL: sort the rows by group and gather x with qllm_gather_columns)");
  if (!knob("QLLM_BITGEMM", 1)) return set_error(QLLM_ERR_UNSUPPORTED, "QLLM_BITGEMM is off; %s", kInstead);
  if (M < kBitGemmMinM)
    return set_error(QLLM_ERR_UNSUPPORTED, "the 2..8-bit prefill kernel serves %d rows and up (got M=%d); call qllm_linear_forward_bitpanel (17..512 rows) or qllm_linear_forward, or %s", kBitGemmMinM, M, kInstead);
  if (const char *why = bitgemm_refusal(*w))
    return set_error(QLLM_ERR_UNSUPPORTED, "the 2..8-bit prefill kernel: %s (got bits=%d K=%d N=%d g=%d layout=%d); %s", why, w->bits, w->K, w->N, w->group_size, w->layout, kInstead);
  if ((double)M * w->K * 2 >= 2147483648.0) return set_error(QLLM_ERR_UNSUPPORTED, "the 2..8-bit prefill kernel: M x K activations must be below 2 GiB (M=%d K=%d); %s", M, w->K, kInstead);
  return QLLM_OK;
}

int qllm_linear_forward_bitgemm(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *workspace,
                                size_t workspace_bytes, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  if (!x || !y) return set_error(QLLM_ERR_INVALID, "x / y must not be NULL");
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  if (act_dtype != QLLM_F16 && act_dtype != QLLM_BF16 && act_dtype != QLLM_F16_IN_BF16_OUT)
    return set_error(QLLM_ERR_INVALID, "act_dtype must be QLLM_F16 or QLLM_F16_IN_BF16_OUT");
  rc = bitgemm_check(w, M);
  if (rc) return rc;
  if (act_dtype == QLLM_BF16)
    return set_error(QLLM_ERR_UNSUPPORTED, "the 2..8-bit prefill kernel reads fp16 activations: convert x to fp16, pass QLLM_F16_IN_BF16_OUT (qllm_convert_bf16_to_f16), or use qllm_dequant + a GEMM");
  if ((uintptr_t)x % 16 || (uintptr_t)y % 16) return set_error(QLLM_ERR_UNSUPPORTED, "the 2..8-bit prefill kernel: x and y must be 16-byte aligned; use qllm_dequant + a GEMM");
  const BitGemmGeom g = bitgemm_geometry(*w, M, usable_ws(workspace, workspace_bytes));
  BitGemmParams p;
  fill_bit_params(p, w, x, y, M, QLLM_F16);
  p.bits = w->bits;
  p.out_bf16 = act_dtype == QLLM_F16_IN_BF16_OUT;
  p.split_k = g.split_k;
  if (g.split_k > 1) carve(workspace, &p.counters, &p.slabs);
  return launch_bitgemm(p, g, (hipStream_t)stream);
}

size_t qllm_bitgemm_workspace_bytes(const qllm_weight_t *w, int32_t M) {
  return counters_and_slabs(!w || validate_weight(w) || M <= 0 || bitgemm_check(w, M), [&] { return bitgemm_geometry(*w, M, SIZE_MAX); });
}

int qllm_bitgemm_describe(const qllm_weight_t *w, int32_t M, int32_t have_workspace, char *buf, size_t buflen) {
  clear_error();
  if (int rc = check_describe_args(w, M, buf, buflen)) return rc;
  if (bitgemm_check(w, M)) return describe_refusal(QLLM_ERR_UNSUPPORTED, kUnsupported, buf, buflen);  // (a g_idx too: its text says what to do)
  const BitGemmGeom g = bitgemm_geometry(*w, M, have_workspace ? SIZE_MAX : 0);
  snprintf(buf, buflen, "bitgemm bits=%d tile=256x128 tiles=%d split_k=%d", w->bits, g.tiles, g.split_k);
  return QLLM_OK;
}

// why qllm_linear_forward_bitgroup does not serve (w[0..n), M): the status -- QLLM_ERR_INVALID for arguments no call takes,
// QLLM_ERR_UNSUPPORTED for calls this kernel does not take --, with the text in qllm_last_error(); QLLM_OK: served
static int bitgroup_check(const qllm_weight_t *w, int n, int M) {
  static const char kInstead[] = "call qllm_linear_forward layer by layer";
  if (!w) return set_error(QLLM_ERR_INVALID, kArraysNull);
  if (int rc = check_layer_count(n, kBitGroupMaxLayers, "qllm_linear_forward_bitgroup: ")) return rc;
  if (int rc = check_layers(w, n)) return rc;
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  auto family = [](const qllm_weight_t &l) { return is_native(l) ? 2 : (l.layout == QLLM_LAYOUT_AWQ_GEMM ? 1 : 0); };
  for (int i = 0; i < n; ++i) {
    if (w[i].g_idx) return set_error(QLLM_ERR_INVALID, "qllm_linear_forward_bitgroup takes plain layers (layer %d: g_idx must be NULL); %s", i, kInstead);
    if (w[i].K != w[0].K || w[i].bits != w[0].bits || w[i].group_size != w[0].group_size || family(w[i]) != family(w[0]) ||
        w[i].add_zero_bias != w[0].add_zero_bias)
      return set_error(QLLM_ERR_INVALID, "qllm_linear_forward_bitgroup: layers must agree on in_features, bits, group size, layout family and add_zero_bias (layer %d differs)", i);
  }
  if (!knob("QLLM_BITGROUP", 1)) return set_error(QLLM_ERR_UNSUPPORTED, "QLLM_BITGROUP is off; %s", kInstead);
  if (M > kBitGemvMaxM) return set_error(QLLM_ERR_UNSUPPORTED, "the grouped bit-stream matvec serves 1..%d rows (got M=%d); %s", kBitGemvMaxM, M, kInstead);
  for (int i = 0; i < n; ++i)
    if (!bitgemv_ok(w[i], M))
      return set_error(QLLM_ERR_UNSUPPORTED, "the grouped bit-stream matvec serves GPTQ / HQQ row-stream layers of 2..8 bits with K %% 32 == 0 and group_size %% 32 == 0 "
                       "(layer %d: bits=%d K=%d N=%d g=%d layout=%d); %s", i, w[i].bits, w[i].K, w[i].N, w[i].group_size, w[i].layout, kInstead);
  return QLLM_OK;
}

int qllm_linear_forward_bitgroup(const qllm_weight_t *w, void *const *y, int32_t n_weights, const void *x, int32_t M, int32_t act_dtype,
                                 void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  if (!y) return set_error(QLLM_ERR_INVALID, kArraysNull);
  if (int rc = bitgroup_check(w, n_weights, M)) return rc;
  for (int i = 0; i < n_weights; ++i)
    if (int rc = check_io(x, y[i], M, act_dtype)) return rc;
  const BitGroupGeom g = bitgemv_group_geometry(w, n_weights, M, usable_ws(workspace, workspace_bytes));
  BitGemvGroupParams gp;
  memset(&gp, 0, sizeof(gp));
  gp.x = x;
  gp.M = M;
  gp.K = w[0].K;
  gp.group_size = w[0].group_size;
  gp.act_bf16 = (act_dtype == QLLM_BF16);
  gp.n_prob = n_weights;
  for (int k = 0; k < n_weights; ++k) {  // launch order: widest first
    const int i = g.order[k];
    BitGemvGroupMember &q = gp.prob[k];
    fill_layer(q, w[i], y[i]);
    q.N = w[i].N;
    q.add_zero_bias = w[i].add_zero_bias;
    q.ksplit = g.split[i];
    q.n_col_blocks = g.n_col_blocks[i];
    q.chunk_units = g.chunk_units[i];
    if (g.split[i] > 1) {  // the member's own counters and slabs, carved from the one workspace
      q.counters = (int *)workspace + g.counter_off[i];
      q.slabs = (float *)((char *)workspace + kCounterBytes + g.slab_off[i]);
    }
    gp.block_begin[k] = g.block_begin[i];
  }
  return launch_bitgemv_group(gp, g, w[0].bits, (hipStream_t)stream);
}

size_t qllm_bitgroup_workspace_bytes(const qllm_weight_t *w, int32_t n_weights, int32_t M) {
  return counters_and_slabs(bitgroup_check(w, n_weights, M), [&] { return bitgemv_group_geometry(w, n_weights, M, SIZE_MAX); });
}

int qllm_bitgroup_describe(const qllm_weight_t *w, int32_t n_weights, int32_t M, int32_t have_workspace, char *buf, size_t buflen) {
  clear_error();
  if (!buf || buflen == 0) return set_error(QLLM_ERR_INVALID, "buf must not be NULL");
  if (int rc = bitgroup_check(w, n_weights, M)) return describe_refusal(rc, kUnsupported, buf, buflen);
  const BitGroupGeom g = bitgemv_group_geometry(w, n_weights, M, have_workspace ? SIZE_MAX : 0);
  char splits[64] = "";
  size_t at = 0;
  for (int i = 0; i < n_weights && at < sizeof(splits); ++i) at += snprintf(splits + at, sizeof(splits) - at, i ? ",%d" : "%d", g.split[i]);
  snprintf(buf, buflen, "bitgroup bits=%d cols=%d layers=%d blocks=%d split_k=%s", w[0].bits, bitgemv_cols(), n_weights, g.grid, splits);
  return QLLM_OK;
}

int qllm_convert_bf16_to_f16(const void *src, void *dst, size_t n, void *stream) {
  clear_error();
  if (!src || !dst || n % 8 != 0 || (uintptr_t)src % 16 != 0 || (uintptr_t)dst % 16 != 0)
    return set_error(QLLM_ERR_INVALID, "qllm_convert_bf16_to_f16: 16-byte aligned buffers, n a multiple of 8");
  return n ? launch_bf16_to_f16(src, dst, n, (hipStream_t)stream) : QLLM_OK;
}

size_t qllm_hqq_quantize_workspace_bytes(int32_t N, int32_t K, int32_t group_size, int32_t iters) {
  return hqq_quant_workspace_bytes(N, K, group_size, iters);
}

int qllm_hqq_quantize(const void *w_nk, int32_t w_dtype, int32_t N, int32_t K, int32_t bits, int32_t group_size, int32_t iters, float lp_norm,
                      float beta, float kappa, void *qweight, void *scales, void *zeros, int32_t *rounds_run_dev, void *workspace,
                      size_t workspace_bytes, void *stream) {
  clear_error();
  if (int rc = check_quant_layer("w_nk / qweight / scales / zeros", !w_nk || !qweight || !scales || !zeros, w_dtype, N, K, group_size)) return rc;
  if (bits < 1 || bits > 8) return set_error(QLLM_ERR_INVALID, "bad bits (%d)", bits);
  if (iters < 1 || iters > 64) return set_error(QLLM_ERR_INVALID, "iters must be 1..64 (got %d)", iters);
  if (!(beta > 0.f) || !(kappa > 0.f) || !(lp_norm > 0.f)) return set_error(QLLM_ERR_INVALID, "lp_norm, beta and kappa must be positive");
  if ((uintptr_t)w_nk % 16 || (uintptr_t)qweight % 4 || (uintptr_t)scales % 2 || (uintptr_t)zeros % 2 || (uintptr_t)rounds_run_dev % 4)
    return set_error(QLLM_ERR_INVALID, "w_nk must be 16-byte aligned, the outputs aligned to their element size");
  if (!hqq_quant_shape_ok(N, K, bits, group_size))
    return set_error(QLLM_ERR_UNSUPPORTED, "the HQQ quantizer serves bits 2/3/4/8, group_size %% 32 == 0 in 32..1024, K %% group_size == 0, N %% 16 == 0 "
                     "(got bits=%d group_size=%d K=%d N=%d)", bits, group_size, K, N);
  if (!(lp_norm < 1.f)) return set_error(QLLM_ERR_UNSUPPORTED, "the HQQ quantizer serves lp_norm < 1 (got %g)", (double)lp_norm);
  if (int rc = check_workspace("qllm_hqq_quantize", workspace, workspace_bytes, hqq_quant_workspace_bytes(N, K, group_size, iters))) return rc;
  return launch_hqq_quantize(w_nk, w_dtype, N, K, bits, group_size, iters, lp_norm, beta, kappa, qweight, scales, zeros, rounds_run_dev, workspace,
                             workspace_bytes, (hipStream_t)stream);
}

size_t qllm_gptq_quantize_workspace_bytes(int32_t N, int32_t K) { return gptq_quant_workspace_bytes(N, K); }

// what the two GPTQ entry points check alike, in this order, all of it before any device work
static int gptq_check(const char *fn, const void *w_nk, int32_t w_dtype, const float *u_kk, int32_t N, int32_t K, int32_t bits, int32_t group_size,
                      int32_t sym, const int32_t *codes_kn, const float *scales_ng, const float *zeros_ng, const void *wq_nk, const float *loss_n,
                      const void *workspace, size_t workspace_bytes) {
  if (int rc = check_quant_layer("w_nk / codes_kn / scales_ng / zeros_ng", !w_nk || !codes_kn || !scales_ng || !zeros_ng, w_dtype, N, K, group_size))
    return rc;
  if (sym < 0 || sym > 1) return set_error(QLLM_ERR_INVALID, "sym must be 0 or 1 (got %d)", sym);
  if (!gptq_quant_shape_ok(K, bits, group_size))
    return set_error(QLLM_ERR_UNSUPPORTED, "the GPTQ quantizer serves bits 2..8 and group_size 32 / 64 / 128 / K (got bits=%d group_size=%d K=%d)",
                     bits, group_size, K);
  if (int rc = check_whole_groups(K, group_size)) return rc;
  if (K % 4 != 0) return set_error(QLLM_ERR_INVALID, "K must be a multiple of 4 (K=%d)", K);
  if ((uintptr_t)u_kk % 16) return set_error(QLLM_ERR_INVALID, "u_kk must be 16-byte aligned: its tiles are read four floats at a time");
  const int esz = elem_size(w_dtype);
  if ((uintptr_t)w_nk % esz || (uintptr_t)wq_nk % esz || (uintptr_t)codes_kn % 4 || (uintptr_t)scales_ng % 4 ||
      (uintptr_t)zeros_ng % 4 || (uintptr_t)loss_n % 4)
    return set_error(QLLM_ERR_INVALID, "%s", kElemAligned);
  return check_workspace(fn, workspace, workspace_bytes, gptq_quant_workspace_bytes(N, K));
}

int qllm_gptq_quantize(const void *w_nk, int32_t w_dtype, const float *u_kk, int32_t N, int32_t K, int32_t bits, int32_t group_size, int32_t sym,
                       int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, float *loss_n, void *workspace, size_t workspace_bytes,
                       void *stream) {
  clear_error();
  if (int rc = gptq_check("qllm_gptq_quantize", w_nk, w_dtype, u_kk, N, K, bits, group_size, sym, codes_kn, scales_ng, zeros_ng, wq_nk, loss_n,
                          workspace, workspace_bytes))
    return rc;
  return launch_gptq_quantize(w_nk, w_dtype, u_kk, N, K, bits, group_size, sym, codes_kn, scales_ng, zeros_ng, wq_nk, loss_n, workspace,
                              (hipStream_t)stream);
}

int qllm_gptq_quantize_static(const void *w_nk, int32_t w_dtype, const float *u_kk, const int32_t *perm_k, int32_t N, int32_t K, int32_t bits,
                              int32_t group_size, int32_t sym, int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, float *loss_n,
                              void *workspace, size_t workspace_bytes, void *stream) {
  clear_error();
  if ((uintptr_t)perm_k % 4) return set_error(QLLM_ERR_INVALID, "perm_k must be 4-byte aligned");
  if (int rc = gptq_check("qllm_gptq_quantize_static", w_nk, w_dtype, u_kk, N, K, bits, group_size, sym, codes_kn, scales_ng, zeros_ng, wq_nk,
                          loss_n, workspace, workspace_bytes))
    return rc;
  return launch_gptq_quantize_static(w_nk, w_dtype, u_kk, perm_k, N, K, bits, group_size, sym, codes_kn, scales_ng, zeros_ng, wq_nk, loss_n,
                                     workspace, (hipStream_t)stream);
}

size_t qllm_awq_clip_search_workspace_bytes(int32_t N, int32_t K, int32_t group_size) { return awq_clip_search_workspace_bytes(N, K, group_size); }

// what the two AWQ entry points check alike: the weight, its type, the shape and the grid
static int awq_check_layer(const void *w_nk, int32_t w_dtype, int32_t N, int32_t K, int32_t bits, int32_t group_size) {
  if (int rc = check_quant_layer("w_nk", !w_nk, w_dtype, N, K, group_size)) return rc;
  if (!awq_quant_shape_ok(bits, group_size))
    return set_error(QLLM_ERR_UNSUPPORTED, "the AWQ quantizer serves bits 2..8 and group_size 32 / 64 / 128 (got bits=%d group_size=%d)", bits, group_size);
  if (int rc = check_whole_groups(K, group_size)) return rc;
  if ((uintptr_t)w_nk % elem_size(w_dtype)) return set_error(QLLM_ERR_INVALID, "%s", kElemAligned);
  return QLLM_OK;
}

int qllm_awq_clip_search(const void *w_nk, int32_t w_dtype, const float *gram, int32_t N, int32_t K, int32_t bits, int32_t group_size, int32_t n_grid,
                         float max_shrink, float *best_max_ng, int32_t *best_idx_ng, float *err_ng2, void *workspace, size_t workspace_bytes,
                         void *stream) {
  clear_error();
  if (!gram || !best_max_ng || !best_idx_ng || !err_ng2) return set_error(QLLM_ERR_INVALID, "gram / best_max_ng / best_idx_ng / err_ng2 must not be NULL");
  if (int rc = awq_check_layer(w_nk, w_dtype, N, K, bits, group_size)) return rc;
  if (!awq_clip_candidates(n_grid, max_shrink))
    return set_error(QLLM_ERR_UNSUPPORTED, "the clip search evaluates int(max_shrink * n_grid) = 1..10 candidates, 0 < max_shrink <= 1 (got n_grid=%d max_shrink=%g)",
                     n_grid, (double)max_shrink);
  if ((uintptr_t)gram % kAwqGramAlign) return set_error(QLLM_ERR_INVALID, "gram must be 16-byte aligned: its tiles are read four floats at a time");
  if ((uintptr_t)best_max_ng % 4 || (uintptr_t)best_idx_ng % 4 || (uintptr_t)err_ng2 % 4) return set_error(QLLM_ERR_INVALID, "%s", kElemAligned);
  if (int rc = check_workspace("qllm_awq_clip_search", workspace, workspace_bytes, awq_clip_search_workspace_bytes(N, K, group_size))) return rc;
  return launch_awq_clip_search(w_nk, w_dtype, gram, N, K, bits, group_size, n_grid, max_shrink, best_max_ng, best_idx_ng, err_ng2, (hipStream_t)stream);
}

int qllm_awq_quantize(const void *w_nk, int32_t w_dtype, const float *col_scale_k, const float *clip_ng, int32_t N, int32_t K, int32_t bits,
                      int32_t group_size, int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, void *stream) {
  clear_error();
  if (int rc = awq_check_layer(w_nk, w_dtype, N, K, bits, group_size)) return rc;
  if ((uintptr_t)col_scale_k % 4 || (uintptr_t)clip_ng % 4 || (uintptr_t)codes_kn % 4 || (uintptr_t)scales_ng % 4 || (uintptr_t)zeros_ng % 4 ||
      (uintptr_t)wq_nk % elem_size(w_dtype))
    return set_error(QLLM_ERR_INVALID, "%s", kElemAligned);
  if (!codes_kn && !scales_ng && !zeros_ng && !wq_nk) return set_error(QLLM_ERR_INVALID, "every output is NULL: nothing to write");
  return launch_awq_quantize(w_nk, w_dtype, col_scale_k, clip_ng, N, K, bits, group_size, codes_kn, scales_ng, zeros_ng, wq_nk, (hipStream_t)stream);
}

int qllm_debug_timeline(void *buf, int32_t n_slots) {  // n_slots x 24 x u64
  clear_error();
  g_timeline = (uint64_t *)buf;
  g_timeline_slots = buf ? n_slots : 0;
  g_timeline_next = 0;
  return QLLM_OK;
}

int qllm_linear_forward(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *workspace,
                        size_t workspace_bytes, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  if (act_dtype == QLLM_F16_IN_BF16_OUT) {
    // x already converted by the caller: only the 256x128 prefill kernel writes bf16 from fp16 inputs (out_bf16) -- the call must be
    // one the regular path hands to that kernel (the same Decision and the same tile choice)
    rc = check_io(x, y, M, QLLM_F16);
    if (rc) return rc;
    if (w->bits != 4 || w->g_idx || M <= 64)
      return set_error(QLLM_ERR_UNSUPPORTED, "QLLM_F16_IN_BF16_OUT: 4-bit prefill calls of the 256x128 kernel only");
    const Decision d = decide_single(w, M, QLLM_F16);
    if (d.route != ROUTE_TILE) return set_error(QLLM_ERR_UNSUPPORTED, kNotPrefillKernel, M, w->K, w->N);
    GemmParams p;
    fill_launch_params(p, w, x, y, M, QLLM_F16);
    return run_tile_gemm(p, d.layout, workspace, workspace_bytes, (hipStream_t)stream, true);
  }
  rc = check_io(x, y, M, act_dtype);
  if (rc) return rc;
  const Decision d = decide_single(w, M, act_dtype);
  void *ys[1] = {y};
  return execute(d, w, ys, 1, x, M, act_dtype, workspace, workspace_bytes, (hipStream_t)stream);
}

int qllm_linear_forward_allreduce(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *const *peers_dev,
                                  int32_t rank, int32_t world, size_t slot_bytes, int32_t *status_dev, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  rc = check_io(x, y, M, act_dtype);
  if (rc) return rc;
  if (!peers_dev) return set_error(QLLM_ERR_INVALID, "qllm_linear_forward_allreduce: peers_dev is NULL");
  if (world < 1 || world > kCommMaxWorld || rank < 0 || rank >= world) return set_error(QLLM_ERR_INVALID, "world must be 1..%d and 0 <= rank < world (rank=%d world=%d)", kCommMaxWorld, rank, world);
  StripPlan pl;
  // the batch-1 kernel's shapes only (callers run the layer and qllm_allreduce_oneshot / RCCL separately for everything else)
  if (M != 1 || !is_native(*w) || w->bits != 4 || w->group_size != 128 || !strip_plan(w, 1, 1, &pl) || !pl.one_nw)
    return set_error(QLLM_ERR_UNSUPPORTED, "fused all-reduce: batch-1 calls on native 4-bit layers with 128-wide groups (M=%d bits=%d g=%d layout=%d)", M, w->bits, w->group_size, w->layout);
  if ((size_t)w->N * 2 > slot_bytes || slot_bytes % 16 != 0 || (uintptr_t)y % 16 != 0)
    return set_error(QLLM_ERR_UNSUPPORTED, "fused all-reduce: N * 2 <= slot_bytes, slot_bytes %% 16 == 0, y 16-byte aligned (N=%d slot=%zu)", w->N, slot_bytes);
  Strip1Params p;
  void *ys[1] = {y};
  fill_strip1_params(p, w, ys, 1, x, 1, act_dtype);
  p.ar_peers = peers_dev;
  p.ar_status = status_dev;
  p.ar_rank = rank;
  p.ar_world = world;
  p.ar_slot_bytes = (uint32_t)slot_bytes;
  return launch_strip1_allreduce(p, pl.one_nw, pl.one_maxs, w->N / 16, (hipStream_t)stream);
}

// y = linear(w, act(gate) * up): the SWIGLU forms of the batch-1 kernel (strip1_swiglu.hip); decide_swiglu says what is served
int qllm_linear_forward_swiglu(const qllm_weight_t *w, const void *gate, const void *up, void *y, int32_t M, int32_t act_dtype, int32_t act,
                               void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  if (!gate || !up) return set_error(QLLM_ERR_INVALID, "gate / up must not be NULL");
  rc = check_io(gate, y, M, act_dtype);
  if (rc) return rc;
  if ((uintptr_t)up % 16 != 0) return set_error(QLLM_ERR_INVALID, "up must be 16-byte aligned");
  if (y == gate || y == up) return set_error(QLLM_ERR_INVALID, "y must not alias gate / up");
  StripPlan pl;
  rc = decide_swiglu(w, M, act, &pl);
  if (rc) return rc;
  Strip1Params p;
  void *ys[1] = {y};
  fill_strip1_params(p, w, ys, 1, gate, M, act_dtype);
  p.x2 = up;
  return launch_strip1_swiglu(p, pl.one_nw, pl.one_maxs, w->N / 16, (hipStream_t)stream);
}

// what that call would launch, as text ("swiglu " + the plain call's plan line), or why it is refused -- no device work
int qllm_swiglu_describe(const qllm_weight_t *w, int32_t M, char *buf, size_t buflen) {
  clear_error();
  if (!w || !buf || buflen < 64) return set_error(QLLM_ERR_INVALID, "w / buf must not be NULL (buf >= 64 bytes)");
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  Decision d;
  memset(&d, 0, sizeof(d));
  d.route = ROUTE_STRIP;
  int rc = validate_weight(w);
  if (rc == QLLM_OK) rc = decide_swiglu(w, M, QLLM_ACT_SILU, &d.strip);
  if (rc) return describe_refusal(rc, kRefused, buf, buflen);
  return describe_fused("swiglu", d, w, 1, M, buf, buflen);
}

// y = residual + linear(w, x), or residual + linear(w, act(x) * up): the RESID forms of the batch-1 kernel (strip1_resid.hip,
// strip1_swiglu_resid.hip); decide_residual says what is served
int qllm_linear_forward_residual(const qllm_weight_t *w, const void *x, const void *up, const void *residual, void *y, int32_t M, int32_t act_dtype,
                                 int32_t act, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  if (!residual) return set_error(QLLM_ERR_INVALID, "residual must not be NULL");
  rc = check_io(x, y, M, act_dtype);
  if (rc) return rc;
  if ((uintptr_t)up % 16 != 0) return set_error(QLLM_ERR_INVALID, "up must be 16-byte aligned");
  if ((uintptr_t)residual % 2 != 0 || (uintptr_t)y % 2 != 0) return set_error(QLLM_ERR_INVALID, "residual / y must be aligned to the element size");
  // y may BE the residual row (the thread that writes element n is the only one that reads it, and reads first); nothing else may overlap
  auto overlap = [](const void *a, size_t na, const void *b, size_t nb) { return (uintptr_t)a < (uintptr_t)b + nb && (uintptr_t)b < (uintptr_t)a + na; };
  const size_t ybytes = (size_t)M * w->N * 2, xbytes = (size_t)M * w->K * 2;
  if (y != residual && overlap(y, ybytes, residual, ybytes)) return set_error(QLLM_ERR_INVALID, "y may be residual itself, but must not overlap it otherwise");
  if (overlap(y, ybytes, x, xbytes) || (up && overlap(y, ybytes, up, xbytes))) return set_error(QLLM_ERR_INVALID, "y must not alias x / up (every block reads the whole row)");
  if (up && act != QLLM_ACT_SILU) return set_error(QLLM_ERR_INVALID, "act=%d is not an activation (QLLM_ACT_SILU) for the up vector", act);
  StripPlan pl;
  rc = decide_residual(w, M, &pl);
  if (rc) return rc;
  Strip1Params p;
  void *ys[1] = {y};
  fill_strip1_params(p, w, ys, 1, x, M, act_dtype);
  p.x2 = up;
  p.residual = residual;
  return up ? launch_strip1_swiglu_resid(p, pl.one_nw, pl.one_maxs, w->N / 16, (hipStream_t)stream)
            : launch_strip1_resid(p, pl.one_nw, pl.one_maxs, w->N / 16, (hipStream_t)stream);
}

// what that call would launch, as text ("residual " / "residual swiglu " + the plain call's plan line), or why it is refused -- no device work
int qllm_residual_describe(const qllm_weight_t *w, int32_t M, int32_t swiglu, char *buf, size_t buflen) {
  clear_error();
  if (!w || !buf || buflen < 64) return set_error(QLLM_ERR_INVALID, "w / buf must not be NULL (buf >= 64 bytes)");
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  Decision d;
  memset(&d, 0, sizeof(d));
  d.route = ROUTE_STRIP;
  int rc = validate_weight(w);
  if (rc == QLLM_OK) rc = decide_residual(w, M, &d.strip);
  if (rc) return describe_refusal(rc, kRefused, buf, buflen);
  return describe_fused(swiglu ? "residual swiglu" : "residual", d, w, 1, M, buf, buflen);
}

// y = weight * round(x * rstd) per row: the standalone RMSNorm kernel (rmsnorm.hip)
int qllm_rmsnorm(const void *x, const void *weight, void *y, int32_t M, int32_t K, float eps, int32_t act_dtype, float *rstd_out, void *stream) {
  clear_error();
  if (!x || !weight || !y) return set_error(QLLM_ERR_INVALID, "x / weight / y must not be NULL");
  if (M <= 0 || K <= 0) return set_error(QLLM_ERR_INVALID, "M and K must be >= 1 (got M=%d K=%d)", M, K);
  if (act_dtype != QLLM_F16 && act_dtype != QLLM_BF16) return set_error(QLLM_ERR_INVALID, "act_dtype must be QLLM_F16 or QLLM_BF16");
  if ((uintptr_t)x % 16 || (uintptr_t)weight % 16 || (uintptr_t)y % 16) return set_error(QLLM_ERR_INVALID, "x / weight / y must be 16-byte aligned");
  if ((uintptr_t)rstd_out % 4) return set_error(QLLM_ERR_INVALID, "rstd_out must be 4-byte aligned");
  if (K % 8 != 0) return set_error(QLLM_ERR_INVALID, "K must be a multiple of 8 (whole 16-byte chunks; got %d)", K);
  if (!(eps >= 0.f)) return set_error(QLLM_ERR_INVALID, "eps must be >= 0");
  if (K > kRmsNormMaxK) return set_error(QLLM_ERR_UNSUPPORTED, "rmsnorm serves K <= %d (got %d)", kRmsNormMaxK, K);
  return launch_rmsnorm(x, weight, y, M, K, eps, act_dtype == QLLM_BF16, rstd_out, (hipStream_t)stream);
}

// y_i = linear(w_i, RMSNorm(x)): the NORM forms of the batch-1 kernel (strip1_norm.hip); decide_rmsnorm says what is served
int qllm_linear_forward_rmsnorm(const qllm_weight_t *w, void *const *y, int32_t n_weights, const void *x, const void *norm_weight, float eps,
                                int32_t M, int32_t act_dtype, float *rstd_out, void *stream) {
  clear_error();
  if (!w || !y) return set_error(QLLM_ERR_INVALID, kArraysNull);
  if (int rc = check_layer_count(n_weights, kMaxProblems)) return rc;
  if (!norm_weight) return set_error(QLLM_ERR_INVALID, "norm_weight must not be NULL");
  auto output_ok = [&](int i) {
    if (int rc = check_io(x, y[i], M, act_dtype)) return rc;
    if (y[i] == x || y[i] == norm_weight) return set_error(QLLM_ERR_INVALID, "y must not alias x / norm_weight (every block reads the whole row)");
    return (int)QLLM_OK;
  };
  if (int rc = check_layers(w, n_weights, output_ok)) return rc;
  if ((uintptr_t)norm_weight % 16 != 0) return set_error(QLLM_ERR_INVALID, "norm_weight must be 16-byte aligned");
  if ((uintptr_t)rstd_out % 4) return set_error(QLLM_ERR_INVALID, "rstd_out must be 4-byte aligned");
  if (!(eps >= 0.f)) return set_error(QLLM_ERR_INVALID, "eps must be >= 0");
  if (w[0].K % 8 != 0) return set_error(QLLM_ERR_INVALID, "K must be a multiple of 8 (got %d)", w[0].K);
  Decision d;
  if (int rc = decide_rmsnorm(w, n_weights, M, &d)) return rc;
  Strip1Params p;
  const int max_strips = fill_strip1_params(p, w, y, n_weights, x, M, act_dtype);
  p.norm_w = norm_weight;
  p.norm_eps = eps;
  p.rstd_out = rstd_out;
  return launch_strip1_norm(p, d.strip.one_nw, d.strip.one_maxs, n_weights, max_strips, (hipStream_t)stream);
}

// what that call would launch, as text ("rmsnorm " + the plain grouped call's plan line), or why it is refused -- no device work
int qllm_rmsnorm_describe(const qllm_weight_t *w, int32_t n_weights, int32_t M, char *buf, size_t buflen) {
  clear_error();
  if (!w || !buf || buflen < 64) return set_error(QLLM_ERR_INVALID, "w / buf must not be NULL (buf >= 64 bytes)");
  if (int rc = check_layer_count(n_weights, kMaxProblems)) return rc;
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  Decision d;
  int rc = check_layers(w, n_weights);
  if (rc == QLLM_OK) rc = decide_rmsnorm(w, n_weights, M, &d);
  if (rc) return describe_refusal(rc, kRefused, buf, buflen);
  return describe_fused("rmsnorm", d, w, n_weights, M, buf, buflen);
}

// q_out = q * cos + rotate_half(q) * sin, k_out likewise: the rotary embedding of q and k in one launch (rope.hip)
int qllm_rope(const void *q, const void *k, const void *cos, const void *sin, void *q_out, void *k_out, int32_t rows, int32_t q_heads, int32_t k_heads,
              int32_t head_dim, int64_t q_row_stride, int64_t q_head_stride, int64_t k_row_stride, int64_t k_head_stride, int32_t cos_rows,
              int32_t act_dtype, void *stream) {
  clear_error();
  if (!q || !cos || !sin || !q_out) return set_error(QLLM_ERR_INVALID, "q / cos / sin / q_out must not be NULL");
  if (k_heads < 0 || (k_heads == 0) != (k == nullptr) || (k_heads == 0) != (k_out == nullptr))
    return set_error(QLLM_ERR_INVALID, "k and k_out must not be NULL with k_heads >= 1, and both NULL with k_heads == 0 (got k_heads=%d)", k_heads);
  if (rows <= 0 || q_heads <= 0 || head_dim <= 0)
    return set_error(QLLM_ERR_INVALID, "rows, q_heads and head_dim must be >= 1 (got rows=%d q_heads=%d head_dim=%d)", rows, q_heads, head_dim);
  if (act_dtype != QLLM_F16 && act_dtype != QLLM_BF16) return set_error(QLLM_ERR_INVALID, "act_dtype must be QLLM_F16 or QLLM_BF16");
  if (cos_rows <= 0 || rows % cos_rows != 0) return set_error(QLLM_ERR_INVALID, "cos_rows must be >= 1 and divide rows (got cos_rows=%d rows=%d)", cos_rows, rows);
  if ((uintptr_t)q % 16 || (uintptr_t)k % 16 || (uintptr_t)cos % 16 || (uintptr_t)sin % 16 || (uintptr_t)q_out % 16 || (uintptr_t)k_out % 16)
    return set_error(QLLM_ERR_INVALID, "q / k / cos / sin / q_out / k_out must be 16-byte aligned");
  const int64_t strides[4] = {q_row_stride, q_head_stride, k_row_stride, k_head_stride};
  for (int i = 0; i < (k ? 4 : 2); ++i)
    if (strides[i] < 0 || strides[i] % 8 != 0)
      return set_error(QLLM_ERR_INVALID, "row and head strides must be non-negative multiples of 8 elements (got %lld)", (long long)strides[i]);
  // an output may BE its input only where both have one layout (a thread then writes what it alone has read)
  if ((q_out == q && (q_head_stride != head_dim || q_row_stride != (int64_t)q_heads * head_dim)) ||
      (k && k_out == k && (k_head_stride != head_dim || k_row_stride != (int64_t)k_heads * head_dim)))
    return set_error(QLLM_ERR_INVALID, "an output may be its input only with contiguous strides (head_stride == head_dim, row_stride == heads * head_dim)");
  if (head_dim % 16 != 0 || head_dim < 16 || head_dim > kRopeMaxHeadDim)
    return set_error(QLLM_ERR_UNSUPPORTED, "rope serves head_dim %% 16 == 0, 16 <= head_dim <= %d (got %d)", kRopeMaxHeadDim, head_dim);
  return launch_rope(q, k, cos, sin, q_out, k_out, rows, q_heads, k_heads, head_dim, q_row_stride, q_head_stride, k_row_stride, k_head_stride, cos_rows,
                     act_dtype == QLLM_BF16, (hipStream_t)stream);
}

// ---- attention over the KV cache: the host rules of the decode and the prefill entries, each written once -----------------------------------
// What differs between the two kernels is an argument: the name in the "%s serves ..." texts, the pointers and strides an entry has and
// the words its texts call them by.  The entries call these in one order -- the call,
// the layout, the length and the mask's reach (their own: one row of one stride against rows of two), what the kernel serves -- with the
// rules only one of them has in between.

// sizes, the number of query rows (q_len NULL: one, the decode entries), the head ratio
static int check_attn_shape(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, const int32_t *q_len, int64_t max_len) {
  if (batch <= 0 || q_heads <= 0 || kv_heads <= 0 || head_dim <= 0 || max_len <= 0)
    return set_error(QLLM_ERR_INVALID, "batch, q_heads, kv_heads, head_dim and max_len must be >= 1 (got %d, %d, %d, %d, %lld)", batch, q_heads, kv_heads,
                     head_dim, (long long)max_len);
  if (q_len && (*q_len < 2 || *q_len > max_len))
    return set_error(QLLM_ERR_INVALID, "q_len must lie in 2..max_len (got q_len=%d max_len=%lld); one token is qllm_attn_decode's", *q_len, (long long)max_len);
  if (q_heads % kv_heads != 0) return set_error(QLLM_ERR_INVALID, "kv_heads must divide q_heads (got q_heads=%d kv_heads=%d)", q_heads, kv_heads);
  return QLLM_OK;
}

// what both kernels are built for; the bound on the grid is each entry's own
static int check_attn_served(const char *name, int32_t q_heads, int32_t kv_heads, int32_t head_dim) {
  if (head_dim != 64 && head_dim != 128) return set_error(QLLM_ERR_UNSUPPORTED, "%s serves head_dim 64 and 128 (got %d)", name, head_dim);
  if (q_heads / kv_heads > kAttnDecodeMaxGroup)
    return set_error(QLLM_ERR_UNSUPPORTED, "%s serves 1..%d query heads per kv head (got %d)", name, kAttnDecodeMaxGroup, q_heads / kv_heads);
  return QLLM_OK;
}

// the head of a call: the four pointers every call has, the shape, the window, the activation type, the mask and its kind
static int check_attn_call(const void *q, const void *k_cache, const void *v_cache, const void *out, int32_t batch, int32_t q_heads, int32_t kv_heads,
                           int32_t head_dim, const int32_t *q_len, int64_t max_len, int64_t window, int32_t act_dtype, int32_t mask_kind, const void *mask) {
  if (!q || !k_cache || !v_cache || !out) return set_error(QLLM_ERR_INVALID, "q / k_cache / v_cache / out must not be NULL");
  int rc = check_attn_shape(batch, q_heads, kv_heads, head_dim, q_len, max_len);
  if (rc != QLLM_OK) return rc;
  if (window < 0) return set_error(QLLM_ERR_INVALID, "window must be 0 (none) or >= 1 (got %lld)", (long long)window);
  if (act_dtype != QLLM_F16 && act_dtype != QLLM_BF16) return set_error(QLLM_ERR_INVALID, "act_dtype must be QLLM_F16 or QLLM_BF16");
  if (mask_kind != QLLM_ATTN_MASK_NONE && mask_kind != QLLM_ATTN_MASK_BOOL && mask_kind != QLLM_ATTN_MASK_ADDITIVE)
    return set_error(QLLM_ERR_INVALID, "mask_kind must be QLLM_ATTN_MASK_NONE, _BOOL or _ADDITIVE (got %d)", mask_kind);
  if ((mask_kind == QLLM_ATTN_MASK_NONE) != (mask == nullptr)) return set_error(QLLM_ERR_INVALID, "mask must be NULL exactly with QLLM_ATTN_MASK_NONE");
  return QLLM_OK;
}

// alignment of the `n_ptrs` tensors `ptr_names` lists (a NULL one is aligned), of the device length and of an additive mask; then the
// first `n_strides` strides, which `stride_words` names
static int check_attn_layout(const char *ptr_names, const void *const *ptrs, int n_ptrs, const int64_t *kv_len_dev, int32_t mask_kind, const void *mask,
                             const char *stride_words, const int64_t *strides, int n_strides) {
  for (int i = 0; i < n_ptrs; ++i)
    if ((uintptr_t)ptrs[i] % 16) return set_error(QLLM_ERR_INVALID, "%s must be 16-byte aligned", ptr_names);
  if ((uintptr_t)kv_len_dev % 8 || (mask_kind == QLLM_ATTN_MASK_ADDITIVE && (uintptr_t)mask % 2))
    return set_error(QLLM_ERR_INVALID, "kv_len_dev must be 8-byte aligned and an additive mask 2-byte aligned");
  for (int i = 0; i < n_strides; ++i)
    if (strides[i] < 0 || strides[i] % 8 != 0)
      return set_error(QLLM_ERR_INVALID, "%s strides must be non-negative multiples of 8 elements (got %lld)", stride_words, (long long)strides[i]);
  return QLLM_OK;
}

// ---- single-token attention over the KV cache (attn_decode.hip) ------------------------------------------------------------------------
// what the kernel serves, and one arrival counter per (sequence, kv head) in the counter page
static int check_attn_decode_served(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim) {
  int rc = check_attn_served("attn_decode", q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return rc;
  if (batch > 65535 || kv_heads > 65535 || (int64_t)batch * kv_heads > (int64_t)(kCounterBytes / sizeof(int)))
    return set_error(QLLM_ERR_UNSUPPORTED, "attn_decode serves batch * kv_heads <= %d (got %lld)", (int)(kCounterBytes / sizeof(int)), (long long)batch * kv_heads);
  return QLLM_OK;
}

size_t qllm_attn_decode_workspace_bytes(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t max_len) {
  const bool refused = check_attn_shape(batch, q_heads, kv_heads, head_dim, nullptr, max_len) != QLLM_OK ||
                       check_attn_decode_served(batch, q_heads, kv_heads, head_dim) != QLLM_OK;
  clear_error();
  return refused ? kCounterBytes : kCounterBytes + attn_decode_geom(batch, q_heads, kv_heads, head_dim, max_len).partial_bytes;
}

int qllm_attn_decode_describe(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t max_len, char *buf, size_t buflen) {
  clear_error();
  if (!buf || buflen == 0) return set_error(QLLM_ERR_INVALID, "buf must not be NULL or empty");
  int rc = check_attn_shape(batch, q_heads, kv_heads, head_dim, nullptr, max_len);
  if (rc == QLLM_OK) rc = check_attn_decode_served(batch, q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return describe_refusal(rc, kRefused, buf, buflen);
  const AttnDecodeGeom g = attn_decode_geom(batch, q_heads, kv_heads, head_dim, max_len);
  snprintf(buf, buflen, "attn_decode tile=%d splits=%d chunk=%lld grid=%dx%dx%d group=%d combine=last-block", g.tile, g.splits, (long long)g.chunk, g.splits,
           kv_heads, batch, q_heads / kv_heads);
  return QLLM_OK;
}

int qllm_attn_decode(const void *q, const void *k_new, const void *v_new, void *k_cache, void *v_cache, const void *mask, void *out, int32_t batch,
                     int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len, int64_t q_row_stride,
                     int64_t q_head_stride, int64_t k_new_row_stride, int64_t k_new_head_stride, int64_t v_new_row_stride, int64_t v_new_head_stride,
                     int64_t cache_batch_stride, int64_t cache_head_stride, int64_t cache_pos_stride, int32_t mask_kind, int64_t mask_len,
                     int64_t mask_batch_stride, float scaling, int32_t act_dtype, void *workspace, size_t workspace_bytes, void *stream) {
  return qllm_attn_decode_window(q, k_new, v_new, k_cache, v_cache, mask, out, batch, q_heads, kv_heads, head_dim, kv_len, kv_len_dev, max_len, 0, q_row_stride,
                                 q_head_stride, k_new_row_stride, k_new_head_stride, v_new_row_stride, v_new_head_stride, cache_batch_stride, cache_head_stride,
                                 cache_pos_stride, mask_kind, mask_len, mask_batch_stride, scaling, act_dtype, workspace, workspace_bytes, stream);
}

int qllm_attn_decode_window(const void *q, const void *k_new, const void *v_new, void *k_cache, void *v_cache, const void *mask, void *out, int32_t batch,
                            int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len, int64_t window,
                            int64_t q_row_stride, int64_t q_head_stride, int64_t k_new_row_stride, int64_t k_new_head_stride, int64_t v_new_row_stride,
                            int64_t v_new_head_stride, int64_t cache_batch_stride, int64_t cache_head_stride, int64_t cache_pos_stride, int32_t mask_kind,
                            int64_t mask_len, int64_t mask_batch_stride, float scaling, int32_t act_dtype, void *workspace, size_t workspace_bytes,
                            void *stream) {
  clear_error();
  int rc = check_attn_call(q, k_cache, v_cache, out, batch, q_heads, kv_heads, head_dim, nullptr, max_len, window, act_dtype, mask_kind, mask);
  if (rc != QLLM_OK) return rc;
  if ((k_new == nullptr) != (v_new == nullptr)) return set_error(QLLM_ERR_INVALID, "k_new and v_new must be given together or not at all");
  const int64_t strides[9] = {q_row_stride, q_head_stride, cache_batch_stride, cache_head_stride, cache_pos_stride,
                              k_new_row_stride, k_new_head_stride, v_new_row_stride, v_new_head_stride};  // the last four count with an append only
  const void *const ptrs[6] = {q, k_new, v_new, k_cache, v_cache, out};
  rc = check_attn_layout("q / k_new / v_new / k_cache / v_cache / out", ptrs, 6, kv_len_dev, mask_kind, mask, "row, head, batch and position", strides,
                         k_new ? 9 : 5);
  if (rc != QLLM_OK) return rc;
  const int64_t need_len = kv_len_dev ? max_len : kv_len + (k_new ? 1 : 0);  // the positions a call may reach
  if (!kv_len_dev && (kv_len < 0 || need_len > max_len))
    return set_error(QLLM_ERR_INVALID, "kv_len%s must lie in 0..max_len (got kv_len=%lld max_len=%lld)", k_new ? " + 1 (append)" : "", (long long)kv_len, (long long)max_len);
  if (mask && (mask_len < need_len || mask_batch_stride < 0))
    return set_error(QLLM_ERR_INVALID, "the mask must cover %lld positions (%s) with a non-negative batch stride (got mask_len=%lld stride=%lld)", (long long)need_len,
                     kv_len_dev ? "max_len: the length is on the device" : "kv_len, + 1 with an append", (long long)mask_len, (long long)mask_batch_stride);
  rc = check_attn_decode_served(batch, q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return rc;
  const AttnDecodeGeom g = attn_decode_geom(batch, q_heads, kv_heads, head_dim, max_len);
  rc = check_workspace("qllm_attn_decode", workspace, workspace_bytes, kCounterBytes + g.partial_bytes);
  if (rc != QLLM_OK) return rc;

  AttnDecodeParams p;
  p.q = q, p.k_new = k_new, p.v_new = v_new, p.k_cache = k_cache, p.v_cache = v_cache, p.mask = mask, p.out = out;
  p.kv_len_dev = kv_len_dev, p.kv_len = kv_len, p.max_len = max_len, p.window = window;
  p.q_row = q_row_stride, p.q_head = q_head_stride, p.kn_row = k_new_row_stride, p.kn_head = k_new_head_stride, p.vn_row = v_new_row_stride,
  p.vn_head = v_new_head_stride, p.c_batch = cache_batch_stride, p.c_head = cache_head_stride, p.c_pos = cache_pos_stride, p.mask_batch = mask_batch_stride;
  p.chunk = g.chunk, p.batch = batch, p.q_heads = q_heads, p.kv_heads = kv_heads, p.mask_kind = mask_kind, p.splits = g.splits, p.scaling = scaling;
  carve(workspace, &p.counters, &p.partials);
  return launch_attn_decode(p, head_dim, act_dtype == QLLM_BF16, (hipStream_t)stream);
}

// the same call over a ring-buffer cache of `slots` positions (attn_decode_ring.hip): the decode entry's rules in its order, with `slots`
// where it has max_len in the shape, the ring's two rules (1 <= window <= slots; a total with no upper end) in the places of the window's
// sign and of the length's range, and the geometry, the workspace and the mask's reach of a linear call whose max_len is the window
int qllm_attn_decode_ring(const void *q, const void *k_new, const void *v_new, void *k_cache, void *v_cache, const void *mask, void *out, int32_t batch,
                          int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t total, const int64_t *total_dev, int64_t slots, int64_t window,
                          int64_t q_row_stride, int64_t q_head_stride, int64_t k_new_row_stride, int64_t k_new_head_stride, int64_t v_new_row_stride,
                          int64_t v_new_head_stride, int64_t cache_batch_stride, int64_t cache_head_stride, int64_t cache_pos_stride, int32_t mask_kind,
                          int64_t mask_len, int64_t mask_batch_stride, float scaling, int32_t act_dtype, void *workspace, size_t workspace_bytes,
                          void *stream) {
  clear_error();
  int rc = check_attn_call(q, k_cache, v_cache, out, batch, q_heads, kv_heads, head_dim, nullptr, slots, window, act_dtype, mask_kind, mask);
  if (rc != QLLM_OK) return rc;
  if (window < 1 || slots < window)
    return set_error(QLLM_ERR_INVALID, "a ring needs 1 <= window <= slots (got window=%lld slots=%lld)", (long long)window, (long long)slots);
  if ((k_new == nullptr) != (v_new == nullptr)) return set_error(QLLM_ERR_INVALID, "k_new and v_new must be given together or not at all");
  const int64_t strides[9] = {q_row_stride, q_head_stride, cache_batch_stride, cache_head_stride, cache_pos_stride,
                              k_new_row_stride, k_new_head_stride, v_new_row_stride, v_new_head_stride};  // the last four count with an append only
  const void *const ptrs[6] = {q, k_new, v_new, k_cache, v_cache, out};
  rc = check_attn_layout("q / k_new / v_new / k_cache / v_cache / out", ptrs, 6, total_dev, mask_kind, mask, "row, head, batch and position", strides,
                         k_new ? 9 : 5);
  if (rc != QLLM_OK) return rc;
  if (!total_dev && total < 0) return set_error(QLLM_ERR_INVALID, "total must be >= 0 (got %lld); it has no upper end", (long long)total);
  // the columns a call may reach: the visible positions, at most the window's
  const int64_t need_len = total_dev || total >= window ? window : total + (k_new ? 1 : 0);
  if (mask && (mask_len < need_len || mask_batch_stride < 0))
    return set_error(QLLM_ERR_INVALID, "the mask must cover %lld positions (%s) with a non-negative batch stride (got mask_len=%lld stride=%lld)", (long long)need_len,
                     total_dev ? "the window: the total is on the device" : "min(total, + 1 with an append; window)", (long long)mask_len,
                     (long long)mask_batch_stride);
  rc = check_attn_decode_served(batch, q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return rc;
  const AttnDecodeGeom g = attn_decode_geom(batch, q_heads, kv_heads, head_dim, window);
  rc = check_workspace("qllm_attn_decode_ring", workspace, workspace_bytes, kCounterBytes + g.partial_bytes);
  if (rc != QLLM_OK) return rc;

  AttnDecodeParams p;
  p.q = q, p.k_new = k_new, p.v_new = v_new, p.k_cache = k_cache, p.v_cache = v_cache, p.mask = mask, p.out = out;
  p.kv_len_dev = total_dev, p.kv_len = total, p.max_len = slots, p.window = window;
  p.q_row = q_row_stride, p.q_head = q_head_stride, p.kn_row = k_new_row_stride, p.kn_head = k_new_head_stride, p.vn_row = v_new_row_stride,
  p.vn_head = v_new_head_stride, p.c_batch = cache_batch_stride, p.c_head = cache_head_stride, p.c_pos = cache_pos_stride, p.mask_batch = mask_batch_stride;
  p.chunk = g.chunk, p.batch = batch, p.q_heads = q_heads, p.kv_heads = kv_heads, p.mask_kind = mask_kind, p.splits = g.splits, p.scaling = scaling;
  carve(workspace, &p.counters, &p.partials);
  return launch_attn_decode_ring(p, head_dim, act_dtype == QLLM_BF16, (hipStream_t)stream);
}

// ---- prefill attention over the KV cache (attn_prefill.hip) ------------------------------------------------------------------------------
// what the kernel serves, and a grid of (row tiles, q_heads, batch)
static int check_attn_prefill_served(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim) {
  int rc = check_attn_served("attn_prefill", q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return rc;
  if (batch > 65535 || q_heads > 65535)
    return set_error(QLLM_ERR_UNSUPPORTED, "attn_prefill serves batch <= 65535 and q_heads <= 65535 (got %d, %d)", batch, q_heads);
  return QLLM_OK;
}

int qllm_attn_prefill_describe(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t q_len, int64_t max_len, char *buf,
                               size_t buflen) {
  clear_error();
  if (!buf || buflen == 0) return set_error(QLLM_ERR_INVALID, "buf must not be NULL or empty");
  int rc = check_attn_shape(batch, q_heads, kv_heads, head_dim, &q_len, max_len);
  if (rc == QLLM_OK) rc = check_attn_prefill_served(batch, q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return describe_refusal(rc, kRefused, buf, buflen);
  snprintf(buf, buflen, "attn_prefill q_tile=%d kv_tile=%d grid=%dx%dx%d group=%d", kAttnPrefillQTile, kAttnPrefillKvTile,
           (q_len + kAttnPrefillQTile - 1) / kAttnPrefillQTile, q_heads, batch, q_heads / kv_heads);
  return QLLM_OK;
}

int qllm_attn_prefill(const void *q, const void *k_cache, const void *v_cache, const void *mask, void *out, int32_t batch, int32_t q_heads,
                      int32_t kv_heads, int32_t head_dim, int32_t q_len, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len,
                      int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, int64_t cache_batch_stride, int64_t cache_head_stride,
                      int64_t cache_pos_stride, int32_t mask_kind, int64_t mask_len, int64_t mask_batch_stride, int64_t mask_row_stride, int32_t causal,
                      float scaling, int32_t act_dtype, void *stream) {
  return qllm_attn_prefill_window(q, k_cache, v_cache, mask, out, batch, q_heads, kv_heads, head_dim, q_len, kv_len, kv_len_dev, max_len, 0, q_batch_stride,
                                  q_head_stride, q_row_stride, cache_batch_stride, cache_head_stride, cache_pos_stride, mask_kind, mask_len, mask_batch_stride,
                                  mask_row_stride, causal, scaling, act_dtype, stream);
}

int qllm_attn_prefill_window(const void *q, const void *k_cache, const void *v_cache, const void *mask, void *out, int32_t batch, int32_t q_heads,
                             int32_t kv_heads, int32_t head_dim, int32_t q_len, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len, int64_t window,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, int64_t cache_batch_stride, int64_t cache_head_stride,
                             int64_t cache_pos_stride, int32_t mask_kind, int64_t mask_len, int64_t mask_batch_stride, int64_t mask_row_stride,
                             int32_t causal, float scaling, int32_t act_dtype, void *stream) {
  clear_error();
  int rc = check_attn_call(q, k_cache, v_cache, out, batch, q_heads, kv_heads, head_dim, &q_len, max_len, window, act_dtype, mask_kind, mask);
  if (rc != QLLM_OK) return rc;
  if (causal != 0 && causal != 1) return set_error(QLLM_ERR_INVALID, "causal must be 0 or 1 (got %d)", causal);
  const int64_t strides[6] = {q_batch_stride, q_head_stride, q_row_stride, cache_batch_stride, cache_head_stride, cache_pos_stride};
  const void *const ptrs[4] = {q, k_cache, v_cache, out};
  rc = check_attn_layout("q / k_cache / v_cache / out", ptrs, 4, kv_len_dev, mask_kind, mask, "batch, head, row and position", strides, 6);
  if (rc != QLLM_OK) return rc;
  if (!kv_len_dev && (kv_len < q_len || kv_len > max_len))
    return set_error(QLLM_ERR_INVALID, "kv_len must lie in q_len..max_len (got kv_len=%lld q_len=%d max_len=%lld)", (long long)kv_len, q_len, (long long)max_len);
  const int64_t need_len = kv_len_dev ? max_len : kv_len;  // the positions a call may reach
  if (mask && (mask_len < need_len || mask_batch_stride < 0 || mask_row_stride < 0))
    return set_error(QLLM_ERR_INVALID, "the mask must cover %lld positions (%s) with non-negative batch and row strides (got mask_len=%lld strides=%lld, %lld)",
                     (long long)need_len, kv_len_dev ? "max_len: the length is on the device" : "kv_len", (long long)mask_len, (long long)mask_batch_stride,
                     (long long)mask_row_stride);
  rc = check_attn_prefill_served(batch, q_heads, kv_heads, head_dim);
  if (rc != QLLM_OK) return rc;
  if (window > 0 && !causal) return set_error(QLLM_ERR_UNSUPPORTED, "attn_prefill serves a sliding window on causal calls only (got window=%lld causal=0)", (long long)window);

  AttnPrefillParams p;
  p.q = q, p.k_cache = k_cache, p.v_cache = v_cache, p.mask = mask, p.out = out;
  p.kv_len_dev = kv_len_dev, p.kv_len = kv_len, p.max_len = max_len, p.window = window;
  p.q_batch = q_batch_stride, p.q_head = q_head_stride, p.q_row = q_row_stride, p.c_batch = cache_batch_stride, p.c_head = cache_head_stride,
  p.c_pos = cache_pos_stride, p.mask_batch = mask_batch_stride, p.mask_row = mask_row_stride;
  p.batch = batch, p.q_heads = q_heads, p.kv_heads = kv_heads, p.q_len = q_len, p.mask_kind = mask_kind, p.causal = causal, p.scaling = scaling;
  return launch_attn_prefill(p, head_dim, act_dtype == QLLM_BF16, (hipStream_t)stream);
}

int qllm_dequant(const qllm_weight_t *w, void *out, int32_t out_dtype, int32_t out_transposed, void *stream) {
  clear_error();
  int rc = validate_weight(w);
  if (rc) return rc;
  if (!out) return set_error(QLLM_ERR_INVALID, "out must not be NULL");
  if (out_dtype != QLLM_F16 && out_dtype != QLLM_BF16) return set_error(QLLM_ERR_INVALID, "out_dtype must be f16 or bf16");
  if (is_native(*w)) return set_error(QLLM_ERR_UNSUPPORTED, "qllm_dequant reads the reference layouts: convert with qllm_unpack_native first");
  return launch_dequant(*w, zero_kind_of(*w), out, out_dtype, out_transposed ? 1 : 0, (hipStream_t)stream);
}

int qllm_ort_gemv(const void *x, const void *qweight, const void *scales, const void *qzeros, const int32_t *g_idx,
                  int32_t groupsize, int32_t bits, int32_t in_features, int32_t add_zero_bias, void *y, int32_t M, int32_t N,
                  int32_t act_dtype, void *workspace, size_t workspace_bytes, void *stream) {
  qllm_weight_t w = {qweight, scales, qzeros, g_idx, nullptr, in_features, N, groupsize, bits, QLLM_LAYOUT_GPTQ, add_zero_bias};
  return qllm_linear_forward(&w, x, y, M, act_dtype, workspace, workspace_bytes, stream);
}

int qllm_ort_dequant(const void *qweight, const void *scales, const void *qzeros, const int32_t *g_idx, int32_t groupsize,
                     int32_t bits, int32_t in_features, int32_t add_zero_bias, void *out_kn, int32_t N, void *stream) {
  qllm_weight_t w = {qweight, scales, qzeros, g_idx, nullptr, in_features, N, groupsize, bits, QLLM_LAYOUT_GPTQ, add_zero_bias};
  return qllm_dequant(&w, out_kn, QLLM_F16, 0, stream);
}

int qllm_awq_gemm_forward(const void *x, const void *qweight, const void *scales, const void *qzeros, int32_t split_k_iters,
                          void *y, int32_t M, int32_t K, int32_t N, int32_t group_size, int32_t act_dtype, void *workspace,
                          size_t workspace_bytes, void *stream) {
  (void)split_k_iters;
  qllm_weight_t w = {qweight, scales, qzeros, nullptr, nullptr, K, N, group_size, 4, QLLM_LAYOUT_AWQ_GEMM, 0};
  return qllm_linear_forward(&w, x, y, M, act_dtype, workspace, workspace_bytes, stream);
}

int qllm_ort_dequantize4bits(const void *qweight, const void *scales, const void *qzeros, int32_t zeros_f16, const int32_t *g_idx,
                             int32_t block_size, int32_t in_features, int32_t out_features, void *out_nk, void *stream) {
  clear_error();
  if (!qweight || !scales || !qzeros || !out_nk) return set_error(QLLM_ERR_INVALID, "qweight / scales / qzeros / out must not be NULL");
  if (in_features <= 0 || out_features <= 0) return set_error(QLLM_ERR_INVALID, "in_features/out_features must be >= 1 (K=%d N=%d)", in_features, out_features);
  if (block_size < 16 || block_size % 16) return set_error(QLLM_ERR_INVALID, "block_size must be a multiple of 16 (got %d)", block_size);
  if (in_features % block_size) return set_error(QLLM_ERR_UNSUPPORTED, "in_features must be a multiple of block_size (K=%d block=%d)", in_features, block_size);
  if ((uintptr_t)qweight % 8 || (uintptr_t)out_nk % 16) return set_error(QLLM_ERR_INVALID, "qweight must be 8-byte and out 16-byte aligned");
  return launch_ort_dequant(qweight, scales, qzeros, zeros_f16 ? 1 : 0, g_idx, block_size, in_features, out_features, out_nk, (hipStream_t)stream);
}

// Which kernel a forward call with these descriptors and M rows (fp16 activations) would run, as text -- no device work.  It asks the
// SAME decision functions the forward entry points execute (decide_single / decide_group, choose_tile, *_split_for) and prints the result.
int qllm_plan_describe(const qllm_weight_t *w, int32_t n_weights, int32_t M, int32_t have_workspace, char *buf, size_t buflen) {
  clear_error();
  if (!w || !buf || buflen < 64) return set_error(QLLM_ERR_INVALID, "w / buf must not be NULL (buf >= 64 bytes)");
  if (int rc = check_layer_count(n_weights, kMaxProblems)) return rc;
  if (M <= 0) return set_error(QLLM_ERR_INVALID, "M must be >= 1 (got %d)", M);
  if (int rc = check_layers(w, n_weights)) return rc;
  const Decision d = n_weights == 1 ? decide_single(&w[0], M, QLLM_F16) : decide_group(w, n_weights, M, QLLM_F16);
  if (d.route == ROUTE_NONE && d.rc == QLLM_ERR_INVALID) return d.rc;  // (layers that cannot share a launch at all: the forward call's own status)
  describe(d, w, n_weights, M, have_workspace ? (size_t)-1 : 0, buf, buflen);
  clear_error();
  return QLLM_OK;
}

int qllm_native_sizes(const qllm_weight_t *src, size_t *qweight_bytes, size_t *scales_bytes, size_t *qzeros_bytes) {
  clear_error();
  if (!src || !qweight_bytes || !scales_bytes || !qzeros_bytes) return set_error(QLLM_ERR_INVALID, "src / outputs must not be NULL");
  if (src->K <= 0 || src->N <= 0 || src->group_size <= 0) return set_error(QLLM_ERR_INVALID, "bad K/N/group_size (%d/%d/%d)", src->K, src->N, src->group_size);
  const bool f16z = src->layout == QLLM_LAYOUT_HQQ || src->layout == QLLM_LAYOUT_NATIVE_F16Z;
  if (int rc = native_shape_ok(src->bits, src->K, src->N, src->group_size, !f16z && src->qzeros)) return rc;
  const size_t G = (size_t)(src->K + src->group_size - 1) / src->group_size;
  *qweight_bytes = (size_t)src->K * src->bits / 32 * src->N * 4;
  *scales_bytes = G * src->N * 2;
  *qzeros_bytes = !src->qzeros ? 0 : (f16z ? G * src->N * 2 : G * (src->N / 16) * 8);
  return QLLM_OK;
}

int qllm_repack_native(const qllm_weight_t *src, void *qweight_out, void *scales_out, void *qzeros_out, void *stream) {
  clear_error();
  int rc = validate_weight(src);
  if (rc) return rc;
  if (is_native(*src)) return set_error(QLLM_ERR_INVALID, "source is already in the native layout");
  if (src->g_idx) return set_error(QLLM_ERR_UNSUPPORTED, "act-order layers: sort the rows by group first (the native layout has contiguous groups)");
  if (src->K % src->group_size != 0) return set_error(QLLM_ERR_UNSUPPORTED, "the native layout needs K %% group_size == 0 (K=%d g=%d)", src->K, src->group_size);
  if ((rc = native_shape_ok(src->bits, src->K, src->N, src->group_size, src->layout != QLLM_LAYOUT_HQQ && src->qzeros))) return rc;
  if (!qweight_out || !scales_out || (src->qzeros && !qzeros_out)) return set_error(QLLM_ERR_INVALID, "output buffers must not be NULL");
  if ((uintptr_t)qweight_out % 16 || (uintptr_t)scales_out % 16 || (uintptr_t)qzeros_out % 8) return set_error(QLLM_ERR_INVALID, "output buffers must be 16-byte (qzeros: 8-byte) aligned");
  return launch_repack_native(*src, zero_kind_of(*src), qweight_out, scales_out, qzeros_out, (hipStream_t)stream);
}

int qllm_unpack_native(const qllm_weight_t *native, int32_t dst_layout, void *qweight_out, void *scales_out, void *qzeros_out, void *stream) {
  clear_error();
  int rc = validate_weight(native);
  if (rc) return rc;
  if (!is_native(*native)) return set_error(QLLM_ERR_INVALID, "source is not in the native layout");
  if (dst_layout < QLLM_LAYOUT_GPTQ || dst_layout > QLLM_LAYOUT_HQQ) return set_error(QLLM_ERR_INVALID, "dst_layout must be GPTQ, AWQ_GEMM or HQQ");
  if ((dst_layout == QLLM_LAYOUT_HQQ) != (native->layout == QLLM_LAYOUT_NATIVE_F16Z))
    return set_error(QLLM_ERR_INVALID, "fp16 zero points <-> HQQ, packed / no zero points <-> GPTQ / AWQ_GEMM");
  if (dst_layout == QLLM_LAYOUT_AWQ_GEMM && (native->bits != 4 || !native->qzeros)) return set_error(QLLM_ERR_INVALID, "AWQ GEMM layout is 4-bit with packed zero points");
  if (!qweight_out || !scales_out || (native->qzeros && !qzeros_out)) return set_error(QLLM_ERR_INVALID, "output buffers must not be NULL");
  return launch_unpack_native(*native, dst_layout, qweight_out, scales_out, qzeros_out, (hipStream_t)stream);
}

int qllm_unpack_qweight(const void *qweight, int32_t layout, int32_t bits, int32_t K, int32_t N, int32_t *q_kn, void *stream) {
  clear_error();
  if (!qweight || !q_kn) return set_error(QLLM_ERR_INVALID, "qweight / q_kn must not be NULL");
  if (bits < 2 || bits > 8 || K <= 0 || N <= 0) return set_error(QLLM_ERR_INVALID, "bad bits/K/N (%d/%d/%d)", bits, K, N);
  if (layout == QLLM_LAYOUT_AWQ_GEMM && (bits != 4 || N % 8)) return set_error(QLLM_ERR_INVALID, "AWQ GEMM layout is 4-bit, N%%8==0");
  if (layout != QLLM_LAYOUT_AWQ_GEMM && (K * bits) % 32) return set_error(QLLM_ERR_INVALID, "K*bits must be a multiple of 32");
  return launch_unpack_qweight(qweight, layout, bits, K, N, q_kn, (hipStream_t)stream);
}

int qllm_pack_qweight(const int32_t *q_kn, int32_t layout, int32_t bits, int32_t K, int32_t N, void *qweight, void *stream) {
  clear_error();
  if (!qweight || !q_kn) return set_error(QLLM_ERR_INVALID, "qweight / q_kn must not be NULL");
  if (bits < 2 || bits > 8 || K <= 0 || N <= 0) return set_error(QLLM_ERR_INVALID, "bad bits/K/N (%d/%d/%d)", bits, K, N);
  if (layout == QLLM_LAYOUT_AWQ_GEMM && (bits != 4 || N % 8)) return set_error(QLLM_ERR_INVALID, "AWQ GEMM layout is 4-bit, N%%8==0");
  if (layout != QLLM_LAYOUT_AWQ_GEMM && (K * bits) % 32) return set_error(QLLM_ERR_INVALID, "K*bits must be a multiple of 32");
  return launch_pack_qweight(q_kn, layout, bits, K, N, qweight, (hipStream_t)stream);
}

}  // extern "C"
