/*
 * qllm_mi355x.h -- C ABI of libqllm_mi355x.so: the MI355X (gfx950 / CDNA4) replacement for the native
 * extensions behind QLLM's quantized-linear forward (fused int4 dequant + matmul).
 *
 * Boundary it replaces (all citations relative to /root/reference):
 *   qllm.ort_ops.gemv        csrc/ort_cuda/ort_ops.cc:94-140   (op_gemv -> dq_gemv.cu gemv<half> / Gemv_g)
 *   qllm.ort_ops.dequant     csrc/ort_cuda/ort_ops.cc:58-92    (dequant_any_bit -> DequantizeAndUnpackWeight*)
 *   qllm.awq_inference_engine.gemm_forward_cuda
 *                            csrc/awq_cuda/quantization/gemm_cuda.h:3-4, gemm_cuda_gen.cu:1102-1161
 *   QuantLinearTorchFunction.forward (+bias) of the three q_layers
 *                            qllm/modeling/q_layers/quant_linear_gptq.py:71-85,136-143
 *                            qllm/modeling/q_layers/quant_linear_hqq.py:31-38,76-80
 *                            qllm/modeling/q_layers/quant_linear_awq.py:142-148
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer on the current HIP device unless noted;
 *     inputs are borrowed, contiguous, row-major; the library never allocates or frees device memory and never
 *     synchronises the host with the device -- every entry point is hipGraph-capturable.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  The reference's default-stream
 *     launches (dq_gemv.cu:166,563; gemm_cuda_gen.cu:1083) are NOT reproduced.
 *   - every function returns a qllm_status_t (0 = ok).  Nothing aborts (contrast dq_gemv.cu:156-159,172-176);
 *     the message for the calling thread's last failure is qllm_last_error().
 *   - weight layouts are exactly the reference's state-dict buffers:
 *       GPTQ     qweight i32 [K*bits/32, N] (column n = little-endian bit stream along K)
 *                qzeros  i32 [ceil(K/g), N*bits/32] (row G = bit stream along N), or NULL => symmetric 2^(bits-1)
 *                scales  f16 [ceil(K/g), N];  g_idx i32 [K] or NULL (NULL = k / group_size)
 *       AWQ_GEMM qweight i32 [K, N/8], nibble i of word (k,j) = q[k, 8j+{0,2,4,6,1,3,5,7}[i]]; qzeros i32 [K/g, N/8]
 *                same interleave; scales f16 [K/g, N]; 4-bit only; no g_idx
 *       HQQ      qweight as GPTQ; qzeros f16 [ceil(K/g), N] (un-packed, non-integer); no g_idx
 *   - numerics, by kernel path (qllm_plan_describe() names the path a call takes):
 *       qllm_dequant / qllm_ort_dequant, the tile GEMMs ("gemm3": the wave-specialised 256x128 kernel, the default from M = 384 /
 *       768; "gemm2": 33 / 65 <= M below that and bf16 activations below 1024 rows; "gemm": ragged N, non-uniform act-order) and the
 *       split-K decode kernel ("skinny"):
 *         W[k,n] = fp16( fp16(s*q) - fp16(z*s) ) exactly as DequantizeLinearBlockWise (quant_linear_gptq.py:38-48) -- one IEEE
 *         rounding per op, bit-identical to the CPU path -- then y = x.W accumulated in fp32, bias added in fp32, one
 *         rounding to the activation dtype (bf16 activations on "gemm3": x is converted to fp16 first and the fp16 result is
 *         rounded to bf16, the arithmetic of the reference's own shim, quant_linear_awq.py:29-36).
 *       the full-K decode kernel ("strip": M <= 32 everywhere, M <= 64 for K <= 4096 and at most 4096 columns; every layout it
 *       serves -- the reference row streams in place and the native strip-major layout; the default decode path):
 *         y = sum_G s_G * ( sum_{k in G} x_k q_k  -  z_G * sum_{k in G} x_k ) evaluated in fp32, i.e. x.W for the UNROUNDED
 *         W = s*(q - z); it differs from the path above by the fp16 rounding noise of W (<= 3e-4 relative measured; the
 *         tests bound every decode case at 2e-3 against float64 of the reference's W and at 1e-2 against the CPU path).
 *     The bit-exactness guarantee therefore holds for the dequant entry points and the paths of the first group only.
 */
#ifndef QLLM_MI355X_H_
#define QLLM_MI355X_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define QLLM_ABI_VERSION 7

typedef enum qllm_status {
  QLLM_OK = 0,
  QLLM_ERR_INVALID = 1,     /* bad shape / null pointer / misalignment (the reference's TORCH_CHECK / invalid_argument) */
  QLLM_ERR_UNSUPPORTED = 2, /* valid request this build has no fused kernel for (caller may use dequant + GEMM) */
  QLLM_ERR_WORKSPACE = 3,   /* workspace NULL or smaller than qllm_workspace_bytes() */
  QLLM_ERR_LAUNCH = 4,      /* HIP launch failure (message carries hipGetErrorString) */
  QLLM_ERR_DEVICE = 5       /* no gfx950 device / wrong architecture */
} qllm_status_t;

typedef enum qllm_layout {
  QLLM_LAYOUT_GPTQ = 0,     /* QuantLinearGPTQ   quant_linear_gptq.py:92-117 */
  QLLM_LAYOUT_AWQ_GEMM = 1, /* WQLinear_GEMM     quant_linear_awq.py:38-68   */
  QLLM_LAYOUT_HQQ = 2,      /* QuantLinearHQQ    quant_linear_hqq.py:47-68   */
  /* the library's own strip-major layout (no reference counterpart; see "native layout" below): built once at load time
   * from any of the three layouts above with qllm_repack_native(), converted back bit-exactly with qllm_unpack_native() */
  QLLM_LAYOUT_NATIVE = 3,      /* packed integer (or no) zero points: from GPTQ / AWQ_GEMM */
  QLLM_LAYOUT_NATIVE_F16Z = 4  /* fp16 zero points: from HQQ */
} qllm_layout_t;

typedef enum qllm_dtype {
  QLLM_F16 = 0,
  QLLM_BF16 = 1,
  /* qllm_linear_forward only (ABI 4): x is fp16 -- bf16 activations the CALLER converted once, e.g. for q/k/v which share their
   * input -- and y is written as bf16(fp16(result)): the reference's own bf16 shim around its fp16 kernels
   * (quant_linear_awq.py:29-36, 144-146) with the conversion of x hoisted out of the call.  Served where the 256x128 prefill
   * kernel serves a bf16 call (the call that would otherwise convert x into the workspace); QLLM_ERR_UNSUPPORTED elsewhere. */
  QLLM_F16_IN_BF16_OUT = 2,
  QLLM_F32 = 3 /* the quantizers' w_dtype only (ABI 7) */
} qllm_dtype_t;

/* elementwise bf16 -> fp16 (round to nearest even), n a multiple of 8: the conversion the QLLM_F16_IN_BF16_OUT caller hoists (ABI 4) */
int qllm_convert_bf16_to_f16(const void *src, void *dst, size_t n, void *stream);

/* One quantized linear layer's buffers: the reference module's state dict, by pointer. */
typedef struct qllm_weight {
  const void *qweight;  /* i32, layout-dependent shape (see above) */
  const void *scales;   /* f16 [ceil(K/g), N] */
  const void *qzeros;   /* i32 packed (GPTQ/AWQ), f16 [ceil(K/g), N] (HQQ), or NULL (GPTQ symmetric) */
  const int32_t *g_idx; /* i32 [K] act-order group map, or NULL for k / group_size (GPTQ only) */
  const void *bias;     /* f16 [N] or NULL */
  int32_t K;            /* in_features  */
  int32_t N;            /* out_features */
  int32_t group_size;   /* > 0 (callers map the reference's -1 to K) */
  int32_t bits;         /* 2..8 (AWQ_GEMM: 4) */
  int32_t layout;       /* qllm_layout_t */
  int32_t add_zero_bias;/* COMPATIBLE_WITH_AUTOGPTQ: stored zero + this, masked (GPTQ packed zeros only) */
} qllm_weight_t;

typedef struct qllm_device_info {
  char arch[32];              /* e.g. "gfx950" (feature suffixes stripped) */
  int32_t compute_units;      /* 256 on MI355X */
  int32_t wavefront_size;     /* 64 */
  int32_t lds_bytes_per_cu;   /* 163840 */
  int32_t clock_khz;
  int64_t hbm_bytes;
} qllm_device_info_t;

/* ---- library ------------------------------------------------------------------------------------------- */
int qllm_abi_version(void);
/* 1 for a lab build of the library (-DQLLM_LAB: the dispatchers' tuning knobs QLLM_* are re-read from the environment at every call),
 * 0 for the release build (knobs are the measured defaults unless set through qllm_set_knob; only QLLM_NUM_CU is read from the environment).  Tools that A/B through the environment
 * assert on it instead of timing the same kernel twice (ABI 5). */
int qllm_is_lab_build(void);
/* Planner thresholds (ABI 6).  The kernel-selection tree was measured on Llama-2-7B / 70B shapes (profiles/r06_shape_table.md has other
 * families); a deployment may move these thresholds without rebuilding.  Process-global, not synchronised with forward calls running on
 * other threads: set them before serving.  Settable names (values outside the range every built kernel covers are refused):
 *   QLLM_STRIP1 0|1|2, QLLM_STRIP1_MAX_M 1..4, QLLM_STRIP1_3BIT 0|1, QLLM_PANEL 0|1, QLLM_PANEL_MIN_M 17..129, QLLM_PANEL_GROUP_MIN_M 17..129, QLLM_GEMM2 0|1, QLLM_GEMM3 0|1,
 *   QLLM_GEMM2_MIN_M >= 33, QLLM_GEMM3_MIN_M >= 0 (0: the measured 384 / 768 line), QLLM_GEMM2_SPLITK 0|1, QLLM_GEMM3_TAIL 0|1, QLLM_GEMM3_BF16 0|1, QLLM_GEMM3_GROUP 0|1,
 *   QLLM_SKINNY_MAX_M 0..64, QLLM_STRIP_MIN >= 0, QLLM_S1_T256_NW16 0|1 (batch 1, K = 6272..8192: 16 waves x 16 k-steps instead of 8 x 32), QLLM_BITGEMV 0|1, QLLM_BITPANEL 0|1, QLLM_BITPANEL_LDS 0|1, QLLM_BITPANEL_MAX_M 17..512 (the last three: qllm_linear_forward_bitpanel, no route),
 *   QLLM_BITGROUP 0|1, QLLM_BITGROUP_MAX_M 0..16 (qllm_linear_forward_bitgroup, no route),
 *   QLLM_BITGEMM 0|1, QLLM_BITGEMM_MIN_M 129..65536 (qllm_linear_forward_bitgemm, no route),
 *   QLLM_GATHER_ROWS 0|1 (qllm_gather_columns, no route; qllm_gather_describe reflects it).
 * qllm_plan_describe() reflects them (it asks the same decision functions the forward calls execute).  QLLM_ERR_INVALID for any other name. */
int qllm_set_knob(const char *name, int32_t value);
int qllm_get_knob(const char *name, int32_t *value, int32_t *is_set);
void qllm_reset_knobs(void);
/* Thread-local, never NULL; "" when the calling thread's last call succeeded. */
const char *qllm_last_error(void);
/* Fills `out` for HIP device `device`; QLLM_ERR_DEVICE if there is none or it is not gfx950. */
int qllm_device_info(int device, qllm_device_info_t *out);

/* ---- workspace ----------------------------------------------------------------------------------------- */
/* Bytes of scratch qllm_linear_forward()/qllm_linear_forward_grouped() need for `w` at M rows (split-K slabs +
 * arrival counters).  The region must be zero-filled once (qllm_workspace_init) before first use; the kernels
 * leave it clean.  One workspace may be shared by calls that are ordered on one stream. */
size_t qllm_workspace_bytes(const qllm_weight_t *w, int32_t M);
/* The same for a known activation dtype: only bf16 calls of the 256x128 prefill kernel need the fp16 staging copy of x
 * (M * K * 2 bytes) that qllm_workspace_bytes() has to assume.  (ABI 4) */
size_t qllm_workspace_bytes_act(const qllm_weight_t *w, int32_t M, int32_t act_dtype);
int qllm_workspace_init(void *workspace, size_t bytes, void *stream);

/* ---- the hot path -------------------------------------------------------------------------------------- */
/* y[M,N] = x[M,K] . dequant(w) (+ bias).  x, y in `act_dtype`; scales/bias stay f16 (bf16 activations are
 * converted on load, replacing the reference's bf16->f16 shims, ort_ops.cc:119-138, quant_linear_awq.py:29-36).
 * Dispatch: M <= 32 (<= 64 on small shapes) -> weight-streaming MFMA matvec (HBM-bound); native 4-bit layers at 17 <= M <= 128 ->
 * the panel kernel (activation tiles shared through LDS, weight fragments from registers); larger M -> LDS-tiled MFMA GEMM
 * (qllm_plan_describe names the kernel; profiles/r03_mid_m.md, r04_mid_m.md hold the measurements behind the lines).
 * Fused widths: 4 bits everywhere; 3 bits (GPTQ / HQQ row stream; fp16, symmetric or packed zero points) for M <= 64 and, with
 * K % 64 == 0, N % 128 == 0 and fp16 activations, for every larger M; every other width / shape returns QLLM_ERR_UNSUPPORTED and the
 * caller takes the reference's own two-step branch (qllm_dequant + a dense GEMM, quant_linear_gptq.py:81-85).
 * Native 4-bit layers at M > 64 need K % 64 == 0 and a power-of-two group size; N % 128 == 0, or (round 7, Falcon-7B's 4544 / 4672)
 * N % 128 == 64 on single layers: the prefill kernel's last column tile is then half wide (plan string " n_tail=64"), split over K
 * where the tiles leave CUs idle -- qllm_workspace_bytes covers those splits.  At batch 1 the native 4-bit layers with 64-wide groups
 * take K % 128 == 64 too (the batch-1 kernel); the fused all-reduce entry keeps to 128-wide groups.
 * Replaces QuantLinearTorchFunction.forward + bias for all three layouts. */
int qllm_linear_forward(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype,
                        void *workspace, size_t workspace_bytes, void *stream);

/* n_weights layers that share the SAME input x (q/k/v, gate/up) in ONE launch: y[i] = x . dequant(w[i]).
 * `w` and `y` are HOST arrays of length n_weights (<= 8); all w[i] must agree on K, bits, layout family and
 * group_size.  Decode and mid-batch sizes: M <= 32 (<= 64 for narrow groups) on the strip kernels; native 4-bit layers (N % 64 == 0,
 * K % 64 == 0, group size 32 to 64 rows / 64 / 128) up to M = 128 in one launch of the panel kernel, split-K partials in the
 * workspace.  Prefill sizes (ABI 6, round 6): from 384 rows, 2..4 four-bit
 * layers of one storage kind (row-stream or strip-major; not AWQ words in place), N % 128 == 0, K % 64 == 0, at least one 256x128 tile
 * per CU over the group, run as ONE grid of the prefill kernel (bf16 natively).  When the group's tiles do not fill whole rounds of CUs the
 * last round is split over K: that needs kCounter (16 KB) + tail_tiles x split x 128 KB of workspace -- at most 16 KB + 128 KB per CU
 * (16 KB + 32 MB on 256 CUs); with less the launch simply does not split.  QLLM_ERR_UNSUPPORTED otherwise: call layer by layer.
 * Workspace for a group: the sum of qllm_workspace_bytes_act() over its layers (n_weights x the widest layer's covers it too), and
 * from 384 rows at least 16 KB + 128 KB per CU -- the group's tail split counts the tiles of all its layers, which no layer's size bounds. */
int qllm_linear_forward_grouped(const qllm_weight_t *w, void *const *y, int32_t n_weights, const void *x,
                                int32_t M, int32_t act_dtype, void *workspace, size_t workspace_bytes,
                                void *stream);

/* Diagnostics (process-global, not thread-safe; NULL switches it off): the next native-layout decode launches (4 bits, g128: the
 * batch-1 "lds-slab" form and the batch 2..32 "dma-A" form) each take one 192-byte slot of `buf` (device memory, n_slots x 24 x
 * u64, in launch order) and record 100 MHz device timestamps of wave 0 of their first, middle and last block: [entry, loads issued
 * (dma-A: ring requested), x staged (dma-A: first stage landed), rounds done, after the block barrier, exit, -, -] x 3.  A launch
 * captured into a hipGraph keeps its slot.  tools/lab/cbench.cpp --timeline [--m 16]. */
int qllm_debug_timeline(void *buf, int32_t n_slots);

/* W[K,N] (out_transposed = 0) or W[N,K] (out_transposed = 1) in `out_dtype`, bit-identical to
 * DequantizeLinearBlockWise / DequantAndUnpack / unpack().  All bits 2..8, all layouts, optional g_idx.
 * Replaces ort_ops.dequant (ort_ops.cc:58-92). */
int qllm_dequant(const qllm_weight_t *w, void *out, int32_t out_dtype, int32_t out_transposed, void *stream);

/* ---- reference-named entry points (flat signatures mirroring the pybind functions) ---------------------- */
/* ort_ops.gemv(x, qweight, scales, qzeros, g_idx, groupsize, bits, in_features, add_zero_bias) -> y[M,N]
 * (ort_ops.cc:94-98).  The reference restricts this to M <= 8 and 4 bits at the call site
 * (quant_linear_gptq.py:76-80); here any M dispatches like qllm_linear_forward. */
int qllm_ort_gemv(const void *x, const void *qweight, const void *scales, const void *qzeros,
                  const int32_t *g_idx, int32_t groupsize, int32_t bits, int32_t in_features,
                  int32_t add_zero_bias, void *y, int32_t M, int32_t N, int32_t act_dtype, void *workspace,
                  size_t workspace_bytes, void *stream);

/* ort_ops.dequant(qweight, scales, qzeros, g_idx, groupsize, bits, in_features, add_zero_bias) -> W[K,N] f16
 * (ort_ops.cc:58-63). */
int qllm_ort_dequant(const void *qweight, const void *scales, const void *qzeros, const int32_t *g_idx,
                     int32_t groupsize, int32_t bits, int32_t in_features, int32_t add_zero_bias, void *out_kn,
                     int32_t N, void *stream);

/* ort_ops.Dequantize4Bits(qweight u8 [N, K/block, block/2], scales [N*K/block], qzeros, g_idx, block_size, in_features,
 * out_features) -> W[N,K] f16 (ort_ops.cc:161-197; kernels dq.cu:79-245): the ORT / MatMulNBits blob layout that
 * QuantLinearORT stores (quant_linear_onnxruntime.py:85-153).  `qzeros` is either packed u8 (two 4-bit zero points per
 * byte, ceil(K/block / 2) bytes per row; zeros_f16 = 0) or fp16 [N, K/block] (zeros_f16 = 1); `g_idx` (NULL unless the
 * layer is act-order) maps each input channel to its block.  Needs block_size % 16 == 0 and in_features % block_size == 0.
 * Numerics follow the reference's Python path: fp16((q - z) * s), with the difference rounded to fp16 first when the
 * zero points are fp16. */
int qllm_ort_dequantize4bits(const void *qweight, const void *scales, const void *qzeros, int32_t zeros_f16,
                             const int32_t *g_idx, int32_t block_size, int32_t in_features, int32_t out_features,
                             void *out_nk, void *stream);

/* awq_inference_engine.gemm_forward_cuda(x[M,K], qweight[K,N/8], scales[K/g,N], qzeros[K/g,N/8], split_k_iters)
 * -> y[M,N] (gemm_cuda.h:3-4).  `split_k_iters` is accepted for signature parity and ignored: the reduction
 * over K is carried in fp32, never as the reference's fp16 partial sums (gemm_cuda_gen.cu:1115,1160). */
int qllm_awq_gemm_forward(const void *x, const void *qweight, const void *scales, const void *qzeros,
                          int32_t split_k_iters, void *y, int32_t M, int32_t K, int32_t N, int32_t group_size,
                          int32_t act_dtype, void *workspace, size_t workspace_bytes, void *stream);

/* Diagnostics: which kernel a forward call with these descriptors (1 = qllm_linear_forward, > 1 = the grouped call) and M
 * rows would run, written as text into buf ("strip ...", "skinny ...", "gemm2 ...", "gemm ...", "unsupported ...").  Pure host
 * code -- pointers are only tested for NULL / alignment, never dereferenced -- so the dispatch table can be checked without a
 * GPU.  No reference counterpart. */
int qllm_plan_describe(const qllm_weight_t *w, int32_t n_weights, int32_t M, int32_t have_workspace, char *buf,
                       size_t buflen);

/* ---- native layout ------------------------------------------------------------------------------------------ */
/* The reference's layouts are shaped for ITS kernels: GPTQ / HQQ store [K*bits/32][N] words (a 16-column strip of a layer is
 * K/8 separate 64-byte segments), AWQ stores [K][N/8] words (a row is N/2 bytes).  A batch-1 matvec on MI355X is fastest when
 * every workgroup streams ONE contiguous region (tools/lab/memlab2.hip: one Llama-2-7B decoder layer's four launches read
 * 25.96 us in the row-stream forms, 21.45 us strip-major), so the library has a layout of its own, built once at load time:
 *     qweight i32 [N/16][K*bits/32][16]   word (s, r, i) = GPTQ word (r, 16 s + i)
 *     scales  f16 [N/16][G][16]           G = K / group_size
 *     qzeros  NATIVE:      i32 [N/16][G][2]  4 bits: nibble e of word j = stored zero point of column 16 s + 8 j + e;
 *                                            3 bits: column 16 s + i at bit 3 i of the 64-bit little-endian pair;  or NULL
 *             NATIVE_F16Z: f16 [N/16][G][16]
 *     bias f16 [N] (natural order); g_idx must be NULL (act-order layers: sort the rows by group first, qllm_gather_columns)
 * Shapes: bits 3 or 4, K % 32 == 0, N % 16 == 0 (3-bit packed zero points: N % 32 == 0), group_size % 32 == 0, K % group_size == 0.
 * A descriptor with layout = QLLM_LAYOUT_NATIVE[_F16Z] is accepted by qllm_linear_forward / _grouped (M <= 64 with group size
 * 64 / 128, and -- 4 bits -- 32; larger M: see qllm_plan_describe); qllm_dequant reads the reference layouts only (QLLM_ERR_UNSUPPORTED: convert
 * back with qllm_unpack_native first).  Pure integer permutations: repack then unpack is the identity.  Counterpart in the reference: the load-time repacks of its own kernel formats (quant_linear_awq.py:95-140). */
int qllm_native_sizes(const qllm_weight_t *src, size_t *qweight_bytes, size_t *scales_bytes, size_t *qzeros_bytes);
int qllm_repack_native(const qllm_weight_t *src, void *qweight_out, void *scales_out, void *qzeros_out, void *stream);
/* dst_layout: QLLM_LAYOUT_GPTQ / _AWQ_GEMM (from NATIVE) or QLLM_LAYOUT_HQQ (from NATIVE_F16Z); outputs are the reference's buffers */
int qllm_unpack_native(const qllm_weight_t *native, int32_t dst_layout, void *qweight_out, void *scales_out, void *qzeros_out,
                       void *stream);

/* ---- layout conversion on device (repack) ----------------------------------- */
/* Integer grid q[K,N] (i32, natural order) <-> packed qweight of `layout`/`bits`.
 * Replaces general_pack_on_row / general_unpack_on_row (+ AWQ reorder) (compress_weight.py:46-92,
 * quant_linear_awq.py:95-140). */
int qllm_unpack_qweight(const void *qweight, int32_t layout, int32_t bits, int32_t K, int32_t N, int32_t *q_kn,
                        void *stream);
int qllm_pack_qweight(const int32_t *q_kn, int32_t layout, int32_t bits, int32_t K, int32_t N, void *qweight,
                      void *stream);

/* out[m, k] = x[m, perm[k]] for a row-major [M, K] matrix of 2-byte activations (fp16 or bf16; act_dtype only names the
 * element size).  The act-order helper: the reference's kernels index scales[g_idx[k]] per weight row
 * (quant_linear_gptq.py:38-43, ort_ops gemv/dequant with g_idx); this library serves act-order layers from a copy whose rows
 * are sorted by group (perm = argsort(g_idx), built at load with qllm_unpack_qweight / qllm_pack_qweight), which needs the same
 * permutation applied to the columns of x at every forward.  perm: K int32 on the device, a permutation of 0..K-1 (entries are
 * not range-checked).  x, perm, out 16-byte aligned, out must not alias x; K % 8 == 0 and K <= 28672, else QLLM_ERR_UNSUPPORTED. */
int qllm_gather_columns(const void *x, const int32_t *perm, void *out, int32_t M, int32_t K, int32_t act_dtype, void *stream);
/* The launch qllm_gather_columns makes for M rows of K columns, as text in buf: "gather rows=2 cpt=4 grid=33 lds=57344" (the kernel that
 * stages `rows` rows per step, `cpt` 8-column chunks per thread) or "gather columns chunks=4 parts=2 rows_per_block=2 grid=32x2 lds=44032"
 * (the row-at-a-time kernel); "unsupported (...)" for a K the entry refuses, "gather nothing (M=0)" for no rows.  Pure host code, the rule
 * the launcher itself executes: a function of M, K, the device's CU count (256 without a device) and the knob QLLM_GATHER_ROWS 0|1
 * (qllm_set_knob; 0: every M on the row-at-a-time kernel).  QLLM_ERR_INVALID: NULL or empty buf, M < 0, K < 1.
 * ABI: the symbol is ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged): probe for it by symbol. */
int qllm_gather_describe(int32_t M, int32_t K, char *buf, size_t buflen);

/* y[M,N] = x[:, perm_k] . dequant(w) (+ bias): qllm_gather_columns and qllm_linear_forward in ONE launch, for the layers the bit-stream
 * matvec serves (csrc/bitgemv_ao.hip: the gather happens while the kernel stages x in LDS; no gathered copy of x is written).  The
 * act-order entry for the widths without a strip kernel: w describes the row-sorted copy of an act-order layer (a PLAIN descriptor,
 * g_idx NULL, the layer's own scales / qzeros / bias), perm_k = argsort(g_idx).  The result is bit-identical to qllm_linear_forward on
 * a qllm_gather_columns copy of x.
 * When to use it: every column block gathers x for itself, so the saved launch pays at M <= 2 (0.2-2 us faster than the two calls on
 * Llama-2-7B shapes) and the two calls are faster from about M = 4 on (profiles/bitgemv_actorder.md).
 * Served: exactly the calls qllm_linear_forward hands to that matvec -- GPTQ / HQQ row-stream layouts, bits 2..8, K % 32 == 0,
 * group_size % 32 == 0, 1 <= M <= 16, QLLM_BITGEMV not switched off; everything else is QLLM_ERR_UNSUPPORTED (gather with
 * qllm_gather_columns and call qllm_linear_forward, or qllm_dequant + a GEMM).  w->g_idx set, a NULL or not 16-byte aligned perm_k,
 * NULL x / y: QLLM_ERR_INVALID.  Every error is raised before any device work.
 * perm_k: K int32 on the device, a permutation of 0..K-1.  Every entry is clamped to 0..K-1 before it is used: an array that is not
 * a permutation gives a wrong result, never an access outside x.
 * Workspace: qllm_workspace_bytes_act(w, M, act_dtype) (the matvec's slabs and counters); NULL: no K split.  No host
 * synchronisation; hipGraph-capturable.  No reference counterpart (the reference's act-order kernels index scales[g_idx[k]]). */
int qllm_linear_forward_permuted(const qllm_weight_t *w, const int32_t *perm_k, const void *x, void *y, int32_t M, int32_t act_dtype,
                                 void *workspace, size_t workspace_bytes, void *stream);

/* y[M,N] = x[M,K] . dequant(w) (+ bias) for MID-BATCH calls, 17 <= M <= 512, on the row-stream layouts read in place, at every width
 * from 2 to 8 bits (csrc/bitpanel.hip: 64-column panels x up to 128 rows per block on v_mfma_f32_16x16x32_f16, x tiles shared through
 * LDS, weight fragments built in registers from the packed words, split-K through the workspace).  An ADDITIVE entry: the planner
 * does not know it -- qllm_linear_forward and qllm_plan_describe answer these calls as before ("unsupported (no fused kernel ...)"
 * for 2 / 5 / 6 / 7 / 8 bits above 16 rows), and a caller that used to take qllm_dequant + a dense GEMM there (2 K N bytes of fp16 W
 * written and read back) may call this instead.  It also serves the in-place 3- / 4-bit layers the planner refuses (ragged N).
 * Served: GPTQ / HQQ layouts, bits 2..8, K % 32 == 0, group_size % 32 == 0, any N >= 1 (HQQ: even N, 4-byte aligned zeros); packed
 * (with add_zero_bias), NULL (symmetric) or fp16 zero points; optional bias; fp16 or bf16 activations (bf16 is converted to fp16 while
 * x is staged, y is bf16: what the bit-stream matvec does); packed words below 2 GiB, 512 x K activations below 1 GiB.
 * QLLM_ERR_UNSUPPORTED: M < 17 (qllm_linear_forward serves those), M > 512, another layout, shape or alignment, QLLM_BITPANEL = 0 --
 * the message names the alternative (qllm_dequant + a GEMM).  QLLM_ERR_INVALID: NULL x / y, w->g_idx set (act-order: call it on the
 * row-sorted copy with a qllm_gather_columns copy of x).  Every error is raised before any device work.
 * Numerics: the strips' unrounded-W contract -- exact integers q - z (fp16 zero points: the reference's one fp16 rounding of q - z)
 * into the matrix cores, one fp32 y += s_g * acc_g per group, y rounded once; deterministic with and without a split.
 * Workspace: qllm_bitpanel_workspace_bytes(w, M) = the 16 KB counter page every route shares (qllm_workspace_init; left zero after
 * every call) + the fp32 partial panels of the split.  NULL, misaligned (256 bytes) or too small: no K split, the call is still
 * served.  No host synchronisation; hipGraph-capturable.  Not built: a grouped (sibling) form of THIS kernel (the decode sizes have one:
 * qllm_linear_forward_bitgroup below).  M > 512: qllm_linear_forward_bitgemm below (129 rows and up).
 * Knobs (qllm_set_knob): QLLM_BITPANEL 0|1; QLLM_BITPANEL_LDS 0|1 picks the kernel's ingest of the packed words (0, the default: straight
 * into registers; 1: staged through LDS; same bits either way, A/B in profiles/bitpanel.md); QLLM_BITPANEL_MAX_M 17..512 is read by CALLERS that route by row count (the Python
 * modules: the largest row count they send here) -- the entry itself always takes up to 512 rows.  QLLM_BITPANEL_MAX_M_DEFAULT is what
 * such callers use while the knob is unset (0 would mean they do not call the entry at all): the largest measured row count at which
 * the entry is at least 5 % faster than qllm_dequant + a dense GEMM on every shape and width of profiles/bitpanel.md (256: 1.07x at
 * worst; at 512 rows it loses on 4096 x 11008 layers, 0.79-0.86x).
 * ABI: the three symbols are ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged, as for qllm_linear_forward_permuted and the
 * quantizer entries before them): an integrator that may meet an older library of the same ABI number probes for them by symbol.
 * Replaces, for these calls, the dequantise-then-matmul forward of quant_linear_gptq.py:81-85. */
#define QLLM_BITPANEL_MAX_M_DEFAULT 256
int qllm_linear_forward_bitpanel(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *workspace,
                                 size_t workspace_bytes, void *stream);
size_t qllm_bitpanel_workspace_bytes(const qllm_weight_t *w, int32_t M);
/* The geometry that call would launch, as text: "bitpanel bits=5 cols=64 row_tiles=4 row_blocks=1 split_k=4", or "unsupported (...)".
 * Pure host code (pointers are tested for NULL / alignment only); have_workspace = 0: the call without a workspace (no split). */
int qllm_bitpanel_describe(const qllm_weight_t *w, int32_t M, int32_t have_workspace, char *buf, size_t buflen);

/* y[M,N] = x[M,K] . dequant(w) (+ bias) for PREFILL calls, M >= 129, on the row-stream layouts read in place, at every width from 2 to
 * 8 bits (csrc/bitgemm.hip: the 256 x 128 x 64 tile of the 3- / 4-bit prefill kernel -- eight matrix waves on v_mfma_f32_32x32x16_f16
 * fed by LDS-DMA, four dequant waves that each own one column and one 32-k unit = `bits` word rows -- with split-K through the
 * workspace).  An ADDITIVE entry: the planner does not know it -- qllm_linear_forward, qllm_plan_describe and qllm_workspace_bytes*
 * answer as before -- and a caller that used to take qllm_dequant + a dense GEMM above qllm_linear_forward_bitpanel's rows (2 K N bytes
 * of fp16 W written and read back on every call) may call this instead.  It also serves the in-place 3- / 4-bit layers whose N is no
 * multiple of 128.
 * Served: GPTQ / HQQ layouts, bits 2..8, M >= 129, K % 64 == 0, group_size % 32 == 0 (any such size: group_size == K and a ragged last
 * group included), N % 8 == 0; packed (with add_zero_bias), NULL (symmetric) or fp16 zero points; optional bias; act_dtype QLLM_F16
 * (fp16 x, fp16 y) or QLLM_F16_IN_BF16_OUT (fp16 x -- a bf16 caller converts once, qllm_convert_bf16_to_f16 -- and bf16 y rounded
 * fp32 -> fp16 -> bf16, as the 4-bit prefill kernel does); x and y 16-byte aligned; M K 2 and K N bits / 8 below 2 GiB.
 * QLLM_ERR_UNSUPPORTED: M < 129 (qllm_linear_forward_bitpanel / qllm_linear_forward serve those), QLLM_BF16 ("convert x to fp16, pass
 * QLLM_F16_IN_BF16_OUT"), another layout, shape or alignment, QLLM_BITGEMM = 0 -- the message names the alternative.
 * QLLM_ERR_INVALID: NULL x / y, w->g_idx set (act-order: call it on the row-sorted copy with a qllm_gather_columns copy of x), bits
 * outside 2..8.  Every error is raised before any device work.
 * Numerics: the prefill kernel's fp16 contract, not the strips' -- the B tile holds fp16(q s) - fp16(z s), bit for bit what
 * qllm_dequant writes; fp32 sums; y rounded once; deterministic with and without a split.
 * Workspace: qllm_bitgemm_workspace_bytes(w, M) = the 16 KB counter page every route shares (left zero after every call) + tiles x S
 * fp32 partial tiles of 256 x 128.  S is the largest power of two <= 8 with tiles x S <= CUs and at least 8 k-tiles (of 64) per block.
 * NULL, misaligned (256 bytes) or too small: S = 1, the call is still served.  No host synchronisation; hipGraph-capturable.
 * Not built: a grouped (sibling) form, native bf16 MFMA, K % 64 != 0, N % 8 != 0, the AWQ layout.
 * Knobs (qllm_set_knob): QLLM_BITGEMM 0|1; QLLM_BITGEMM_MIN_M 129..65536 is read by CALLERS that route by row count (the Python modules:
 * the fewest rows they send here, above QLLM_BITPANEL_MAX_M) -- the entry itself always takes M >= 129.  QLLM_BITGEMM_MIN_M_DEFAULT is
 * what such callers use while the knob is unset; 0 means they do not call the entry at all.  The rule (profiles/bitgemm.md): the
 * smallest measured M >= 257 from which the entry is at least 5 % faster than qllm_dequant + a dense GEMM on every shape and width,
 * at that M and every larger measured one; 0 if there is none or while the table is not measured.  Measured: 1.27x at worst from 257 to
 * 2048 rows, 0.93-1.20x at 4096 -- no such M, hence 0; a deployment whose calls stay below about 2048 rows sets the knob to 257.
 * ABI: the three symbols are ADDITIVE within ABI 7, like the bitpanel symbols.
 * Replaces, for these calls, the dequantise-then-matmul forward of quant_linear_gptq.py:81-85. */
#define QLLM_BITGEMM_MIN_M_DEFAULT 0
int qllm_linear_forward_bitgemm(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *workspace,
                                size_t workspace_bytes, void *stream);
size_t qllm_bitgemm_workspace_bytes(const qllm_weight_t *w, int32_t M);
/* The geometry that call would launch, as text: "bitgemm bits=8 tile=256x128 tiles=64 split_k=4", or "unsupported (...)".
 * Pure host code (pointers are tested for NULL / alignment only); have_workspace = 0: the call without a workspace (no split). */
int qllm_bitgemm_describe(const qllm_weight_t *w, int32_t M, int32_t have_workspace, char *buf, size_t buflen);

/* y_i[M,N_i] = x[M,K] . dequant(w_i) (+ bias_i) for 1..4 layers that read the SAME activations (q/k/v, gate/up) at DECODE sizes,
 * 1 <= M <= 16, in ONE launch of the bit-stream matvec (csrc/bitgemv_group.hip: the kernel body of csrc/bitgemv.hip; the members' blocks
 * follow one another, widest member first).  The grouped form of the widths qllm_linear_forward_grouped refuses -- 2, 5, 6, 7, 8 bits
 * (3 / 4-bit row-stream layers are taken too).  An ADDITIVE entry: the planner does not know it -- qllm_linear_forward_grouped,
 * qllm_plan_describe and qllm_workspace_bytes* answer as before.  n_weights == 1 is a plain qllm_linear_forward.
 * The contract: y_i is BIT-IDENTICAL to qllm_linear_forward(&w[i], x, ...) called with that layer's own workspace.  Every member keeps
 * the K split of its own single launch and has its own counter and slab range of the one workspace; the group is not split as one wide
 * layer.  Results never depend on which layers were grouped.
 * Served: every member a call qllm_linear_forward hands to that matvec (GPTQ / HQQ layouts, bits 2..8, K % 32 == 0, group_size % 32 ==
 * 0, HQQ: even N); packed (with add_zero_bias), NULL or fp16 zero points and the bias may differ per member; fp16 or bf16 activations.
 * QLLM_ERR_INVALID: NULL x / y[i], n_weights outside 1..4, members that disagree on K, bits, group size, layout family or add_zero_bias,
 * a g_idx.  QLLM_ERR_UNSUPPORTED: M > 16, another layout or shape, QLLM_BITGROUP = 0 -- the message names the alternative
 * (qllm_linear_forward layer by layer).  Every error is raised before any device work.
 * Workspace: qllm_bitgroup_workspace_bytes(w, n_weights, M) = the 16 KB counter page every route shares (qllm_workspace_init; left zero
 * after every call) + sum_i split_i M N_i 4 bytes of fp32 slabs.  NULL, misaligned (256 bytes), too small for ALL members' slabs, or
 * more than 4096 column blocks of 32 in the group: NO member splits -- the call is still served and equals the single calls made
 * without a workspace.  No host synchronisation; hipGraph-capturable.  Not built: act-order members, groups mixing widths.
 * Knobs (qllm_set_knob): QLLM_BITGROUP 0|1; QLLM_BITGROUP_MAX_M 0..16 is read by CALLERS that route by row count (the Python modules'
 * sibling groups: the largest row count they send here, 0: never) -- the entry itself always takes up to 16 rows.
 * QLLM_BITGROUP_MAX_M_DEFAULT is what such callers use while the knob is unset: the largest row count up to which the grouped launch was
 * not slower than the member launches, by more than the spread of repeated measurements, in any cell of profiles/bitgemv_group.md.
 * ABI: three ADDITIVE symbols within ABI 7: probe for them by symbol.  No reference counterpart (the reference runs one module per
 * nn.Linear, qllm/utils/modelutils.py:161-181). */
#define QLLM_BITGROUP_MAX_M_DEFAULT 16
int qllm_linear_forward_bitgroup(const qllm_weight_t *w, void *const *y, int32_t n_weights, const void *x, int32_t M, int32_t act_dtype,
                                 void *workspace, size_t workspace_bytes, void *stream);
size_t qllm_bitgroup_workspace_bytes(const qllm_weight_t *w, int32_t n_weights, int32_t M);
/* The geometry that call would launch, as text: "bitgroup bits=8 cols=32 layers=3 blocks=520 split_k=4,4,4" (split_k in the caller's
 * order), or "unsupported (...)".  Pure host code; have_workspace = 0: the call without a workspace (no member splits). */
int qllm_bitgroup_describe(const qllm_weight_t *w, int32_t n_weights, int32_t M, int32_t have_workspace, char *buf, size_t buflen);

/* y[M,N] = act(gate)[M,K] * up[M,K] . dequant(w) (+ bias): the down-projection of a SwiGLU MLP with the elementwise product
 * act_fn(gate_proj(x)) * up_proj(x) formed INSIDE the linear launch (csrc/strip1_swiglu.hip: the SWIGLU forms of the batch-1 kernel,
 * csrc/strip1_kernel.hpp).  The kernel routes every element of its input through registers on the way to LDS; the staging pass loads
 * the matching chunk of `up` in the same batch, computes s = g / (1 + expf(-g)) in fp32, rounds s to act_dtype, multiplies by u in fp32
 * and rounds again -- the two roundings of the eager expression -- and goes on as the plain kernel: the launch returns BIT FOR BIT what
 * qllm_linear_forward returns on x = act(gate) * up rounded that way, one dependent launch and one [M, K] round trip less.
 * `act`: QLLM_ACT_SILU.  gate / up: contiguous [M, K] of act_dtype (QLLM_F16 / QLLM_BF16), 16-byte aligned; y as for
 * qllm_linear_forward, and it must not alias gate or up.
 * Served: exactly the calls qllm_linear_forward runs on the batch-1 kernel ("strip1 ..." in qllm_plan_describe), with the same waves x
 * round -- native-layout layers (NATIVE, NATIVE_F16Z); M = 1: 4 bits with 128- or 64-wide groups, and 3 bits; M = 2..4: 4 bits,
 * 128-wide groups, K <= 16384.  QLLM_ERR_UNSUPPORTED for everything else -- other layouts, act-order, other widths, M >= 5, a
 * QLLM_STRIP1* knob that takes the shape off that kernel, another `act` -- and the caller runs the activation and
 * qllm_linear_forward as before.  QLLM_ERR_INVALID: NULL / misaligned pointers, M < 1, y aliasing an input.  Every error is raised
 * before any device work.  No workspace, no host synchronisation; hipGraph-capturable.  Not built: GELU gates, the fused all-reduce
 * form, a norm in front (a residual behind: qllm_linear_forward_residual below).
 * ABI: the two symbols are ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged, as for the bitpanel / bitgroup symbols): probe for them
 * by symbol.  The reference's counterpart was its fused_mlp / QuantLlamaMLP (import left commented out in
 * qllm/modeling/q_layers/__init__.py:4). */
#define QLLM_ACT_SILU 0
int qllm_linear_forward_swiglu(const qllm_weight_t *w, const void *gate, const void *up, void *y, int32_t M, int32_t act_dtype, int32_t act,
                               void *stream);
/* What that call (act = QLLM_ACT_SILU) would launch, as text: "swiglu " followed by the plan line of the plain call ("swiglu strip1 nw=15
 * round=24 grid=strips x 1 layout=strip-major"), or "refused: " and the refusal text.  Pure host code. */
int qllm_swiglu_describe(const qllm_weight_t *w, int32_t M, char *buf, size_t buflen);

/* ---- RMSNorm: standalone, and fused into the launch of the layers it feeds ------------------------------------------------------------ */
/* y[M,K] = weight[K] * round(x[M,K] * rstd), rstd = rsqrt(mean(x^2) + eps) per row: the RMSNorm of the Llama family as ONE kernel
 * (csrc/rmsnorm.hip: one block per row, 16-byte loads, the row kept in registers between the reduction and the output), with the eager
 * LlamaRMSNorm's arithmetic step by step: squares and their sum in fp32 (an fp16 / bf16 square is exact in fp32), rstd in fp32,
 * h = x * rstd rounded to act_dtype, y = weight * h in fp32 rounded to act_dtype.  The order of the sum depends on K only: results are
 * deterministic.  x / y: contiguous [M, K] of act_dtype (QLLM_F16 / QLLM_BF16); weight: [K] of the same type; all three 16-byte
 * aligned; K % 8 == 0, K <= 65536 (QLLM_ERR_UNSUPPORTED above); any M >= 1; y may alias x.  rstd_out: [M] floats, or NULL.
 * QLLM_ERR_INVALID for NULL / misaligned pointers, M < 1, K % 8 != 0 -- before any device work.  hipGraph-capturable.
 * The reference's counterpart is TritonLlamaRMSNorm (qllm/modeling/q_layers/triton_norm.py). */
int qllm_rmsnorm(const void *x, const void *weight, void *y, int32_t M, int32_t K, float eps, int32_t act_dtype, float *rstd_out, void *stream);
/* y_i[1,N_i] = RMSNorm(x)[1,K] . dequant(w_i) (+ bias_i) for the n_weights layers that share x (q/k/v, gate/up), with the norm formed
 * INSIDE the grouped launch (csrc/strip1_norm.hip: the NORM forms of the batch-1 kernel, csrc/strip1_kernel.hpp).  The waves of a block
 * together stage all of x; each sums the fp32 squares of the elements it owns, one barrier and NW partials later every wave of every
 * block holds the same rstd bit for bit, and each chunk is rewritten in registers as norm_weight * round(x * rstd) -- the two roundings
 * above -- before the plain kernel's code goes on.  Contract: the launch returns BIT FOR BIT what qllm_linear_forward_grouped returns on
 * xn = norm_weight * (x.float() * rstd).to(dtype), with rstd the value it reports in rstd_out ([M] floats written by one block, or NULL).
 * Its order of summation is not qllm_rmsnorm's: the two may differ in rare last-bit roundings of xn.
 * Served: exactly the M = 1 calls qllm_linear_forward(_grouped) runs on the batch-1 kernel ("strip1 ..." in qllm_plan_describe) for
 * native-layout layers (NATIVE, NATIVE_F16Z) -- 4 bits with 128- or 64-wide groups, and 3 bits -- with the same waves x round.
 * QLLM_ERR_UNSUPPORTED for everything else (M >= 2: the four-row forms are not built; other layouts and widths; members that disagree
 * on K / group_size / bits; a QLLM_STRIP1* knob that takes the shape off that kernel): run qllm_rmsnorm and the plain call.
 * QLLM_ERR_INVALID: NULL / misaligned pointers, M < 1, a y aliasing x or norm_weight.  Every error is raised before any device work.  No
 * workspace, no host synchronisation; hipGraph-capturable.
 * ABI: the three symbols are ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged, as for the SwiGLU symbols): probe for them by symbol. */
int qllm_linear_forward_rmsnorm(const qllm_weight_t *w, void *const *y, int32_t n_weights, const void *x, const void *norm_weight, float eps,
                                int32_t M, int32_t act_dtype, float *rstd_out, void *stream);
/* What that call would launch, as text: "rmsnorm " followed by the plan line of the plain grouped call ("rmsnorm strip1 nw=8 round=16
 * exact grid=strips x 3 layout=strip-major"), or "refused: " and the refusal text.  Pure host code. */
int qllm_rmsnorm_describe(const qllm_weight_t *w, int32_t n_weights, int32_t M, char *buf, size_t buflen);

/* ---- the residual add of a decoder layer, fused into the launch in front of it --------------------------------------------------------- */
/* y[1,N] = residual[1,N] + x[1,K] . dequant(w) (+ bias)                    (up == NULL)
 * y[1,N] = residual[1,N] + (act(x) * up)[1,K] . dequant(w) (+ bias)        (up != NULL: x is the gate vector, act = QLLM_ACT_SILU)
 * with the add formed INSIDE the linear launch (csrc/strip1_resid.hip, csrc/strip1_swiglu_resid.hip: the RESID forms of the batch-1
 * kernel, csrc/strip1_kernel.hpp) -- hidden = residual + o_proj(attn) and hidden = residual + down_proj(act(gate) * up) of a decoder
 * layer without the elementwise kernel behind the launch.  The 16 threads of a block that store its outputs round their fp32 value to
 * act_dtype as the plain launch does, add their element of `residual` in fp32 and round again: the eager add of two tensors.
 * Contract: the launch returns BIT FOR BIT residual + qllm_linear_forward(w, x) (residual + qllm_linear_forward_swiglu(w, x, up))
 * as torch adds two fp16 / bf16 tensors, on all finite inputs.  The element is loaded with the kernel's first loads, so the epilogue
 * waits for nothing new -- except in the ten SWIGLU forms that sit at their register bound (plain 128-wide groups with rounds of 24,
 * 56 and 64 k-steps; Llama-2-7B's down_proj, K = 11008, is one), which issue the load behind their last MFMA, ahead of the cross-wave
 * sum it is needed after.
 * x / up: contiguous [1, K] of act_dtype (QLLM_F16 / QLLM_BF16), 16-byte aligned; residual / y: [1, N] of act_dtype, aligned to the
 * element.  y may be `residual` itself (the thread that writes an element is the only one that reads it, and it reads first); any other
 * overlap of y with residual, x or up is QLLM_ERR_INVALID.
 * Served: exactly the M = 1 calls qllm_linear_forward runs on the batch-1 kernel ("strip1 ..." in qllm_plan_describe) for native-layout
 * layers (NATIVE, NATIVE_F16Z) -- 4 bits with 128- or 64-wide groups, and 3 bits -- with the same waves x round: what
 * qllm_linear_forward_swiglu serves at one row.  QLLM_ERR_UNSUPPORTED for everything else (M >= 2, other layouts and widths, act-order,
 * a QLLM_STRIP1* knob that takes the shape off that kernel): run the launch and add.  QLLM_ERR_INVALID: NULL x / residual / y,
 * misaligned x / up (16 bytes) or residual / y (the element), M < 1, a bad act_dtype, an overlap as above, act != QLLM_ACT_SILU with up
 * set.  Every error is raised before any device work.  No workspace, no host synchronisation; hipGraph-capturable.  Not built: M > 1,
 * the fused all-reduce form with a residual, the 2/5/6/7/8-bit widths.
 * ABI: the two symbols are ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged, as for the SwiGLU and RMSNorm symbols): probe for them
 * by symbol. */
int qllm_linear_forward_residual(const qllm_weight_t *w, const void *x, const void *up, const void *residual, void *y, int32_t M,
                                 int32_t act_dtype, int32_t act, void *stream);
/* What that call would launch, as text: "residual " (swiglu != 0: "residual swiglu ") followed by the plan line of the plain call
 * ("residual strip1 nw=8 round=16 exact grid=strips x 1 layout=strip-major"), or "refused: " and the refusal text.  Pure host code. */
int qllm_residual_describe(const qllm_weight_t *w, int32_t M, int32_t swiglu, char *buf, size_t buflen);

/* ---- rotary position embedding of q and k ------------------------------------------------------------------------------------------------ */
/* q_out = q * cos + rotate_half(q) * sin and k_out = k * cos + rotate_half(k) * sin, rotate_half(x) = cat(-x2, x1) of the two halves of
 * a head (the Llama / Mistral / Qwen2 convention: column d pairs with d + head_dim / 2), for both tensors in ONE launch (csrc/rope.hip;
 * the eager expression is ten elementwise kernels).  The arithmetic is the eager expression's, rounding for rounding, in act_dtype
 * (QLLM_F16 / QLLM_BF16): a = round(x * c), b = round(r * s), out = round(float(a) + float(b)) with r = -x2 for the first half and x1
 * for the second -- bit for bit what transformers' apply_rotary_pos_emb returns.
 * rows = batch * sequence tokens.  q: element (row, head, d) at q + row * q_row_stride + head * q_head_stride + d (strides in elements:
 * a view into a wider buffer is served); k likewise with k_heads heads (k_heads != q_heads: grouped-query attention).  q_out / k_out:
 * contiguous [rows, heads, head_dim].  cos / sin: contiguous [cos_rows, head_dim]; row r reads row r % cos_rows, so one [S, D] table
 * broadcast over a batch and a [B * S, D] table are both served.  An output may be its input when the strides agree (q_row_stride ==
 * q_heads * head_dim, q_head_stride == head_dim): each thread reads everything it needs before it writes.  k == NULL, k_out == NULL and
 * k_heads == 0 serve q alone.
 * QLLM_ERR_INVALID: a NULL q / cos / sin / q_out, k / k_out not matching k_heads, rows / q_heads / head_dim < 1, a bad act_dtype, a
 * cos_rows that does not divide rows, a pointer that is not 16-byte aligned, a stride that is negative or no multiple of 8.
 * QLLM_ERR_UNSUPPORTED: head_dim % 16 != 0, head_dim < 16 or head_dim > 256.  Every error is raised before any device work.  No
 * workspace, no LDS, no host synchronisation; hipGraph-capturable.  Not built: the interleaved (GPT-J) convention, partial rotary,
 * cos / sin from positions.
 * ABI: the symbol is ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged): probe for it by symbol. */
int qllm_rope(const void *q, const void *k, const void *cos, const void *sin, void *q_out, void *k_out, int32_t rows, int32_t q_heads,
              int32_t k_heads, int32_t head_dim, int64_t q_row_stride, int64_t q_head_stride, int64_t k_row_stride, int64_t k_head_stride,
              int32_t cos_rows, int32_t act_dtype, void *stream);

/* ---- single-token attention over the KV cache -------------------------------------------------------------------------------------------- */
/* out = softmax(scaling * q K^T + mask) V for ONE query token per sequence against caches [batch, kv_heads, max_len, head_dim] of which
 * the first kv_len positions count, in ONE launch (csrc/attn_decode.hip, flash-decoding): a block owns one (batch entry, kv head, split of
 * the positions) and all q_heads / kv_heads query heads of that kv head, so a K / V row is read once for the whole group; fp32 scores, an
 * fp32 online softmax, fp32 P.V on the vector ALU, one rounding to act_dtype (QLLM_F16 / QLLM_BF16) at the store.  The splits' (m, l, acc)
 * go through the workspace; the last block to arrive for a (batch entry, kv head) combines them in split order, so the result is the same
 * bits on every call.  Splits and grid are functions of (batch, kv_heads, head_dim, max_len) and the device's CU count only -- never of
 * kv_len: a captured launch serves every length.
 * q: element (b, head, d) at q + b * q_row_stride + head * q_head_stride + d (strides in elements; a view into a wider buffer is served).
 * out: contiguous [batch, q_heads, head_dim] -- the row o_proj takes.  Caches: element (b, h, pos, d) at cache + b * cache_batch_stride +
 * h * cache_head_stride + pos * cache_pos_stride + d, the same three strides for k_cache and v_cache.
 * Length: kv_len, or with kv_len_dev != NULL the int64 the kernel reads there (clamped to 0..max_len).  Positions >= kv_len are never
 * loaded.
 * Append: with k_new / v_new ([batch, kv_heads, head_dim], row and head strides each, as qllm_rope takes them) position kv_len is the new
 * token: the kernel stores the two rows into the caches and attends over kv_len + 1 positions.  With the length on the device kv_len + 1 >
 * max_len cannot be refused here: the kernel then stores nothing and attends over the first max_len positions of the cache.
 * Mask: one row per batch entry, element (b, pos) at mask + b * mask_batch_stride + pos, pos < mask_len; QLLM_ATTN_MASK_BOOL: bytes, non-zero
 * = visible; QLLM_ATTN_MASK_ADDITIVE: act_dtype values added to the scaled score, a value <= the type's lowest finite number hides the key as
 * a zero byte does (in bf16 a finite bias below about -7e29 that is not that low gets weight 0 against the floor -1e30 the running maximum
 * starts from: a row whose visible keys all carry such a bias stores zeros, not a softmax among them).  It must cover kv_len (+ 1 with an
 * append) positions, max_len with the length on the device.  A row with no visible key stores zeros.
 * Workspace: qllm_attn_decode_workspace_bytes, 16-byte aligned, its counter page zero-filled once (qllm_workspace_init); every call leaves
 * it zero.  QLLM_ERR_INVALID: a NULL q / cache / out, sizes < 1, kv_heads not dividing q_heads, a bad act_dtype or mask_kind, a mask
 * pointer not matching mask_kind, only one of k_new / v_new, a data pointer off 16 bytes, a stride that is negative or no multiple of 8,
 * a host kv_len outside 0..max_len (kv_len + 1 > max_len with an append), a mask too short.  QLLM_ERR_UNSUPPORTED: head_dim other than
 * 64 / 128, more than 8 query heads per kv head, batch * kv_heads > 4096.  QLLM_ERR_WORKSPACE: a missing, misaligned or small
 * workspace.  Every error is raised before any device work.  No host synchronisation; hipGraph-capturable.
 * Not built: chunked attention, quantized and paged caches, per-sequence lengths other than through the mask, rotary
 * inside the kernel, an fp8 cache.  A ring-buffer cache: qllm_attn_decode_ring below.  More than one query token: qllm_attn_prefill below.
 * ABI: the symbols are ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged): probe for them by symbol. */
#define QLLM_ATTN_MASK_NONE 0
#define QLLM_ATTN_MASK_BOOL 1
#define QLLM_ATTN_MASK_ADDITIVE 2
int qllm_attn_decode(const void *q, const void *k_new, const void *v_new, void *k_cache, void *v_cache, const void *mask, void *out, int32_t batch,
                     int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len, int64_t q_row_stride,
                     int64_t q_head_stride, int64_t k_new_row_stride, int64_t k_new_head_stride, int64_t v_new_row_stride, int64_t v_new_head_stride,
                     int64_t cache_batch_stride, int64_t cache_head_stride, int64_t cache_pos_stride, int32_t mask_kind, int64_t mask_len,
                     int64_t mask_batch_stride, float scaling, int32_t act_dtype, void *workspace, size_t workspace_bytes, void *stream);
/* qllm_attn_decode with a sliding window (transformers' sliding_window_overlay on a LINEAR cache: position j lives in slot j).  window =
 * W >= 1: with n the number of counted positions (kv_len, + 1 with an append) the query sits at n - 1 and sees positions max(0, n - W) ..
 * n - 1 only -- W keys including its own -- in addition to the length and the mask.  Positions below that are never loaded, a split wholly
 * below it leaves at once and is not counted, and the lower end follows the length on the device: one captured launch serves lengths on
 * both sides of the window.  A row whose keys inside the window are all masked stores zeros.  window = 0: no window, exactly
 * qllm_attn_decode (which forwards here).  window < 0: QLLM_ERR_INVALID, before any device work.  Workspace, launch shape and the
 * describe text do not depend on the window.  ADDITIVE within ABI 7: probe for it by symbol. */
int qllm_attn_decode_window(const void *q, const void *k_new, const void *v_new, void *k_cache, void *v_cache, const void *mask, void *out, int32_t batch,
                            int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len, int64_t window,
                            int64_t q_row_stride, int64_t q_head_stride, int64_t k_new_row_stride, int64_t k_new_head_stride, int64_t v_new_row_stride,
                            int64_t v_new_head_stride, int64_t cache_batch_stride, int64_t cache_head_stride, int64_t cache_pos_stride, int32_t mask_kind,
                            int64_t mask_len, int64_t mask_batch_stride, float scaling, int32_t act_dtype, void *workspace, size_t workspace_bytes,
                            void *stream);
/* qllm_attn_decode over a RING-BUFFER cache (csrc/attn_decode_ring.hip): what a sliding-window layer needs past its window without moving
 * a row.  The caches hold `slots` = C positions per (batch entry, kv head) and position j lives in slot j mod C; 1 <= window = W <= C.
 * total: the tokens counted before the call, or with total_dev != NULL the int64 the kernel reads there; clamped below at 0 and NOT above:
 * it grows for as long as the generation runs (64-bit throughout).  With k_new / v_new the call appends, n = total + 1, and the kernel
 * stores the two rows into slot (n - 1) mod C; without, n = total.  The query sits at n - 1 and sees positions lo = max(0, n - W) ..
 * n - 1, v = n - lo <= W of them; no other slot is ever loaded.  C >= W makes the append race-free: the slot it overwrites held position
 * n - 1 - C < lo.  Mask: as qllm_attn_decode's, but column r is position lo + r (the mask transformers builds for a sliding layer); it
 * must cover min(n, W) columns, W with the total on the device.  Launch shape, workspace and describe text are those of a linear call
 * whose max_len is W: qllm_attn_decode_workspace_bytes(.., W) and qllm_attn_decode_describe(.., W); split s owns r = j - lo in s * chunk
 * .. (s + 1) * chunk - 1.  The grid never depends on the total: one captured launch serves every length, on both sides of the fill.
 * The result is, bit for bit, qllm_attn_decode's on a linear copy [batch, kv_heads, W, head_dim] holding positions lo .. n - 1 in
 * slots 0 .. v - 1 with kv_len = v (v - 1 and the same append) and the same mask.
 * Errors as qllm_attn_decode's, in its order, with slots for max_len; window < 1 or slots < window and a host total < 0 are
 * QLLM_ERR_INVALID.  Every error is raised before any device work.  No host synchronisation; hipGraph-capturable.
 * Not built: prefill written into the ring by a kernel (qllm_attn_prefill reads linear caches), a ring for full-attention layers.
 * ADDITIVE within ABI 7: probe for it by symbol. */
int qllm_attn_decode_ring(const void *q, const void *k_new, const void *v_new, void *k_cache, void *v_cache, const void *mask, void *out, int32_t batch,
                          int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t total, const int64_t *total_dev, int64_t slots, int64_t window,
                          int64_t q_row_stride, int64_t q_head_stride, int64_t k_new_row_stride, int64_t k_new_head_stride, int64_t v_new_row_stride,
                          int64_t v_new_head_stride, int64_t cache_batch_stride, int64_t cache_head_stride, int64_t cache_pos_stride, int32_t mask_kind,
                          int64_t mask_len, int64_t mask_batch_stride, float scaling, int32_t act_dtype, void *workspace, size_t workspace_bytes,
                          void *stream);
/* The workspace qllm_attn_decode needs: the counter page and the splits' partial results.  Pure host code; shapes the entry refuses need
 * the page alone. */
size_t qllm_attn_decode_workspace_bytes(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t max_len);
/* What a call would launch, as text: "attn_decode tile=64 splits=16 chunk=256 grid=16x32x1 group=1 combine=last-block" (tile: positions per
 * block step; chunk: positions per split, a multiple of the tile; split s owns positions s * chunk .. (s + 1) * chunk - 1), or "refused: "
 * and the refusal text.  Pure host code. */
int qllm_attn_decode_describe(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int64_t max_len, char *buf, size_t buflen);

/* ---- prefill attention over the KV cache --------------------------------------------------------------------------------------------------- */
/* out[b, i, h, :] = softmax_j(scaling * q[b, h, i, :] . K[b, h / G, j, :] + mask[b, i, j]) V[b, h / G, j, :] for q_len >= 2 query rows per
 * sequence against caches that ALREADY hold the q_len new rows, in ONE launch (csrc/attn_prefill.hip, flash attention forward on MFMA):
 * a block of four waves owns one (batch entry, query head, tile of 128 query rows) and walks the keys in tiles of 64; fp32 scores, an fp32
 * online softmax in the log2 domain, P rounded once to act_dtype as the P.V operand, fp32 accumulators, one rounding at the store.  No
 * split over the keys, no workspace: batch * q_heads * ceil(q_len / 128) blocks, a function of the shapes alone -- never of kv_len: a
 * captured launch serves every length.
 * kv_len counts the valid positions INCLUDING the new ones; query row i sits at absolute position kv_len - q_len + i.  causal = 1: key j is
 * visible to row i only if j <= kv_len - q_len + i, and key tiles wholly above a block's diagonal are never read; causal = 0: every
 * j < kv_len counts.
 * q: element (b, head, i, d) at q + b * q_batch_stride + head * q_head_stride + i * q_row_stride + d (strides in elements: the [B, S, Hq, D]
 * projection output viewed as [B, Hq, S, D] is served in place).  out: contiguous [batch, q_len, q_heads, head_dim] -- the rows o_proj
 * takes.  Caches: as qllm_attn_decode takes them, the same three strides for both; they are only read.
 * Length: kv_len, or with kv_len_dev != NULL the int64 the kernel reads there, clamped to q_len..max_len.  Positions >= kv_len are never
 * loaded: their K and V count as zeros.  Keys hidden only by the mask or by causality ARE loaded; their rows are assumed finite.
 * Mask: element (b, i, j) at mask + b * mask_batch_stride + i * mask_row_stride + j, j < mask_len; the two kinds and constants of
 * qllm_attn_decode; mask_batch_stride may be 0.  It is applied in addition to causality.  A row with no visible key stores zeros.
 * QLLM_ERR_INVALID: a NULL q / cache / out, sizes < 1, q_len < 2 or q_len > max_len, kv_heads not dividing q_heads, a bad act_dtype,
 * mask_kind or causal, a mask pointer not matching mask_kind, a data pointer off 16 bytes, a q or cache stride that is negative or no
 * multiple of 8, a negative mask stride, a host kv_len outside q_len..max_len, a mask shorter than kv_len (max_len with the length on the
 * device).  QLLM_ERR_UNSUPPORTED: head_dim other than 64 / 128, more than 8 query heads per kv head, q_heads or batch above 65535.  Every
 * error is raised before any device work.  No host synchronisation; hipGraph-capturable.
 * Not built: a split over the keys for short q_len behind long caches, a ring-buffer cache, chunked attention, quantized and paged
 * caches, rotary or the cache append inside the kernel, dropout, attention weights as an output, backward.
 * ABI: the symbols are ADDITIVE within ABI 7 (QLLM_ABI_VERSION is unchanged): probe for them by symbol. */
int qllm_attn_prefill(const void *q, const void *k_cache, const void *v_cache, const void *mask, void *out, int32_t batch, int32_t q_heads,
                      int32_t kv_heads, int32_t head_dim, int32_t q_len, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len,
                      int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, int64_t cache_batch_stride, int64_t cache_head_stride,
                      int64_t cache_pos_stride, int32_t mask_kind, int64_t mask_len, int64_t mask_batch_stride, int64_t mask_row_stride, int32_t causal,
                      float scaling, int32_t act_dtype, void *stream);
/* qllm_attn_prefill with a sliding window on a linear cache.  window = W >= 1: row i at absolute position p = kv_len - q_len + i sees key j
 * only if p - W < j <= p, in addition to the length and the mask.  A block reads no key tile wholly below the window of its first row;
 * keys hidden by the window inside a tile it does read are loaded (weight exactly 0) and assumed finite.  window = 0: no window, exactly
 * qllm_attn_prefill (which forwards here).  window < 0: QLLM_ERR_INVALID; window >= 1 with causal = 0: QLLM_ERR_UNSUPPORTED; both before
 * any device work.  The launch shape does not depend on the window.  ADDITIVE within ABI 7: probe for it by symbol. */
int qllm_attn_prefill_window(const void *q, const void *k_cache, const void *v_cache, const void *mask, void *out, int32_t batch, int32_t q_heads,
                             int32_t kv_heads, int32_t head_dim, int32_t q_len, int64_t kv_len, const int64_t *kv_len_dev, int64_t max_len, int64_t window,
                             int64_t q_batch_stride, int64_t q_head_stride, int64_t q_row_stride, int64_t cache_batch_stride, int64_t cache_head_stride,
                             int64_t cache_pos_stride, int32_t mask_kind, int64_t mask_len, int64_t mask_batch_stride, int64_t mask_row_stride,
                             int32_t causal, float scaling, int32_t act_dtype, void *stream);
/* What a call would launch, as text: "attn_prefill q_tile=128 kv_tile=64 grid=2x32x1 group=4", or "refused: " and the refusal text.  Pure
 * host code. */
int qllm_attn_prefill_describe(int32_t batch, int32_t q_heads, int32_t kv_heads, int32_t head_dim, int32_t q_len, int64_t max_len, char *buf,
                               size_t buflen);

/* ---- HQQ quantizer (ABI 7) ---------------------------------------------------------------------------------------------------------- */
/* W[N,K] (fp16 / bf16 / fp32 by w_dtype, row-major, 16-byte aligned) -> the HQQ layer buffers: qweight i32 [K*bits/32][N], scales f16
 * [K/g][N] = fp16(1/s), zeros f16 [K/g][N] = fp16(z).  The algorithm is HQQQuant.do_quantize's (qllm/quantization/hqq/quant_hqq.py:34-36,
 * _hqq_quantizer.py:29-121: axis=1, channel_wise, optimize, round_zero) in fp32, the dtype of the reference's CPU solver: per group of
 * g consecutive k of one row, s = min(max_v * (1 / (max - min)), 2e4) (two roundings, as torch divides a scalar by a tensor), z = rint(-min s), then up to `iters` rounds of
 *   Wq = clamp(rint(W s + z), 0, max_v);  x = W - (Wq - z) / s;  We = sign(x) max(|x| - |x|^(lp_norm-1) / beta, 0);
 *   z = mean_group(Wq - (W - We) s);  beta *= kappa
 * stopped, like the reference, after the first round whose TENSOR-wide mean |x| does not fall below the best so far (that round's z
 * update is kept); codes = clamp(rint(W s + z), 0, max_v) with the final fp32 z.  The reference's defaults: iters 20, lp_norm 0.7,
 * beta 10, kappa 1.01.  One fused kernel, run twice around a one-block reduction (csrc/hqq_quant.hip): no host synchronisation, no
 * atomics, bit-reproducible, hipGraph-capturable.  rounds_run_dev (nullable, device int32): the number of rounds that were run.
 * Serves bits 2 / 3 / 4 / 8, g % 32 == 0 with 32 <= g <= 1024, K % g == 0, N % 16 == 0, lp_norm < 1, iters <= 64 (beyond: QLLM_ERR_INVALID);
 * other shapes and lp_norm >= 1: QLLM_ERR_UNSUPPORTED.  Workspace: qllm_hqq_quantize_workspace_bytes() (pure; 0 for shapes never served),
 * 16-byte aligned, needs no initialisation; after the call its first int32 is rounds_run and the floats from byte 256 on are the per-round
 * tensor-wide mean errors.  Debug output: a workspace with room for 2 x N x K/g further floats behind the required bytes (rounded up to
 * 256) also receives the solver's fp32 s [K/g][N] and z [K/g][N] there. */
size_t qllm_hqq_quantize_workspace_bytes(int32_t N, int32_t K, int32_t group_size, int32_t iters);
int qllm_hqq_quantize(const void *w_nk, int32_t w_dtype, int32_t N, int32_t K, int32_t bits, int32_t group_size, int32_t iters,
                      float lp_norm, float beta, float kappa, void *qweight, void *scales, void *zeros, int32_t *rounds_run_dev,
                      void *workspace, size_t workspace_bytes, void *stream);

/* ---- GPTQ quantizer (additive to ABI 7) ---------------------------------------------------------------------------------------------- */
/* The column solver of GPTQ.fasterquant (qllm/quantization/gptq/gptq.py:129-258) with blocksize = 128, static_groups = False, mse = False,
 * perchannel = True, in fp32, for all K columns of a layer in one kernel (csrc/gptq_quant.hip).  The caller prepares what is plumbing:
 * w_nk [N,K] (fp16 / bf16 / fp32 by w_dtype, row-major) with its columns already in processing order (act-order: permuted; dead columns
 * zeroed) and u_kk [K,K] fp32 row-major, the UPPER Cholesky factor of the inverse of the damped (and equally permuted) Hessian; only
 * its upper triangle is used (the 128 x 128 tiles on the diagonal are loaded whole, so what lies below it must be readable, and no
 * value there reaches a result); u_kk is 16-byte aligned and K a multiple of 4 (QLLM_ERR_INVALID otherwise).
 * Columns are walked left to right in blocks of 128 (the last one may be narrower):
 *   per column i:  q = scale * (clamp(rint(w / scale) + zero, 0, maxq) - zero);  err = (w - q) / U[i,i];
 *                  every later column j of the same block: w[j] -= err * U[i,j]   (a product, then a difference: two roundings)
 *   per block:     the columns behind the block receive Err(N x 128) . U[block, j] -- in the order of the blocks -- before they are used.
 * Group parameters are found when column c with c % group_size == 0 is reached, from columns c .. c+group_size-1 in their state at the
 * last BLOCK boundary (all earlier blocks' updates, none of the current block's): with group_size 32 / 64 this differs from the
 * column-by-column state, which makes the 128-column block part of the semantics.  group_size == K (the reference's -1): one set per
 * row from w_nk as given.  find_params (per row of the group): xmin = min(min, 0), xmax = max(max, 0); sym: xmax = max(|xmin|, xmax) and
 * xmin = -xmax where xmin < 0; xmin == xmax == 0 -> (-1, +1); scale = (xmax - xmin) / maxq; zero = (maxq + 1) / 2 (sym) or
 * rint(-xmin / scale), maxq = 2^bits - 1.
 * Outputs: codes_kn i32 [K,N] (column order of w_nk); scales_ng / zeros_ng f32 [N, K/group_size] (zero is integer-valued); wq_nk
 * (nullable) [N,K] = scale * (code - zero) rounded to w's dtype; loss_n (nullable) f32 [N] = sum over the row of (w - q)^2 / U[i,i]^2 / 2.
 * u_kk == NULL stands for the identity: plain round-to-nearest on the same grid (no update; parameters from w_nk itself).
 * Serves bits 2..8 and group_size 32 / 64 / 128 / K (others: QLLM_ERR_UNSUPPORTED); K % group_size != 0, NULL or misaligned buffers:
 * QLLM_ERR_INVALID; all of it before any device work.  Every buffer aligned to its element size.  Workspace:
 * qllm_gptq_quantize_workspace_bytes() (pure: N x K floats, the error history each row tile keeps for its own rows), 16-byte aligned,
 * needs no initialisation.  No host synchronisation, no atomics, bit-reproducible, hipGraph-capturable.
 * Not served (the reference's other switches): mse, trits, Conv layers; static_groups is qllm_gptq_quantize_static below. */
size_t qllm_gptq_quantize_workspace_bytes(int32_t N, int32_t K);
int qllm_gptq_quantize(const void *w_nk, int32_t w_dtype, const float *u_kk, int32_t N, int32_t K, int32_t bits, int32_t group_size,
                       int32_t sym, int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, float *loss_n, void *workspace,
                       size_t workspace_bytes, void *stream);

/* The same solver with static_groups = True (gptq.py:157-165, 207-211, 230-233; csrc/gptq_static.hip): every group's scale / zero is
 * found from the weights as given, before the walk, and the walk only looks them up.  The columns are still processed in the caller's
 * order, so a layer quantized with act-order keeps the trivial g_idx[i] = i / group_size and decodes like a plain one.
 * w_nk [N,K] is in the ORIGINAL column order (dead columns zeroed); perm_k (nullable: identity) i32 [K] maps processing position j to
 * the original column perm_k[j] and must be a permutation of 0..K-1 (not checked here: entries are clamped to 0..K-1, so a bad one
 * gives a wrong result and no access outside the buffers); u_kk (nullable) is in PROCESSING order, as for qllm_gptq_quantize.
 * Parameters of group c of a row: find_params (above) over columns c*group_size .. c*group_size+group_size-1 of w_nk.  Column j of the
 * walk loads w_nk[n][perm_k[j]], uses the parameters of group perm_k[j] / group_size, and its quantization, error, in-block and
 * trailing updates and loss are qllm_gptq_quantize's, rounding for rounding.
 * Outputs as for qllm_gptq_quantize, but codes_kn and wq_nk are already in the ORIGINAL column order (codes_kn[perm_k[j]][n]) and
 * scales_ng / zeros_ng in the original group numbering: nothing is left to un-permute.  u_kk == NULL: round-to-nearest; perm_k is then
 * not consulted and every output equals qllm_gptq_quantize's with u_kk == NULL.  group_size == K: the result of qllm_gptq_quantize on
 * w_nk[:, perm_k] in the original order.  Validation, the served shapes and the workspace (qllm_gptq_quantize_workspace_bytes) are
 * qllm_gptq_quantize's; perm_k 4-byte aligned.  No host synchronisation, no atomics, bit-reproducible, hipGraph-capturable. */
int qllm_gptq_quantize_static(const void *w_nk, int32_t w_dtype, const float *u_kk, const int32_t *perm_k, int32_t N, int32_t K, int32_t bits,
                              int32_t group_size, int32_t sym, int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk,
                              float *loss_n, void *workspace, size_t workspace_bytes, void *stream);

/* ---- AWQ quantizer (additive to ABI 7) ----------------------------------------------------------------------------------------------- */
/* The two device steps of the AWQ search (qllm/quantization/awq/_awq_quantizer.py) with zero_point = True, in fp32 (csrc/awq_quant.hip).
 * pseudo_quantize of a group of group_size values v with minimum vmin and maximum vmax, maxq = 2^bits - 1, true divisions, no contraction:
 *   sc = max(vmax - vmin, 1e-5) / maxq;  z = clamp(-rint(vmin / sc), 0, maxq);  code = clamp(rint(v / sc) + z, 0, maxq);  q = (code - z) * sc
 *
 * qllm_awq_quantize: w_nk [N,K] (fp16 / bf16 / fp32 by w_dtype, row-major), col_scale_k (nullable: 1) f32 [K], clip_ng (nullable: none)
 * f32 [N, K/group_size]:  v = w * col_scale, rounded to w's type when that is a 16-bit one (what an in-place product leaves);
 * v = clamp(v, -clip, clip); the grid above per (row, group).  Outputs, each nullable (not all of them): codes_kn i32 [K,N];
 * scales_ng / zeros_ng f32 [N, K/group_size] (zero is integer-valued); wq_nk [N,K] = (code - z) * sc / col_scale rounded to w's type.
 *
 * qllm_awq_clip_search: auto_clip_layer as a quadratic form.  gram f32 [K/group_size][group_size][group_size], 16-byte aligned: per group
 * the Gram matrix X^T X / tokens of the group's input channels.  Per (row, group) with org = max |w|, for i = 0 .. int(max_shrink *
 * n_grid) - 1 (1..10 candidates):  m = org * float32(1 - i / n_grid);  d = pseudo_quantize(clamp(w, -m, m)) - w;  e_i = d^T gram_j d
 * (fp32 FMAs) = the reference's ((x.q) - (x.w))^2 averaged over the tokens.  The first strict minimum below 1e9 wins (none: i = 0).
 * Outputs: best_max_ng f32 = org * float32(1 - i / n_grid) of the winner, best_idx_ng i32 = i, err_ng2 f32 [N, K/group_size, 2] = (e_0, the
 * winner's e).  Workspace: qllm_awq_clip_search_workspace_bytes() (pure; currently 0: workspace may then be NULL), 16-byte aligned.
 *
 * Both serve bits 2..8 and group_size 32 / 64 / 128 (others: QLLM_ERR_UNSUPPORTED); K % group_size != 0, NULL or misaligned buffers:
 * QLLM_ERR_INVALID; a short or misaligned workspace: QLLM_ERR_WORKSPACE; all of it before any device work.  One launch each, no host
 * synchronisation, no atomics, bit-reproducible, hipGraph-capturable.  Not served: symmetric grids, group_size = -1. */
size_t qllm_awq_clip_search_workspace_bytes(int32_t N, int32_t K, int32_t group_size);
int qllm_awq_clip_search(const void *w_nk, int32_t w_dtype, const float *gram, int32_t N, int32_t K, int32_t bits, int32_t group_size, int32_t n_grid,
                         float max_shrink, float *best_max_ng, int32_t *best_idx_ng, float *err_ng2, void *workspace, size_t workspace_bytes,
                         void *stream);
int qllm_awq_quantize(const void *w_nk, int32_t w_dtype, const float *col_scale_k, const float *clip_ng, int32_t N, int32_t K, int32_t bits,
                      int32_t group_size, int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, void *stream);

/* ---- tensor-parallel decode: one-shot all-reduce over peer-mapped staging buffers (ABI 4; fused form ABI 5) -------------------------------------- */
/* For decode-sized tensors ([1, 8192] fp16 = 16 KB per row-parallel layer) a ring / tree all-reduce is pure latency.  On the xGMI
 * full mesh every rank instead writes its vector into every peer's staging buffer (one hop), waits for the world's flags and sums
 * locally in rank order (bit-identical on every rank).  One process per GPU: each rank allocates ONE staging buffer
 * (qllm_comm_buffer_bytes: 2 parities x world slots + a control block; fine-grained device memory -- qllm_comm_alloc is the only
 * allocation this library ever makes, and only on request), exports it as a 64-byte HIP IPC handle, imports the peers' handles, and
 * passes the device array of the `world` buffer addresses (its own at index `rank`) to every call.  x_inout: n elements (n % 8 == 0,
 * n * 2 <= slot_bytes), summed in place; the call is a single kernel on `stream`, keeps its epoch in device memory and is
 * hipGraph-capturable.  status_dev (nullable): set to 1 by the kernel if a peer never arrived.  Every rank must make the same
 * sequence of calls.  qllm_amd/comm.py wraps it behind torch.distributed; no counterpart in the reference (no distributed code). */
size_t qllm_comm_buffer_bytes(int32_t world, size_t slot_bytes);
int qllm_comm_alloc(size_t bytes, void **ptr);
int qllm_comm_free(void *ptr);
int qllm_comm_export(void *ptr, void *handle64);
int qllm_comm_import(const void *handle64, void **ptr);
int qllm_comm_close(void *ptr);
int qllm_allreduce_oneshot(void *const *peers_dev, int32_t rank, int32_t world, void *x_inout, int32_t n, int32_t act_dtype,
                           size_t slot_bytes, int32_t *status_dev, void *stream);
/* (ABI 5) A row-parallel layer at batch 1 fused with that all-reduce: y[1, N] = sum over ranks of (x_rank . dequant(W_rank)) in ONE
 * launch per rank.  Every block of the batch-1 kernel pushes its 16 partial outputs -- rounded to the activation type exactly as
 * the unfused path's y -- into every peer's staging slot; the rank's last block publishes the flags, waits for the world's and
 * writes the rank-ordered fp32 sum: bit-identical to qllm_linear_forward + qllm_allreduce_oneshot, one kernel boundary less per
 * row-parallel layer (o_proj, down_proj: 160 per Llama-2-70B token).  Same staging buffers, epoch and calling discipline as
 * qllm_allreduce_oneshot (the two may be mixed on one stream).  Serves M == 1 on native 4-bit layers with 128-wide groups whose
 * K per rank the batch-1 kernel takes (<= 16384), N * 2 <= slot_bytes, y 16-byte aligned; anything else: QLLM_ERR_UNSUPPORTED
 * and the caller runs the two calls separately.  No counterpart in the reference (no distributed code). */
int qllm_linear_forward_allreduce(const qllm_weight_t *w, const void *x, void *y, int32_t M, int32_t act_dtype, void *const *peers_dev,
                                  int32_t rank, int32_t world, size_t slot_bytes, int32_t *status_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* QLLM_MI355X_H_ */
