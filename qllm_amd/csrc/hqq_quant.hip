// HQQ quantizer (ABI 7): fp16 / bf16 / fp32 W[N,K] -> HQQ row-stream qweight + fp16 scales / zero points, the half-quadratic
// proximal solver of qllm/quantization/hqq/_hqq_quantizer.py (axis=1, channel_wise, optimize, round_zero) fused into one kernel.
//
// Work split: one block = one tile of 16 rows n x one group of g consecutive k; 16 lanes own one (row, group), E = g/16 consecutive
// elements per lane, held in registers through every round (W is read from HBM exactly once per pass).  Min, max and the mean of the
// zero-point update are 16-lane DPP butterflies (every lane of the row ends with the same bits).  All arithmetic is fp32 with one
// rounding per operation (-ffp-contract=off), in the order of the reference's tensor expressions.
//
// The reference stops the first time the TENSOR-wide mean |W - Wr| fails to decrease.  No host synchronisation, no float atomics:
//   pass 1  runs all `iters` rounds and leaves per-block, per-round sums of |W - Wr| in the workspace (blocks walk their tiles in a
//           fixed order, waves are added in a fixed order);
//   reduce  one block adds the per-block sums in a fixed order (double), replays the reference's comparison and writes the number of
//           rounds the reference would have run to the workspace (and to rounds_run_dev);
//   pass 2  reads that number, re-runs that many rounds (the same instructions on the same data: the same bits) and encodes.
// Codes go through an LDS transpose ([k][16 rows] bytes) so that each packed word row is stored as 16 consecutive int32 along N.
#include "quant_common.hpp"

namespace qllm {

namespace {

constexpr int kHqqHeaderBytes = 1024;  // [0]: rounds to run (int) | [256 ..]: per-round tensor-wide mean |W - Wr| (float[64])
constexpr int kHqqMaxBlocks = 2048;

template <int CTRL>
__device__ __forceinline__ float dpp_peer(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// butterflies over the 16 lanes of a DPP row: quad xor 1, quad xor 2, half-row mirror, row mirror (strip1_kernel.hpp, dpp_add1)
__device__ __forceinline__ float row_sum(float v) {
  v = v + dpp_peer<0xB1>(v);
  v = v + dpp_peer<0x4E>(v);
  v = v + dpp_peer<0x141>(v);
  return v + dpp_peer<0x140>(v);
}
__device__ __forceinline__ float row_min(float v) {
  v = fminf(v, dpp_peer<0xB1>(v));
  v = fminf(v, dpp_peer<0x4E>(v));
  v = fminf(v, dpp_peer<0x141>(v));
  return fminf(v, dpp_peer<0x140>(v));
}
__device__ __forceinline__ float row_max(float v) {
  v = fmaxf(v, dpp_peer<0xB1>(v));
  v = fmaxf(v, dpp_peer<0x4E>(v));
  v = fmaxf(v, dpp_peer<0x141>(v));
  return fmaxf(v, dpp_peer<0x140>(v));
}

// E elements of T at `src`: one aligned vector read when the lane owns exactly E (e == E: src is then E * sizeof(T) aligned),
// element reads under `j < e` for group sizes between two instantiations
template <typename T, int E>
__device__ __forceinline__ void load_elems(const T *src, int e, float (&w)[E]) {
  if (e == E) {
    constexpr int BYTES = E * (int)sizeof(T);
    constexpr int CH = BYTES >= 16 ? 16 : BYTES;  // 4, 8 or 16 bytes per read
    T raw[E];
#pragma unroll
    for (int c = 0; c < BYTES / CH; ++c)
      __builtin_memcpy((char *)raw + c * CH, __builtin_assume_aligned((const char *)src + c * CH, CH), CH);
#pragma unroll
    for (int j = 0; j < E; ++j) w[j] = to_f32(raw[j]);
  } else {
#pragma unroll
    for (int j = 0; j < E; ++j) w[j] = j < e ? to_f32(src[j]) : 0.f;
  }
}

}  // namespace

struct HqqQuantParams {
  const void *w;
  uint32_t *qweight;
  half_t *scales, *zeros;
  float *dbg_s, *dbg_z;   // nullable: the solver's fp32 s and z, [K/g][N]
  float *block_err;       // [blocks][iters]
  int *rounds;            // workspace header
  int N, K, g, bits, iters, e, tiles, final_pass;
  float max_v, pm1;
  float inv_beta[64];     // fp32(1 / beta_r), beta_r carried in double on the host like the reference's Python float
};

template <typename T, int E>
__global__ __launch_bounds__(256) void hqq_quant_kernel(HqqQuantParams p) {
  __shared__ float s_err[4][64];
  __shared__ uint8_t s_q[E * 16 * 16];  // final pass: codes of the tile, [k][row]
  const int tid = threadIdx.x, wave = tid >> 6, row = tid >> 4, l = tid & 15;
  const int e = p.e, g = p.g, G = p.K / g;
  const bool fin = p.final_pass != 0;
  const int rounds = fin ? *p.rounds : p.iters;
  const float max_v = p.max_v, pm1 = p.pm1, gf = (float)g;
  if (tid < 64) { s_err[0][tid] = 0.f; s_err[1][tid] = 0.f; s_err[2][tid] = 0.f; s_err[3][tid] = 0.f; }
  __syncthreads();
  for (int tile = blockIdx.x; tile < p.tiles; tile += gridDim.x) {
    const int nb = tile / G, kg = tile - nb * G;
    const int n = nb * 16 + row;
    float w[E];
    load_elems<T, E>((const T *)p.w + (size_t)n * p.K + (size_t)kg * g + l * e, e, w);
    float mn = __builtin_inff(), mx = -__builtin_inff();
#pragma unroll
    for (int j = 0; j < E; ++j)
      if (j < e) { mn = fminf(mn, w[j]); mx = fmaxf(mx, w[j]); }
    mn = row_min(mn);
    mx = row_max(mx);
    // the reference's `max_v / (max - min)` is torch's scalar / tensor: reciprocal, then the product -- two roundings
    const float s = fminf(__fdiv_rn(1.0f, mx - mn) * max_v, 2e4f);
    float z = rintf(-mn * s);
    for (int r = 0; r < rounds; ++r) {
      const float ib = p.inv_beta[r];
      float acc = 0.f, es = 0.f;
#pragma unroll
      for (int j = 0; j < E; ++j) {
        if (j < e) {
          const float wq = fminf(fmaxf(rintf(w[j] * s + z), 0.f), max_v);
          const float wr = __fdiv_rn(wq - z, s);
          const float x = w[j] - wr;
          const float ax = fabsf(x);
          es += ax;
          // x == 0: |x|^(p-1) = inf, the difference -inf, the max 0 -- never a NaN (the reference's 0 * relu(-inf))
          const float we = copysignf(fmaxf(ax - ib * powf(ax, pm1), 0.f), x);
          acc += wq - (w[j] - we) * s;
        }
      }
      z = __fdiv_rn(row_sum(acc), gf);
      if (!fin) {
        es = row_sum(es);
        es += __shfl_xor(es, 16);
        es += __shfl_xor(es, 32);
        if ((tid & 63) == 0) s_err[wave][r] += es;
      }
    }
    if (fin) {
#pragma unroll
      for (int j = 0; j < E; ++j)
        if (j < e) s_q[(l * e + j) * 16 + row] = (uint8_t)fminf(fmaxf(rintf(w[j] * s + z), 0.f), max_v);
      if (l == 0) {
        const size_t o = (size_t)kg * p.N + n;
        p.scales[o] = (half_t)__fdiv_rn(1.0f, s);
        p.zeros[o] = (half_t)z;
        if (p.dbg_s) { p.dbg_s[o] = s; p.dbg_z[o] = z; }
      }
      __syncthreads();
      const int bits = p.bits, wrows = g * bits / 32;
      for (int idx = tid; idx < wrows * 16; idx += 256) {
        const int r = idx >> 4, c = idx & 15, bit0 = r * 32;
        uint32_t word = 0;
        for (int k = bit0 / bits; k < g && k * bits < bit0 + 32; ++k) {
          const int sh = k * bits - bit0;
          const uint32_t q = s_q[k * 16 + c];
          word |= sh >= 0 ? q << sh : q >> -sh;
        }
        p.qweight[((size_t)kg * wrows + r) * p.N + nb * 16 + c] = word;
      }
      __syncthreads();
    }
  }
  if (!fin) {
    __syncthreads();
    if (tid < p.iters) p.block_err[(size_t)blockIdx.x * p.iters + tid] = ((s_err[0][tid] + s_err[1][tid]) + s_err[2][tid]) + s_err[3][tid];
  }
}

// the reference's loop control: best = 1e4; a round whose tensor-wide mean error is not below the best so far is the last one
__global__ __launch_bounds__(256) void hqq_stop_kernel(const float *block_err, int blocks, int iters, double inv_count, int *header,
                                                       int *rounds_out) {
  __shared__ double s_part[256];
  __shared__ float s_mean[64];
  const int tid = threadIdx.x;
  for (int r = 0; r < iters; ++r) {
    double a = 0.0;
    for (int b = tid; b < blocks; b += 256) a += (double)block_err[(size_t)b * iters + r];
    s_part[tid] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
      if (tid < h) s_part[tid] += s_part[tid + h];
      __syncthreads();
    }
    if (tid == 0) s_mean[r] = (float)(s_part[0] * inv_count);
    __syncthreads();
  }
  if (tid == 0) {
    float best = 1e4f;
    int run = iters;
    for (int r = 0; r < iters; ++r) {
      if (s_mean[r] < best) best = s_mean[r];
      else { run = r + 1; break; }
    }
    header[0] = run;
    if (rounds_out) *rounds_out = run;
  }
  if (tid < 64) ((float *)header)[64 + tid] = tid < iters ? s_mean[tid] : 0.f;
}

static int hqq_blocks(int N, int K, int g) {
  const long tiles = (long)(N / 16) * (K / g);
  return (int)(tiles < kHqqMaxBlocks ? tiles : kHqqMaxBlocks);
}

bool hqq_quant_shape_ok(int N, int K, int bits, int g) {
  return (bits == 2 || bits == 3 || bits == 4 || bits == 8) && g >= 32 && g <= 1024 && g % 32 == 0 && K % g == 0 && N % 16 == 0;
}

size_t hqq_quant_workspace_bytes(int N, int K, int g, int iters) {
  if (N <= 0 || K <= 0 || g <= 0 || iters <= 0 || iters > 64 || K % g || N % 16) return 0;
  return (size_t)kHqqHeaderBytes + (size_t)hqq_blocks(N, K, g) * iters * sizeof(float);
}

template <typename T>
static void hqq_launch_e(const HqqQuantParams &p, int blocks, hipStream_t stream) {
  const int e = p.e;
  if (e <= 2) hipLaunchKernelGGL((hqq_quant_kernel<T, 2>), dim3(blocks), dim3(256), 0, stream, p);
  else if (e <= 4) hipLaunchKernelGGL((hqq_quant_kernel<T, 4>), dim3(blocks), dim3(256), 0, stream, p);
  else if (e <= 8) hipLaunchKernelGGL((hqq_quant_kernel<T, 8>), dim3(blocks), dim3(256), 0, stream, p);
  else if (e <= 16) hipLaunchKernelGGL((hqq_quant_kernel<T, 16>), dim3(blocks), dim3(256), 0, stream, p);
  else if (e <= 32) hipLaunchKernelGGL((hqq_quant_kernel<T, 32>), dim3(blocks), dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((hqq_quant_kernel<T, 64>), dim3(blocks), dim3(256), 0, stream, p);
}

static void hqq_launch(const HqqQuantParams &p, int w_dtype, int blocks, hipStream_t stream) {
  with_w_type(w_dtype, [&](auto tag) { hqq_launch_e<decltype(tag)>(p, blocks, stream); });
}

int launch_hqq_quantize(const void *w_nk, int w_dtype, int N, int K, int bits, int g, int iters, float lp_norm, float beta, float kappa,
                        void *qweight, void *scales, void *zeros, int *rounds_run_dev, void *workspace, size_t workspace_bytes,
                        hipStream_t stream) {
  HqqQuantParams p{};
  p.w = w_nk;
  p.qweight = (uint32_t *)qweight;
  p.scales = (half_t *)scales;
  p.zeros = (half_t *)zeros;
  p.N = N; p.K = K; p.g = g; p.bits = bits; p.iters = iters; p.e = g / 16;
  p.tiles = (N / 16) * (K / g);
  p.max_v = maxq_of(bits);
  p.pm1 = (float)((double)lp_norm - 1.0);
  double b = (double)beta;
  for (int r = 0; r < 64; ++r) {
    p.inv_beta[r] = (float)(1.0 / b);
    b *= (double)kappa;
  }
  const int blocks = hqq_blocks(N, K, g);
  const size_t need = hqq_quant_workspace_bytes(N, K, g, iters), groups = (size_t)N * (K / g);
  p.rounds = (int *)workspace;
  p.block_err = (float *)((char *)workspace + kHqqHeaderBytes);
  // debug output: a workspace with room for 2 x N x K/g more floats after the required bytes also receives the solver's fp32 s and z
  const size_t dbg_at = (need + 255) / 256 * 256;
  if (workspace_bytes >= dbg_at + 2 * groups * sizeof(float)) {
    p.dbg_s = (float *)((char *)workspace + dbg_at);
    p.dbg_z = p.dbg_s + groups;
  }
  p.final_pass = 0;
  hqq_launch(p, w_dtype, blocks, stream);
  hipLaunchKernelGGL(hqq_stop_kernel, dim3(1), dim3(256), 0, stream, p.block_err, blocks, iters, 1.0 / ((double)N * (double)K), p.rounds,
                     rounds_run_dev);
  p.final_pass = 1;
  hqq_launch(p, w_dtype, blocks, stream);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
