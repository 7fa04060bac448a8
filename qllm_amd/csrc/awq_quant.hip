// AWQ quantizer kernels: the clip search of auto_clip_layer and the pseudo-quantizer of pseudo_quantize_tensor (zero_point=True) of
// qllm/quantization/awq/_awq_quantizer.py, on fp16 / bf16 / fp32 W[N,K], in fp32.
//
// Both kernels share one mapping.  Rows and groups are independent.  A block of 256 threads owns 16 rows; 16 lanes (one DPP row) own a
// row and lane l holds g/16 of the current group's g columns in registers (g = 128: columns 4l..4l+3 and 64+4l..64+4l+3; g = 64:
// 4l..4l+3; g = 32: 2l, 2l+1).  A block walks the groups blockIdx.y, blockIdx.y + gridDim.y, ...; no block waits for another one, there
// are no atomics and no workspace: bit-reproducible, and a row's results do not depend on the tile it sits in.
//
// Clip search.  The reference's error of a candidate, ((x.q) - (x.w))^2 averaged over the tokens, is the quadratic form d^T Gm d with
// d = q - w and Gm = X^T X / T of the group's g input channels, so the [rows, tokens, groups, g] tensors of the reference collapse into
// a g x g fp32 tile per group, staged in LDS once per (row tile, group) (64 KB at g = 128).  The lane keeps d of the candidates in
// registers (all ten; at g = 128 five at a time).  The form needs every pair (a, b) of columns once: in 16 steps a copy of d travels round the row's 16 lanes (one
// v_mov_dpp row_ror:1 per value and step; the owner's lane number travels with it, so nothing here depends on the direction of the
// rotation), and at each step a lane adds  sum_b d_b (sum_a d'_a Gm[a][b])  over its own columns b and the visiting columns a, reading
// Gm[a][own columns] with 16-byte LDS loads (8-byte at g = 32).  Lanes of one row read different rows of the tile at different bank
// offsets (4l, resp. 2l + 32k, dwords): conflict-free; the four rows of a wave read the same addresses: a broadcast.  The products are
// explicit FMAs (this file is compiled with -ffp-contract=off: the quantization arithmetic must round where the reference rounds).
#include "quant_common.hpp"

namespace qllm {

namespace {

constexpr int kRows = 16;    // rows per thread block
constexpr int kCand = 10;    // the most clip candidates one search evaluates: int(max_shrink * n_grid) of the reference's defaults

// the c-th column (of the group) that lane l of a row holds, CPL = g / 16 columns per lane
template <int CPL> __device__ __forceinline__ int col_of(int l, int c) {
  if (CPL == 8) return (c >> 2) * 64 + 4 * l + (c & 3);
  return CPL * l + c;
}

// pseudo_quantize_tensor on one value of a group with minimum vmin and maximum vmax: the grid, then the dequantized value
__device__ __forceinline__ void grid_of(float vmin, float vmax, float maxq, float &sc, float &z) {
  sc = __fdiv_rn(fmaxf(vmax - vmin, 1e-5f), maxq);
  z = fminf(fmaxf(-rintf(__fdiv_rn(vmin, sc)), 0.f), maxq);
}
__device__ __forceinline__ float code_of(float v, float sc, float z, float maxq) {
  return fminf(fmaxf(rintf(__fdiv_rn(v, sc)) + z, 0.f), maxq);
}

__device__ __forceinline__ float row_ror1(float v) {   // the value of the neighbouring lane of the same 16-lane row
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xf, 0xf, false));
}
__device__ __forceinline__ int row_ror1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0x121, 0xf, 0xf, false); }

}  // namespace

struct AwqClipParams {
  const void *w;       // [N][K]
  const float *gram;   // [K/g][g][g]
  float *best_max;     // [N][K/g]
  int32_t *best_idx;   // [N][K/g]
  float *err;          // [N][K/g][2]
  int N, K, g, nc;
  float maxq;
  float shrink[kCand]; // float32(1 - i / n_grid)
};

template <typename T, int CPL>
// two waves per SIMD: two blocks per CU, so the 16 rotation steps of one hide the LDS latency of the other (<= 256 registers)
__global__ __launch_bounds__(256, 2) void awq_clip_kernel(AwqClipParams p) {
  constexpr int g = 16 * CPL;
  __shared__ __attribute__((aligned(16))) float s_g[g * g];
  const int tid = threadIdx.x, row = tid >> 4, l = tid & 15;
  const int N = p.N, K = p.K, G = K / g;
  const int n = blockIdx.x * kRows + row;
  const bool live = n < N;
  const float maxq = p.maxq;
  const T *wrow = (const T *)p.w + (size_t)(live ? n : 0) * K;

  for (int j = blockIdx.y; j < G; j += gridDim.y) {
    __syncthreads();   // the tile of the previous group has been read by everyone
    const float *gm = p.gram + (size_t)j * g * g;
    for (int idx = tid; idx < g * g / 4; idx += 256) *(float4 *)&s_g[4 * idx] = *(const float4 *)&gm[4 * idx];

    float w[CPL];
    float mn = 0.f, mx = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      w[c] = live ? to_f32(wrow[(size_t)j * g + col_of<CPL>(l, c)]) : 0.f;
      mn = c ? fminf(mn, w[c]) : w[c];
      mx = c ? fmaxf(mx, w[c]) : w[c];
    }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const MinMax r = minmax_xor({mn, mx}, m); mn = r.mn; mx = r.mx; }
    const float org = fmaxf(fabsf(mn), fabsf(mx));

    // d = q - w of the candidates, kBatch at a time: at g = 128 ten of them with their travelling copy would not leave two blocks per CU
    // their registers
    constexpr int kBatch = CPL == 8 ? 5 : kCand;
    float best = 1e9f, e0 = 0.f;   // the first strict minimum (the reference's err < min_errs, from 1e9)
    int bi = 0;
    __syncthreads();
#pragma unroll 1
    for (int i0 = 0; i0 < kCand; i0 += kBatch) {
      float d[kBatch][CPL], rot[kBatch][CPL], e[kBatch];
#pragma unroll
      for (int i = 0; i < kBatch; ++i) {
        const float m = org * p.shrink[i0 + i];
        float sc, z;
        grid_of(fmaxf(mn, -m), fminf(mx, m), maxq, sc, z);   // clamping is monotone: the extremes of the clamped group
#pragma unroll
        for (int c = 0; c < CPL; ++c) {
          const float v = fminf(fmaxf(w[c], -m), m);
          d[i][c] = (code_of(v, sc, z, maxq) - z) * sc - w[c];
          rot[i][c] = d[i][c];
        }
        e[i] = 0.f;
      }
      int src = l;   // the lane whose columns `rot` holds
#pragma unroll 1
      for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int h = 0; h < (CPL + 3) / 4; ++h) {       // the lane's own columns, four (two at g = 32) at a time
          constexpr int Q = CPL < 4 ? CPL : 4;
          float gq[CPL][Q];
#pragma unroll
          for (int ca = 0; ca < CPL; ++ca) {
            const float *gp = &s_g[col_of<CPL>(src, ca) * g + col_of<CPL>(l, 4 * h)];
            if constexpr (Q == 4) {
              const float4 t = *(const float4 *)gp;
              gq[ca][0] = t.x; gq[ca][1] = t.y; gq[ca][2] = t.z; gq[ca][3] = t.w;
            } else {
              const float2 t = *(const float2 *)gp;
              gq[ca][0] = t.x; gq[ca][1] = t.y;
            }
          }
#pragma unroll
          for (int i = 0; i < kBatch; ++i) {
#pragma unroll
            for (int cb = 0; cb < Q; ++cb) {
              float t = 0.f;
#pragma unroll
              for (int ca = 0; ca < CPL; ++ca) t = __builtin_fmaf(rot[i][ca], gq[ca][cb], t);
              e[i] = __builtin_fmaf(t, d[i][4 * h + cb], e[i]);
            }
          }
        }
        src = row_ror1(src);
#pragma unroll
        for (int i = 0; i < kBatch; ++i)
#pragma unroll
          for (int c = 0; c < CPL; ++c) rot[i][c] = row_ror1(rot[i][c]);
      }
      // the row's sums of this batch, in the order of the candidates
#pragma unroll
      for (int i = 0; i < kBatch; ++i) {
        float s = e[i];
#pragma unroll
        for (int m = 1; m < 16; m <<= 1) s += __shfl_xor(s, m, 16);
        if (i0 + i == 0) e0 = s;
        if (i0 + i < p.nc && s < best) { best = s; bi = i0 + i; }
      }
    }

    if (live && l == 0) {
      const size_t o = (size_t)n * G + j;
      p.best_max[o] = org * p.shrink[bi];
      p.best_idx[o] = bi;
      p.err[2 * o] = e0;
      p.err[2 * o + 1] = best;
    }
  }
}

struct AwqQuantParams {
  const void *w;         // [N][K]
  const float *s;        // nullable, [K]
  const float *clip;     // nullable, [N][K/g]
  int32_t *codes;        // nullable, [K][N]
  float *scales, *zeros; // nullable, [N][K/g]
  void *wq;              // nullable, [N][K] in w's dtype
  int N, K, g;
  float maxq;
};

template <typename T, int CPL>
__global__ __launch_bounds__(256) void awq_quant_kernel(AwqQuantParams p) {
  constexpr int g = 16 * CPL;
  __shared__ int s_q[g * kRows];   // the group's codes, [column][row]: 16 consecutive int32 along N leave together
  const int tid = threadIdx.x, row = tid >> 4, l = tid & 15;
  const int N = p.N, K = p.K, G = K / g;
  const int n = blockIdx.x * kRows + row;
  const bool live = n < N;
  const float maxq = p.maxq;
  const T *wrow = (const T *)p.w + (size_t)(live ? n : 0) * K;

  for (int j = blockIdx.y; j < G; j += gridDim.y) {
    const float m = p.clip && live ? p.clip[(size_t)n * G + j] : 0.f;
    float v[CPL], s[CPL];
    float mn = 0.f, mx = 0.f;
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const int k = j * g + col_of<CPL>(l, c);
      s[c] = p.s ? p.s[k] : 1.f;
      v[c] = live ? to_f32(wrow[k]) : 0.f;
      if (p.s) v[c] = round_to<T>(v[c] * s[c]);
      if (p.clip) v[c] = fminf(fmaxf(v[c], -m), m);
      mn = c ? fminf(mn, v[c]) : v[c];
      mx = c ? fmaxf(mx, v[c]) : v[c];
    }
#pragma unroll
    for (int k = 1; k < 16; k <<= 1) { const MinMax r = minmax_xor({mn, mx}, k); mn = r.mn; mx = r.mx; }
    float sc, z;
    grid_of(mn, mx, maxq, sc, z);
    if (live && l == 0) {
      if (p.scales) p.scales[(size_t)n * G + j] = sc;
      if (p.zeros) p.zeros[(size_t)n * G + j] = z;
    }
    if (p.codes) __syncthreads();   // the previous group's codes have left
#pragma unroll
    for (int c = 0; c < CPL; ++c) {
      const float q = code_of(v[c], sc, z, maxq);
      if (p.codes) s_q[col_of<CPL>(l, c) * kRows + row] = (int)q;
      if (p.wq && live) from_f32((T *)p.wq + (size_t)n * K + j * g + col_of<CPL>(l, c), __fdiv_rn((q - z) * sc, s[c]));
    }
    if (p.codes) {
      __syncthreads();
      for (int idx = tid; idx < g * kRows; idx += 256) store_code(p.codes, s_q, idx, j * g, blockIdx.x * kRows, N);
    }
  }
}

bool awq_quant_shape_ok(int bits, int g) { return bits >= 2 && bits <= 8 && (g == 32 || g == 64 || g == 128); }

int awq_clip_candidates(int n_grid, float max_shrink) {
  if (n_grid < 1 || !(max_shrink > 0.f) || max_shrink > 1.f) return 0;
  const int nc = (int)((double)max_shrink * n_grid);
  return nc >= 1 && nc <= kCand ? nc : 0;
}

size_t awq_clip_search_workspace_bytes(int N, int K, int g) { return 0; }   // the search keeps everything in registers and LDS

namespace {

// enough blocks to fill the machine twice where the layer has them: a block walks every gy-th group
dim3 grid_of_layer(int N, int G) {
  const int tiles = (N + kRows - 1) / kRows;
  int gy = (2048 + tiles - 1) / tiles;
  gy = gy < 1 ? 1 : gy > G ? G : gy;
  return dim3(tiles, gy);
}

template <typename T> void launch_clip(const AwqClipParams &p, dim3 grid, hipStream_t stream) {
  if (p.g == 128) hipLaunchKernelGGL((awq_clip_kernel<T, 8>), grid, dim3(256), 0, stream, p);
  else if (p.g == 64) hipLaunchKernelGGL((awq_clip_kernel<T, 4>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((awq_clip_kernel<T, 2>), grid, dim3(256), 0, stream, p);
}

template <typename T> void launch_quant(const AwqQuantParams &p, dim3 grid, hipStream_t stream) {
  if (p.g == 128) hipLaunchKernelGGL((awq_quant_kernel<T, 8>), grid, dim3(256), 0, stream, p);
  else if (p.g == 64) hipLaunchKernelGGL((awq_quant_kernel<T, 4>), grid, dim3(256), 0, stream, p);
  else hipLaunchKernelGGL((awq_quant_kernel<T, 2>), grid, dim3(256), 0, stream, p);
}

}  // namespace

int launch_awq_clip_search(const void *w_nk, int w_dtype, const float *gram, int N, int K, int bits, int g, int n_grid, float max_shrink,
                           float *best_max, int32_t *best_idx, float *err, hipStream_t stream) {
  AwqClipParams p{};
  p.w = w_nk;
  p.gram = gram;
  p.best_max = best_max;
  p.best_idx = best_idx;
  p.err = err;
  p.N = N; p.K = K; p.g = g;
  p.nc = awq_clip_candidates(n_grid, max_shrink);
  p.maxq = maxq_of(bits);
  for (int i = 0; i < kCand; ++i) p.shrink[i] = (float)(1.0 - (double)i / (double)n_grid);
  const dim3 grid = grid_of_layer(N, K / g);
  with_w_type(w_dtype, [&](auto tag) { launch_clip<decltype(tag)>(p, grid, stream); });
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

int launch_awq_quantize(const void *w_nk, int w_dtype, const float *col_scale, const float *clip_ng, int N, int K, int bits, int g,
                        int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, hipStream_t stream) {
  AwqQuantParams p{};
  p.w = w_nk;
  p.s = col_scale;
  p.clip = clip_ng;
  p.codes = codes_kn;
  p.scales = scales_ng;
  p.zeros = zeros_ng;
  p.wq = wq_nk;
  p.N = N; p.K = K; p.g = g;
  p.maxq = maxq_of(bits);
  const dim3 grid = grid_of_layer(N, K / g);
  with_w_type(w_dtype, [&](auto tag) { launch_quant<decltype(tag)>(p, grid, stream); });
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
