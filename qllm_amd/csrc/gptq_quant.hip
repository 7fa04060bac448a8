// GPTQ quantizer: fp16 / bf16 / fp32 W[N,K] + the upper Cholesky factor U[K,K] of H^-1 -> integer codes, per-group scale / zero, the
// dequantized weights and the per-row loss: GPTQ.fasterquant of qllm/quantization/gptq/gptq.py (blocksize 128, static_groups=False,
// mse=False, perchannel=True) with the quantizer of _gptq_quantizer.py, in fp32, the whole column walk of a layer in ONE launch.
//
// Rows are independent.  A block of 256 threads owns 16 rows through all K columns; 16 lanes own one row and each lane holds 8 of the
// 128 columns of the current column block in registers (columns 4l..4l+3 and 64+4l..64+4l+3: both LDS reads of a row of U are then 256
// contiguous bytes per 16 lanes).  Per 128-column block b:
//   1. lazy trailing update ("left-looking"): w = W[:, block b]; for every earlier block p in order: w -= Err_p(16x128) . U[p, b](128x128).
//      U[p, b] is staged in LDS (64 KB), Err_p comes back from the workspace (each row tile reads only what it wrote itself).  This is
//      the reference's W[:, i2:] -= Err1.matmul(Hinv[i1:i2, i2:]) applied when the columns are needed instead of when the errors are
//      made: the same partial sums subtracted in the same order, and W needs no fp32 working copy -- the workspace holds Err[N,K].
//   2. group parameters from that block-boundary state (groups of 32 / 64 / 128 lie inside one block; group_size == K: from the
//      original row, before the first block).
//   3. the in-block walk with the diagonal block U[b, b] in LDS: column i is quantized by its owner lane, err = (w - q) / U[i,i] goes to
//      the row's 16 lanes by a lane shuffle, and every later column of the block gets w[j] -= err * U[i,j] at once (a product and a
//      difference, two roundings: this file is compiled with -ffp-contract=off).
//   4. codes leave through an LDS transpose ([column][16 rows]) so that 16 consecutive int32 along N are stored together.
// No block waits for another one: no grid-wide synchronisation, no atomics, bit-reproducible.  u == NULL skips 1 and 3: round-to-nearest
// on the same grid.
#include "quant_common.hpp"

namespace qllm {

namespace {

constexpr int kBlk = 128;    // the reference's blocksize: when group parameters are found depends on it, so it is semantics
constexpr int kRows = 16;    // rows per thread block

// InternalGPTQQuantizer.find_params on the minimum / maximum of one row's group (both already taken against 0)
__device__ __forceinline__ void find_params(float xmin, float xmax, float maxq, bool sym, float &scale, float &zero) {
  if (sym) {
    xmax = fmaxf(fabsf(xmin), xmax);
    if (xmin < 0.f) xmin = -xmax;
  }
  if (xmin == 0.f && xmax == 0.f) { xmin = -1.f; xmax = 1.f; }
  scale = __fdiv_rn(xmax - xmin, maxq);
  zero = sym ? (maxq + 1.f) * 0.5f : rintf(__fdiv_rn(-xmin, scale));
}

}  // namespace

struct GptqQuantParams {
  const void *w;
  const float *u;     // nullable
  int32_t *codes;     // [K][N]
  float *scales, *zeros;  // [N][K/g]
  void *wq;           // nullable, [N][K] in w's dtype
  float *loss;        // nullable, [N]
  float *err;         // workspace: [N][K]
  int N, K, g, sym;
  float maxq;
};

template <typename T>
__global__ __launch_bounds__(256) void gptq_quant_kernel(GptqQuantParams p) {
  __shared__ __attribute__((aligned(16))) float s_u[kBlk][kBlk];    // U[p, b] during the trailing update, U[b, b] during the walk
  // Err_p of the tile's rows; after the walk: the block's codes, [column][row].  Rows are padded by four floats: the four rows of a
  // wave read the same k at once, and a 512-byte stride would put them on the same banks.
  __shared__ __attribute__((aligned(16))) float s_e[kRows][kBlk + 4];
  const int tid = threadIdx.x, row = tid >> 4, l = tid & 15;
  const int N = p.N, K = p.K, g = p.g, G = K / g;
  const int n = blockIdx.x * kRows + row;
  const bool live = n < N, sym = p.sym != 0, row_mode = g == K, has_u = p.u != nullptr;
  const float maxq = p.maxq;
  const T *wrow = (const T *)p.w + (size_t)(live ? n : 0) * K;
  const float *u = p.u;
  // a 128 x 128 tile of U, rows r0.., columns c0.., into s_u, 16 bytes at a time (K % 4 == 0 and an aligned u: the launcher sees to it;
  // every tile starts at a multiple of 128 columns); rows >= nrow and columns >= ncol (multiples of 4) are 0
  auto stage_u = [&](int r0, int c0, int nrow, int ncol) {
    for (int idx = tid; idx < kBlk * (kBlk / 4); idx += 256) {
      const int k = idx >> 5, c = (idx & 31) * 4;
      float4 v = {0.f, 0.f, 0.f, 0.f};
      if (k < nrow && c < ncol) v = *(const float4 *)&u[(size_t)(r0 + k) * K + c0 + c];
      *(float4 *)&s_u[k][c] = v;
    }
  };

  float rs = 1.f, rz = 0.f;   // group_size == K: one set per row, from the original W
  if (row_mode) {
    float mn = 0.f, mx = 0.f;
    if (live)
      for (int j = l; j < K; j += 16) { const float v = to_f32(wrow[j]); mn = fminf(mn, v); mx = fmaxf(mx, v); }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const MinMax r = minmax_xor({mn, mx}, m); mn = r.mn; mx = r.mx; }
    find_params(mn, mx, maxq, sym, rs, rz);
    if (live && l == 0) { p.scales[n] = rs; p.zeros[n] = rz; }
  }

  float loss = 0.f;
  for (int i1 = 0; i1 < K; i1 += kBlk) {
    const int count = K - i1 < kBlk ? K - i1 : kBlk;
    int col[8];
    float w[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      col[r] = (r >> 2) * 64 + 4 * l + (r & 3);
      w[r] = live && col[r] < count ? to_f32(wrow[i1 + col[r]]) : 0.f;   // absent columns: 0 is neutral for min / max against 0
    }
    if (has_u) {
      // 1. the updates of every earlier block, in the reference's order
      for (int p1 = 0; p1 < i1; p1 += kBlk) {
        __syncthreads();
        stage_u(p1, i1, kBlk, count);
        for (int idx = tid; idx < kRows * kBlk; idx += 256) {
          const int r = idx >> 7, k = idx & 127, nn = blockIdx.x * kRows + r;
          s_e[r][k] = nn < N ? p.err[(size_t)nn * K + p1 + k] : 0.f;
        }
        __syncthreads();
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 2
        for (int k4 = 0; k4 < kBlk; k4 += 4) {
          const float4 e4 = *(const float4 *)&s_e[row][k4];
          const float e[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
          for (int kk = 0; kk < 4; ++kk) {
            const float4 a = *(const float4 *)&s_u[k4 + kk][4 * l], b = *(const float4 *)&s_u[k4 + kk][64 + 4 * l];
            acc[0] += e[kk] * a.x; acc[1] += e[kk] * a.y; acc[2] += e[kk] * a.z; acc[3] += e[kk] * a.w;
            acc[4] += e[kk] * b.x; acc[5] += e[kk] * b.y; acc[6] += e[kk] * b.z; acc[7] += e[kk] * b.w;
          }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) w[r] -= acc[r];
      }
      __syncthreads();
      stage_u(i1, i1, count, count);
    }

    // 2. group parameters of the lane's two column quads (h = 0: columns < 64, h = 1: columns >= 64)
    float sc[2] = {rs, rs}, zr[2] = {rz, rz};
    if (!row_mode) {
      float mn[2], mx[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        mn[h] = fminf(fminf(fminf(w[4 * h], w[4 * h + 1]), fminf(w[4 * h + 2], w[4 * h + 3])), 0.f);
        mx[h] = fmaxf(fmaxf(fmaxf(w[4 * h], w[4 * h + 1]), fmaxf(w[4 * h + 2], w[4 * h + 3])), 0.f);
#pragma unroll
        for (int m = 1; m < 8; m <<= 1) { const MinMax r = minmax_xor({mn[h], mx[h]}, m); mn[h] = r.mn; mx[h] = r.mx; }
        if (g >= 64) { const MinMax r = minmax_xor({mn[h], mx[h]}, 8); mn[h] = r.mn; mx[h] = r.mx; }
      }
      if (g == 128) { mn[0] = mn[1] = fminf(mn[0], mn[1]); mx[0] = mx[1] = fmaxf(mx[0], mx[1]); }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        find_params(mn[h], mx[h], maxq, sym, sc[h], zr[h]);
        const int c0 = g == 32 ? 64 * h + 32 * (l >> 3) : 64 * h;   // first column of the lane's group in this block
        const bool writer = g == 32 ? (l & 7) == 0 : (l == 0 && (g == 64 || h == 0));
        if (live && writer && c0 < count) {
          const size_t o = (size_t)n * G + (i1 + c0) / g;
          p.scales[o] = sc[h];
          p.zeros[o] = zr[h];
        }
      }
    }

    // 3. the walk
    float qv[8], dq[8], er[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { qv[r] = 0.f; dq[r] = 0.f; er[r] = 0.f; }
    if (!has_u) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        qv[r] = fminf(fmaxf(rintf(__fdiv_rn(w[r], sc[r >> 2])) + zr[r >> 2], 0.f), maxq);
        dq[r] = sc[r >> 2] * (qv[r] - zr[r >> 2]);
        const float d = w[r] - dq[r];
        if (col[r] < count) loss += d * d;
      }
    } else {
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        for (int c = 0; c < 16; ++c) {
          if (64 * h + 4 * c >= count) break;   // (uniform: a ragged last block)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int i = 64 * h + 4 * c + r4, r = 4 * h + r4;
            if (i >= count) continue;
            const float d = s_u[i][i];
            const float x = w[r];
            const float q = fminf(fmaxf(rintf(__fdiv_rn(x, sc[h])) + zr[h], 0.f), maxq);
            const float y = sc[h] * (q - zr[h]);
            const float diff = x - y;
            const float ev = __fdiv_rn(diff, d);
            if (l == c) {
              qv[r] = q; dq[r] = y; er[r] = ev;
              loss += __fdiv_rn(diff * diff, d * d);
            }
            const float e = __shfl(ev, c, 16);
            const float4 b = *(const float4 *)&s_u[i][64 + 4 * l];
            if (h == 0) {
              const float4 a = *(const float4 *)&s_u[i][4 * l];
              const float ua[4] = {a.x, a.y, a.z, a.w};
#pragma unroll
              for (int rr = 0; rr < 4; ++rr)
                if (l > c || (l == c && rr > r4)) w[rr] -= e * ua[rr];
              w[4] -= e * b.x; w[5] -= e * b.y; w[6] -= e * b.z; w[7] -= e * b.w;
            } else {
              const float ub[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
              for (int rr = 0; rr < 4; ++rr)
                if (l > c || (l == c && rr > r4)) w[4 + rr] -= e * ub[rr];
            }
          }
        }
      }
    }

    // 4. outputs of the block
    __syncthreads();
    int *s_q = (int *)&s_e[0][0];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      s_q[col[r] * kRows + row] = (int)qv[r];
      if (live && col[r] < count) {
        const size_t o = (size_t)n * K + i1 + col[r];
        if (p.wq) from_f32((T *)p.wq + o, dq[r]);
        if (has_u && i1 + kBlk < K) p.err[o] = er[r];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < count * kRows; idx += 256) store_code(p.codes, s_q, idx, i1, blockIdx.x * kRows, N);
  }
  if (p.loss) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) loss += __shfl_xor(loss, m, 16);
    if (live && l == 0) p.loss[n] = loss * 0.5f;
  }
}

bool gptq_quant_shape_ok(int K, int bits, int g) {
  return bits >= 2 && bits <= 8 && (g == 32 || g == 64 || g == 128 || g == K);
}

size_t gptq_quant_workspace_bytes(int N, int K) {
  if (N <= 0 || K <= 0) return 0;
  return ((size_t)N * (size_t)K * sizeof(float) + 255) / 256 * 256;   // Err[N][K]
}

int launch_gptq_quantize(const void *w_nk, int w_dtype, const float *u_kk, int N, int K, int bits, int g, int sym, int32_t *codes_kn,
                         float *scales_ng, float *zeros_ng, void *wq_nk, float *loss_n, void *workspace, hipStream_t stream) {
  GptqQuantParams p{};
  p.w = w_nk;
  p.u = u_kk;
  p.codes = codes_kn;
  p.scales = scales_ng;
  p.zeros = zeros_ng;
  p.wq = wq_nk;
  p.loss = loss_n;
  p.err = (float *)workspace;
  p.N = N; p.K = K; p.g = g; p.sym = sym;
  p.maxq = maxq_of(bits);
  const dim3 grid((N + kRows - 1) / kRows), block(256);
  with_w_type(w_dtype, [&](auto tag) { hipLaunchKernelGGL((gptq_quant_kernel<decltype(tag)>), grid, block, 0, stream, p); });
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
