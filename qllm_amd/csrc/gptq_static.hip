// GPTQ quantizer with static groups: GPTQ.fasterquant of qllm/quantization/gptq/gptq.py with static_groups=True (blocksize 128, mse=False,
// perchannel=True), in fp32, one launch per layer.  Every group's scale / zero is fixed from the ORIGINAL weights before the walk, the
// columns are still walked in the caller's processing order (act-order: descending diag(H)), and everything leaves in the original
// column order with the trivial g_idx[i] = i / group_size: act-order quality in a layer that decodes on the plain route.
//
// The decomposition is gptq_quant.hip's: 256 threads own 16 rows, 16 lanes own one row, each lane holds 8 of the 128 columns of the
// current block (two column quads), the trailing update is lazy ("left-looking") from the Err[N][K] workspace with the U tiles staged in
// LDS, and the arithmetic of a column (quantize, error, in-block update, loss) is that kernel's, rounding for rounding (this file is
// compiled with -ffp-contract=off).  What differs:
//   0. a pre-pass finds the parameters of every (row, group) over the original columns c*g .. c*g+g-1 and writes them to scales_ng /
//      zeros_ng, which ARE the table: the block reads its own rows back after a barrier.  (In LDS the table would be K/g * 16 rows * 8
//      bytes, 44 KB at K = 11008 and g = 32: one block per CU instead of the two that overlap the U loads.)
//   1. processing position j stands for the original column perm[j]: w is loaded from there, and codes / wq are stored there; the
//      workspace and U stay in processing order.
//   2. every one of a lane's 8 columns may belong to another group: eight (scale, zero) pairs per lane and block, looked up by column.
// Column indices from perm are clamped to 0..K-1: a perm that is no permutation gives a wrong result, never an access outside the arrays.
// u == NULL is round-to-nearest; the order of the walk then has no effect and perm is not consulted.  group_size == K: one set per row
// (what the reference's static path degenerates to, and what gptq_quant.hip computes for it).
// No block waits for another one: no grid-wide synchronisation, no atomics, bit-reproducible.
#include "quant_common.hpp"

namespace qllm {

namespace {

constexpr int kBlk = 128;    // the reference's blocksize (the order of the updates depends on it)
constexpr int kRows = 16;    // rows per thread block

// InternalGPTQQuantizer.find_params on the minimum / maximum of one row's group (both already taken against 0): gptq_quant.hip's
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

struct GptqStaticParams {
  const void *w;          // [N][K], original column order
  const float *u;         // nullable, [K][K] in processing order
  const int32_t *perm;    // nullable, [K]: processing position -> original column
  int32_t *codes;         // [K][N], original column order
  float *scales, *zeros;  // [N][K/g], original group numbering: output and the walk's table
  void *wq;               // nullable, [N][K] in w's dtype, original column order
  float *loss;            // nullable, [N]
  float *err;             // workspace: [N][K], processing order
  int N, K, g, gshift, sym;   // gshift: log2(g), 31 for group_size == K (every column in group 0)
  float maxq;
};

template <typename T>
__global__ __launch_bounds__(256) void gptq_static_kernel(GptqStaticParams p) {
  __shared__ __attribute__((aligned(16))) float s_u[kBlk][kBlk];    // U[p, b] during the trailing update, U[b, b] during the walk
  // Err_p of the tile's rows; after the walk: the block's codes, [column][row] (rows padded by four floats against bank conflicts)
  __shared__ __attribute__((aligned(16))) float s_e[kRows][kBlk + 4];
  const int tid = threadIdx.x, row = tid >> 4, l = tid & 15;
  const int N = p.N, K = p.K, g = p.g, G = K / g, gshift = p.gshift;
  const int n = blockIdx.x * kRows + row;
  const bool live = n < N, sym = p.sym != 0, has_u = p.u != nullptr;
  const float maxq = p.maxq;
  const T *wrow = (const T *)p.w + (size_t)(live ? n : 0) * K;
  const float *u = p.u;
  const int32_t *perm = has_u ? p.perm : nullptr;
  // the original column behind processing position j (j < K)
  auto column_of = [&](int j) { return perm ? min(max(perm[j], 0), K - 1) : j; };
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

  // 0. the table: the row's 16 lanes take one group at a time
  for (int c = 0; c < G; ++c) {
    float mn = 0.f, mx = 0.f;
    if (live)
      for (int j = l; j < g; j += 16) { const float v = to_f32(wrow[(size_t)c * g + j]); mn = fminf(mn, v); mx = fmaxf(mx, v); }
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) { const MinMax r = minmax_xor({mn, mx}, m); mn = r.mn; mx = r.mx; }
    float s, z;
    find_params(mn, mx, maxq, sym, s, z);
    if (live && l == 0) { p.scales[(size_t)n * G + c] = s; p.zeros[(size_t)n * G + c] = z; }
  }
  __syncthreads();   // (the row's other lanes read what lane 0 wrote)

  float loss = 0.f;
  for (int i1 = 0; i1 < K; i1 += kBlk) {
    const int count = K - i1 < kBlk ? K - i1 : kBlk;
    int col[8], oc[8];
    float w[8], sc[8], zr[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      col[r] = (r >> 2) * 64 + 4 * l + (r & 3);
      const bool here = live && col[r] < count;
      oc[r] = col[r] < count ? column_of(i1 + col[r]) : 0;
      w[r] = here ? to_f32(wrow[oc[r]]) : 0.f;
      const size_t o = (size_t)n * G + (oc[r] >> gshift);
      sc[r] = here ? p.scales[o] : 1.f;
      zr[r] = here ? p.zeros[o] : 0.f;
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

    // 2. the walk
    float qv[8], dq[8], er[8];
#pragma unroll
    for (int r = 0; r < 8; ++r) { qv[r] = 0.f; dq[r] = 0.f; er[r] = 0.f; }
    if (!has_u) {
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        qv[r] = fminf(fmaxf(rintf(__fdiv_rn(w[r], sc[r])) + zr[r], 0.f), maxq);
        dq[r] = sc[r] * (qv[r] - zr[r]);
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
            const float q = fminf(fmaxf(rintf(__fdiv_rn(x, sc[r])) + zr[r], 0.f), maxq);   // (only lane c's is column i's)
            const float y = sc[r] * (q - zr[r]);
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

    // 3. outputs of the block: wq to the original column, the error history by processing position, the codes through an LDS
    // transpose so that the 16 consecutive int32 along N of one column stay one store
    __syncthreads();
    int *s_q = (int *)&s_e[0][0];
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      s_q[col[r] * kRows + row] = (int)qv[r];
      if (live && col[r] < count) {
        if (p.wq) from_f32((T *)p.wq + (size_t)n * K + oc[r], dq[r]);
        if (has_u && i1 + kBlk < K) p.err[(size_t)n * K + i1 + col[r]] = er[r];
      }
    }
    __syncthreads();
    for (int idx = tid; idx < count * kRows; idx += 256) {
      const int nn = blockIdx.x * kRows + (idx & 15);
      if (nn < N) p.codes[(size_t)column_of(i1 + (idx >> 4)) * N + nn] = s_q[idx];
    }
  }
  if (p.loss) {
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) loss += __shfl_xor(loss, m, 16);
    if (live && l == 0) p.loss[n] = loss * 0.5f;
  }
}

int launch_gptq_quantize_static(const void *w_nk, int w_dtype, const float *u_kk, const int32_t *perm_k, int N, int K, int bits, int g, int sym,
                                int32_t *codes_kn, float *scales_ng, float *zeros_ng, void *wq_nk, float *loss_n, void *workspace,
                                hipStream_t stream) {
  GptqStaticParams p{};
  p.w = w_nk;
  p.u = u_kk;
  p.perm = perm_k;
  p.codes = codes_kn;
  p.scales = scales_ng;
  p.zeros = zeros_ng;
  p.wq = wq_nk;
  p.loss = loss_n;
  p.err = (float *)workspace;
  p.N = N; p.K = K; p.g = g; p.sym = sym;
  p.gshift = g == K ? 31 : g == 32 ? 5 : g == 64 ? 6 : 7;   // (gptq_quant_shape_ok: 32 / 64 / 128 / K)
  p.maxq = maxq_of(bits);
  const dim3 grid((N + kRows - 1) / kRows), block(256);
  with_w_type(w_dtype, [&](auto tag) { hipLaunchKernelGGL((gptq_static_kernel<decltype(tag)>), grid, block, 0, stream, p); });
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
