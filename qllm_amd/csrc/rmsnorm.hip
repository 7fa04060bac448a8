// y[M, K] = weight * round(x * rstd), rstd = rsqrt(mean(x^2) + eps) per row: the RMSNorm of the Llama family as ONE kernel (the eager
// module is about eight: to(float32), pow, mean, + eps, rsqrt, mul, to(dtype), weight *), with the eager expression's arithmetic step by
// step -- squares and their sum in fp32 (an fp16 / bf16 square is exact in fp32), rstd in fp32, h = x * rstd rounded to the activation
// type, y = weight * h in fp32 rounded again.  The standalone counterpart of the NORM forms of the batch-1 kernel (strip1_norm.hip):
// the modules use it wherever the fused entry does not serve a call (more rows, other kernels, the final norm).
//
// One block per row.  Every thread loads its 16-byte chunks of the row (chunk c = thread + NT u, u < CH) and of the weight ONCE and keeps
// them in registers across the reduction: the second read of the row is a register read for every K the entry takes (K <= 65536: 1024
// threads x 8 chunks; only there the weight is read behind the reduction, from cache), so y may alias x -- a chunk is read and written
// by the same thread only.  The reduction order is fixed by (NT, CH),
// i.e. by K alone: per thread chunk by chunk and element by element, per wave an xor butterfly, then the waves' partials in index order.
//
// The reference's counterpart is TritonLlamaRMSNorm (qllm/modeling/q_layers/triton_norm.py).
#include "strip1_kernel.hpp"

namespace qllm {

// WLATE (1024 threads x 8 chunks, K > 32768: 128 registers per thread): the weight's chunks are loaded behind the reduction instead of
// being held across it -- the vector is read by every row and sits in cache.
template <int NT, int CH, bool BF16, bool WLATE>
__global__ __launch_bounds__(NT) void rmsnorm_kernel(const uint4_t *x, const uint4_t *weight, uint4_t *y, int chunks, int K, float eps, float *rstd_out) {
  constexpr int NWV = NT / 64;
  __shared__ float part[NWV];
  const size_t row = (size_t)blockIdx.x * chunks;
  uint4_t xv[CH], wv[WLATE ? 1 : CH];
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int c = threadIdx.x + NT * u;
    xv[u] = uint4_t{0, 0, 0, 0};   // (chunks past the row: zeros, which add nothing)
    if constexpr (!WLATE) wv[u] = uint4_t{0, 0, 0, 0};
    if (c < chunks) {
      xv[u] = x[row + c];
      if constexpr (!WLATE) wv[u] = weight[c];
    }
  }
  float ss = 0.f;
#pragma unroll
  for (int u = 0; u < CH; ++u) ss += sumsq_chunk<BF16>(xv[u]);
#pragma unroll
  for (int off = 1; off < 64; off *= 2) ss += __shfl_xor(ss, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
  __syncthreads();
  float tot = part[0];
#pragma unroll
  for (int q = 1; q < NWV; ++q) tot += part[q];
  const float rstd = rms_rstd(tot, K, eps);
  if (rstd_out && threadIdx.x == 0) rstd_out[blockIdx.x] = rstd;
#pragma unroll
  for (int u = 0; u < CH; ++u) {
    const int c = threadIdx.x + NT * u;
    if (c < chunks) y[row + c] = norm_chunk<BF16>(xv[u], WLATE ? weight[c] : wv[WLATE ? 0 : u], rstd);
  }
}

template <int NT, int CH, bool WLATE = false>
static int launch_n(const void *x, const void *weight, void *y, int M, int K, float eps, int act_bf16, float *rstd_out, hipStream_t stream) {
  if (act_bf16)
    hipLaunchKernelGGL((rmsnorm_kernel<NT, CH, true, WLATE>), dim3(M), dim3(NT), 0, stream, (const uint4_t *)x, (const uint4_t *)weight, (uint4_t *)y, K / 8, K, eps, rstd_out);
  else
    hipLaunchKernelGGL((rmsnorm_kernel<NT, CH, false, WLATE>), dim3(M), dim3(NT), 0, stream, (const uint4_t *)x, (const uint4_t *)weight, (uint4_t *)y, K / 8, K, eps, rstd_out);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

// threads x chunks per thread by K alone (so the reduction order is a function of K): 256 threads up to K = 16384, 1024 above
int launch_rmsnorm(const void *x, const void *weight, void *y, int M, int K, float eps, int act_bf16, float *rstd_out, hipStream_t stream) {
  const int chunks = K / 8;
  if (chunks <= 256) return launch_n<256, 1>(x, weight, y, M, K, eps, act_bf16, rstd_out, stream);
  if (chunks <= 512) return launch_n<256, 2>(x, weight, y, M, K, eps, act_bf16, rstd_out, stream);
  if (chunks <= 1024) return launch_n<256, 4>(x, weight, y, M, K, eps, act_bf16, rstd_out, stream);
  if (chunks <= 2048) return launch_n<256, 8>(x, weight, y, M, K, eps, act_bf16, rstd_out, stream);
  if (chunks <= 4096) return launch_n<1024, 4>(x, weight, y, M, K, eps, act_bf16, rstd_out, stream);
  if (chunks <= 8192) return launch_n<1024, 8, true>(x, weight, y, M, K, eps, act_bf16, rstd_out, stream);
  return set_error(QLLM_ERR_UNSUPPORTED, "rmsnorm serves K <= %d (got %d)", kRmsNormMaxK, K);
}

}  // namespace qllm
