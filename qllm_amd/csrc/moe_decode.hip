// The routed experts of a sparse MoE block (Mixtral's block_sparse_moe.experts, Qwen3-MoE's mlp.experts) for T = 1..4 tokens as TWO
// launches, whatever the routing, with nothing going back to the host:
//
//   A  h[slot] = act(x[t] . W_gate[e]) * (x[t] . W_up[e])        slot = t * top_k + j,  e = ids[slot]
//   B  y[t]    = sum_j round(round(h[slot] . W_down[e]) * w[slot])   in ascending expert id
//
// where the family's own loop (one_hot, nonzero -- a host synchronisation per layer --, then per hit expert three GEMMs and about six
// elementwise kernels, then index_add_) cannot be captured in a graph at all.  Format, lane layout and arithmetic of a group:
// moe_decode_kernel.hpp.
//
// Kernel A.  grid (I / 16 strips, T * top_k slots), 8 waves.  A block loads its slot's expert id -- the one dependent load, issued
// first, behind only the loads of x[t], which need nothing -- forms both strip addresses and computes the gate strip and the up strip of
// the SAME 16 columns over all of K = H: wave w takes groups w, w + 8, ..; each lane issues the loads of up to four groups of both
// matrices (14 loads) before its first wait.  x[t] goes through LDS once per block, converted to fp16 and in the pair order of the weight
// words, and serves both matrices.  Lanes sum over their word rows by four xor steps, waves meet in LDS, and eight threads form
// act(g) * u of two columns each with the eager roundings: g and u to the activation type, then swiglu_pair's two.  g and u never
// reach memory.  A slot whose id is outside [0, E) (transformers' masked-expert sentinel is E) leaves at once: its row of h is neither
// written nor, in kernel B, read.
//
// Kernel B.  grid (H / 16 strips, T tokens), 16 waves.  A block owns its 16 output columns for ALL top_k slots of its token: the
// concatenated (slot, group of I) range is cut into 16 equal runs, so Mixtral's 2 x 112 groups and Qwen3-30B-A3B's 8 x 6 keep the same
// number of waves busy.  A lane's h chunk comes straight from memory with the group's weight loads (top_k * I halves can exceed LDS, and
// each chunk is used by one wave only).  A wave's run crosses at most a few slot boundaries; at each it reduces its four columns over its
// word rows and writes red[slot][wave][16] in LDS (zeroed first: a wave that never saw a slot adds 0).  Then thread (slot, column) sums
// the 16 waves in index order, rounds to the activation type, multiplies by the routing weight in fp32 and rounds again; 16 threads add
// the slots' values in ASCENDING EXPERT ID, one rounding per add, starting from +0 -- the order and the roundings of the family's
// index_add_ loop.  One store per output, no atomics, no workspace: the same bits on every call.
#include "kernels.hpp"
#include "moe_decode_kernel.hpp"

namespace qllm {

template <bool BF16>
__global__ __launch_bounds__(kMoeThreadsA) void moe_gate_up_kernel(const MoeGateUpParams p) {
  extern __shared__ uint4_t moe_lds[];            // x[t]: H / 8 chunks | red[wave][gate, up][16] floats
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int slot = blockIdx.y, strip = blockIdx.x;
  const int G = p.H >> 7, NS = p.I >> 4, nchunks = p.H >> 3;
  float *red = (float *)(moe_lds + nchunks);

  const uint4_t *xrow = (const uint4_t *)p.x + (int64_t)(slot / p.top_k) * nchunks;
  uint4_t xv[kMoeXChunks];
#pragma unroll
  for (int i = 0; i < kMoeXChunks; ++i)
    if (tid + i * kMoeThreadsA < nchunks) xv[i] = xrow[tid + i * kMoeThreadsA];
  const int64_t e = p.ids[slot];
  if (e < 0 || e >= p.E) return;                  // (the whole block: e is the block's)

  MoeGroup mg[kMoeRound], mu[kMoeRound];
  auto load_round = [&](int g0) {
#pragma unroll
    for (int j = 0; j < kMoeRound; ++j) {
      const int g = g0 + j * kMoeWavesA;
      if (g < G) {
        mg[j] = moe_load_group(p.gq, p.gs, p.gz, e, NS, strip, G, g, lane);
        mu[j] = moe_load_group(p.uq, p.us, p.uz, e, NS, strip, G, g, lane);
      }
    }
  };
  float ag[4] = {0.f, 0.f, 0.f, 0.f}, au[4] = {0.f, 0.f, 0.f, 0.f};
  auto consume_round = [&](int g0) {
#pragma unroll
    for (int j = 0; j < kMoeRound; ++j) {
      const int g = g0 + j * kMoeWavesA;
      if (g < G) {
        const uint4_t xp = moe_lds[g * 16 + (lane >> 2)];
        moe_consume(mg[j], xp, lane, p.add_zero_bias, ag);
        moe_consume(mu[j], xp, lane, p.add_zero_bias, au);
      }
    }
  };

  load_round(wave);
#pragma unroll
  for (int i = 0; i < kMoeXChunks; ++i)
    if (tid + i * kMoeThreadsA < nchunks) moe_lds[tid + i * kMoeThreadsA] = moe_x_pairs<BF16>(xv[i]);
  __syncthreads();
  consume_round(wave);
  for (int g0 = wave + kMoeRound * kMoeWavesA; g0 < G; g0 += kMoeRound * kMoeWavesA) {
    load_round(g0);
    consume_round(g0);
  }

#pragma unroll
  for (int c = 0; c < 4; ++c) {
    ag[c] = moe_rows_sum(ag[c]);
    au[c] = moe_rows_sum(au[c]);
  }
  if (lane < 4) {
    *(float4_t *)(red + wave * 32 + lane * 4) = float4_t{ag[0], ag[1], ag[2], ag[3]};
    *(float4_t *)(red + wave * 32 + 16 + lane * 4) = float4_t{au[0], au[1], au[2], au[3]};
  }
  __syncthreads();
  if (tid < 8) {                                  // columns 2 tid, 2 tid + 1
    float g0 = 0.f, g1 = 0.f, u0 = 0.f, u1 = 0.f;
#pragma unroll
    for (int w = 0; w < kMoeWavesA; ++w) {
      g0 += red[w * 32 + 2 * tid];
      g1 += red[w * 32 + 2 * tid + 1];
      u0 += red[w * 32 + 16 + 2 * tid];
      u1 += red[w * 32 + 16 + 2 * tid + 1];
    }
    const uint32_t g2 = (uint32_t)moe_bits<BF16>(g0) | ((uint32_t)moe_bits<BF16>(g1) << 16);
    const uint32_t u2 = (uint32_t)moe_bits<BF16>(u0) | ((uint32_t)moe_bits<BF16>(u1) << 16);
    ((uint32_t *)p.h)[((int64_t)slot * p.I + strip * 16) / 2 + tid] = swiglu_pair<BF16>(g2, u2);
  }
}

template <bool BF16>
__global__ __launch_bounds__(kMoeThreadsB) void moe_down_kernel(const MoeDownParams p) {
  __shared__ float red[kMoeMaxTopK * kMoeWavesB * 16];
  __shared__ float val[kMoeMaxTopK * 16];
  __shared__ int eid[kMoeMaxTopK];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t = blockIdx.y, strip = blockIdx.x;
  const int G = p.I >> 7, NS = p.H >> 4, top_k = p.top_k;

  if (tid < top_k) {
    const int64_t e = p.ids[t * top_k + tid];
    eid[tid] = (e >= 0 && e < p.E) ? (int)e : -1;
  }
  for (int i = tid; i < top_k * kMoeWavesB * 16; i += kMoeThreadsB) red[i] = 0.f;
  __syncthreads();

  // this wave's run [c0, c1) of the concatenated (slot, group) range
  const int total = top_k * G, per = (total + kMoeWavesB - 1) / kMoeWavesB;
  const int c0 = wave * per, c1 = min(total, c0 + per);
  const uint4_t *hrows = (const uint4_t *)p.h + (int64_t)t * top_k * (p.I >> 3);
  int cur = -1;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  auto flush = [&]() {
    if (cur >= 0) {
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = moe_rows_sum(acc[c]);
      if (lane < 4) *(float4_t *)(red + (cur * kMoeWavesB + wave) * 16 + lane * 4) = float4_t{acc[0], acc[1], acc[2], acc[3]};
    }
  };
  for (int cb = c0; cb < c1; cb += kMoeRound) {
    MoeGroup m[kMoeRound];
    uint4_t hv[kMoeRound];
    int sl[kMoeRound];
#pragma unroll
    for (int j = 0; j < kMoeRound; ++j) {
      const int c = cb + j;
      sl[j] = -1;
      if (c < c1) {
        const int s = c / G, g = c - s * G, e = eid[s];
        if (e >= 0) {
          sl[j] = s;
          m[j] = moe_load_group(p.dq, p.ds, p.dz, e, NS, strip, G, g, lane);
          hv[j] = hrows[(int64_t)s * (p.I >> 3) + g * 16 + (lane >> 2)];
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kMoeRound; ++j) {
      if (sl[j] >= 0) {                           // (wave-uniform)
        if (sl[j] != cur) {
          flush();
          cur = sl[j];
          acc[0] = acc[1] = acc[2] = acc[3] = 0.f;
        }
        moe_consume(m[j], moe_x_pairs<BF16>(hv[j]), lane, p.add_zero_bias, acc);
      }
    }
  }
  flush();
  __syncthreads();

  if (tid < top_k * 16) {                         // thread (slot, column): round(round(d) * w)
    const int s = tid >> 4, col = tid & 15;
    float d = 0.f;
#pragma unroll
    for (int w = 0; w < kMoeWavesB; ++w) d += red[(s * kMoeWavesB + w) * 16 + col];
    float wt;
    if (p.weights_f32) wt = ((const float *)p.weights)[t * top_k + s];
    else if constexpr (BF16) wt = __builtin_bit_cast(float, (uint32_t)((const uint16_t *)p.weights)[t * top_k + s] << 16);
    else wt = (float)((const half_t *)p.weights)[t * top_k + s];
    // the product is an fp32 value that is rounded again, as eager rounds it: the empty asm keeps hipcc from folding the multiply and the
    // conversion into one v_fma_mixlo_f16, which rounds the exact product once (a different fp16 where the fp32 product lands on a tie)
    float prod = moe_round<BF16>(d) * wt;
    asm volatile("" : "+v"(prod));
    val[tid] = moe_round<BF16>(prod);
  }
  __syncthreads();
  if (tid < 16) {                                 // ascending expert id (equal ids: ascending slot), one rounding per add, from +0
    float y = 0.f;
    int last = -1;
    for (int n = 0; n < top_k; ++n) {
      int best = 0x7fffffff, bs = -1;
      for (int s = 0; s < top_k; ++s) {
        const int key = eid[s] * kMoeMaxTopK + s;
        if (eid[s] >= 0 && key > last && key < best) best = key, bs = s;
      }
      if (bs < 0) break;
      last = best;
      y = moe_round<BF16>(y + val[bs * 16 + tid]);
    }
    ((uint16_t *)p.y)[(int64_t)t * p.H + strip * 16 + tid] = moe_bits<BF16>(y);
  }
}

// shapes, ranges, types and alignment: checked by the entries (capi.hip, check_moe)
int launch_moe_gate_up(const MoeGateUpParams &p0, int T, int act_bf16, hipStream_t stream) {
  MoeGateUpParams p = p0;
  if (!p.gz || !p.uz) p.add_zero_bias = 0;        // (the symmetric grid has no stored zero point to offset)
  const size_t lds = (size_t)p.H * 2 + kMoeWavesA * 32 * sizeof(float);
  auto kernel = act_bf16 ? moe_gate_up_kernel<true> : moe_gate_up_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(p.I / 16, T * p.top_k), dim3(kMoeThreadsA), lds, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

int launch_moe_down(const MoeDownParams &p0, int T, int act_bf16, hipStream_t stream) {
  MoeDownParams p = p0;
  if (!p.dz) p.add_zero_bias = 0;
  auto kernel = act_bf16 ? moe_down_kernel<true> : moe_down_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3(p.H / 16, T), dim3(kMoeThreadsB), 0, stream, p);
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace qllm
