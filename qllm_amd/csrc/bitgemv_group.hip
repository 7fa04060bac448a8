// bitgemv_group: the bit-stream matvec (bitgemv.hip) for up to four layers that read the SAME activations -- q/k/v, gate/up at 2, 5, 6, 7
// and 8 bits -- in ONE launch.  At these widths a decode matvec runs a handful of microseconds and every dependent launch boundary costs
// 1.7-1.9: seven launches per decoder layer become four.  The blocks of the members follow one another, widest
// member first; a block finds its member from the prefix sums at the head of the argument block, forms that member's BitGemvParams and
// runs bitgemv_kernel's body (bitgemv_kernel.hpp) with its block id counted from the member's first block.
//
// The contract: member i's output is bit-identical to qllm_linear_forward(w_i, x).  Every member therefore keeps exactly the K split its
// own single launch gets (bitgemv_split_for), its own chunking of x and its own counter and slab ranges of the one workspace -- a group
// is NOT split as if it were one wide layer, although that would fill the CUs with fewer blocks.  Where the workspace cannot hold all
// members' slabs, or the members' column blocks exceed the shared counter page, NO member splits: the call then equals the single calls
// made without a workspace.  Reached through qllm_linear_forward_bitgroup only: the planner, its routes and qllm_plan_describe do not
// know it.
#include <string.h>

#include <algorithm>

#include "bitgemv_kernel.hpp"
#include "planner.hpp"

namespace qllm {
namespace bg {

template <int BITS, int MT>
__global__ __launch_bounds__(kNW * 64) void bitgemv_group_kernel(const BitGemvGroupParams gp) {
  // block -> member: q/k/v and gate/up take two or one comparisons (the strip kernels' search, strip_kernel.hpp)
  const int b = (int)blockIdx.x;
  int pi = 0;
  if (gp.n_prob > 1) {
    pi = b >= gp.block_begin[1] ? 1 : 0;
    if (gp.n_prob > 2) {
      pi = b >= gp.block_begin[2] ? 2 : pi;
      if (gp.n_prob > 3) pi = b >= gp.block_begin[3] ? 3 : pi;
    }
  }
  // (indexed in the argument block itself, as the strip kernels index p.prob[i]: a uniform index into kernel-argument memory is a
  //  scalar load, not a private copy of the struct -- tests/test_bitgemv_group_cpu.py refuses scratch)
  const BitGemvGroupMember pr = gp.prob[pi];
  BitGemvParams p;
  p.x = gp.x;
  p.qweight = pr.qweight;
  p.scales = pr.scales;
  p.qzeros = pr.qzeros;
  p.bias = pr.bias;
  p.y = pr.y;
  p.slabs = pr.slabs;
  p.counters = pr.counters;
  p.M = gp.M;
  p.K = gp.K;
  p.N = pr.N;
  p.group_size = gp.group_size;
  p.zero_kind = pr.zero_kind;
  p.add_zero_bias = pr.add_zero_bias;
  p.act_bf16 = gp.act_bf16;
  p.ksplit = pr.ksplit;
  p.n_col_blocks = pr.n_col_blocks;
  p.chunk_units = pr.chunk_units;
  bitgemv_body<BITS, MT, false>(p, nullptr, (uint32_t)(b - gp.block_begin[pi]));
}

template <int BITS>
static int launch_g(const BitGemvGroupParams &gp, int mt, int grid, size_t lds, hipStream_t stream) {
#define QLLM_BG(MT_)                                                                                              \
  {                                                                                                               \
    static DeviceLatch attr_done; /* per (kernel, device): the LDS opt-in is a per-device attribute */              \
    if (int rc = lds_optin(attr_done, (const void *)bitgemv_group_kernel<BITS, MT_>)) return rc;                   \
    hipLaunchKernelGGL((bitgemv_group_kernel<BITS, MT_>), dim3(grid), dim3(kNW * 64), lds, stream, gp);           \
  }                                                                                                               \
  break
  switch (mt) {
    case 1: QLLM_BG(1);
    case 2: QLLM_BG(2);
    case 4: QLLM_BG(4);
    case 8: QLLM_BG(8);
    default: QLLM_BG(16);
  }
#undef QLLM_BG
  QLLM_HIP_CHECK(hipGetLastError());
  return QLLM_OK;
}

}  // namespace bg

// The launch geometry of a group (validated members that agree on K, M <= 16).  Member i's split is the one its single launch gets with
// a workspace of its own -- or 1 for EVERY member where `ws_bytes` cannot hold all slabs behind the counter page, or the members' column
// blocks exceed that page.  n_col_blocks / chunk_units / LDS come from bg::geometry, the function the single launch runs.
BitGroupGeom bitgemv_group_geometry(const qllm_weight_t *w, int n, int M, size_t ws_bytes) {
  BitGroupGeom g;
  memset(&g, 0, sizeof(g));
  g.mt = bg::row_tile(M);
  // widest first (stable: equal widths keep the caller's order)
  for (int i = 0; i < n; ++i) g.order[i] = i;
  for (int i = 1; i < n; ++i)
    for (int k = i; k > 0 && w[g.order[k]].N > w[g.order[k - 1]].N; --k) std::swap(g.order[k], g.order[k - 1]);
  size_t slab_bytes = 0;
  int col_blocks = 0;
  for (int i = 0; i < n; ++i) {
    g.split[i] = bitgemv_split_for(M, w[i].K, w[i].N, SIZE_MAX);
    slab_bytes += (size_t)g.split[i] * M * w[i].N * sizeof(float);
    col_blocks += (w[i].N + bg::kCols - 1) / bg::kCols;
  }
  g.slab_bytes = slab_bytes;
  if (ws_bytes < kCounterBytes + slab_bytes || col_blocks > (int)(kCounterBytes / sizeof(int)))
    for (int i = 0; i < n; ++i) g.split[i] = 1;
  static float slab_token;  // (non-NULL tokens, never dereferenced: bg::geometry drops the split of a call without slabs and counters)
  static int counter_token;
  int block = 0, counter = 0;
  size_t slab = 0;
  for (int k = 0; k < n; ++k) {
    const int i = g.order[k];
    BitGemvParams p;
    memset(&p, 0, sizeof(p));
    p.M = M;
    p.K = w[i].K;
    p.N = w[i].N;
    p.ksplit = g.split[i];
    p.slabs = &slab_token;
    p.counters = &counter_token;
    const bg::Geometry one = bg::geometry(p);
    g.n_col_blocks[i] = p.n_col_blocks;
    g.chunk_units[i] = p.chunk_units;
    g.block_begin[i] = block;
    g.counter_off[i] = counter;
    g.slab_off[i] = slab;
    block += one.grid;
    counter += p.n_col_blocks;
    slab += (size_t)g.split[i] * M * w[i].N * sizeof(float);
    g.lds = std::max(g.lds, one.lds);
  }
  g.grid = block;
  return g;
}

int launch_bitgemv_group(const BitGemvGroupParams &gp, const BitGroupGeom &g, int bits, hipStream_t stream) {
  switch (bits) {
    case 2: return bg::launch_g<2>(gp, g.mt, g.grid, g.lds, stream);
    case 3: return bg::launch_g<3>(gp, g.mt, g.grid, g.lds, stream);
    case 4: return bg::launch_g<4>(gp, g.mt, g.grid, g.lds, stream);
    case 5: return bg::launch_g<5>(gp, g.mt, g.grid, g.lds, stream);
    case 6: return bg::launch_g<6>(gp, g.mt, g.grid, g.lds, stream);
    case 7: return bg::launch_g<7>(gp, g.mt, g.grid, g.lds, stream);
    case 8: return bg::launch_g<8>(gp, g.mt, g.grid, g.lds, stream);
  }
  return set_error(QLLM_ERR_UNSUPPORTED, "bitgemv: bits must be 2..8 (got %d)", bits);
}

}  // namespace qllm
