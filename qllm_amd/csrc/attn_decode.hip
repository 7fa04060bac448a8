// out = softmax(scaling * q K^T + mask) V for ONE query token per sequence against a cache [B, Hkv, L_max, D] of which the first kv_len
// positions count: the attention core of a decode step (flash-decoding).  transformers runs torch.cat (or five index kernels) for the cache
// update and sdpa over everything `update` returned -- with a StaticCache all max_cache_len positions behind a mask.
//
// Work split.  A block owns one (batch entry, kv head, split of the key positions) and ALL G = Hq / Hkv query heads of that kv head, so a
// K / V row is read once, not G times.  256 threads; D / 8 lanes share a position, each holding one 16-byte chunk of its K row and of its
// V row (loaded straight into registers, no LDS: the rows are streamed once and shared by nobody) and the matching chunk of the G query
// rows as fp32.  A wave load covers 64 / (D / 8) consecutive positions; a block step U = 4 such loads per wave: the tile, 64 positions at
// D = 128 and 128 at D = 64.  Scores: fp32 dot over the chunk, summed over the D / 8 lanes with DPP adds (all lanes get the sum),
// times scaling.  Softmax: online, fp32, in the log2 domain -- running maximum m, running sum l, unnormalised accumulator acc[G][8] per
// lane, one rescale per U positions.  P.V on the vector ALU with fp32 weights.  The lane groups of a wave merge their (m, l, acc) with
// xor shuffles, the four waves through LDS in wave order, and the block's result goes to the workspace in 16-byte stores.  The live
// splits of a (batch, kv head) take a ticket from its arrival counter behind an agent-scope release (strip1_body.inc); the last to
// arrive combines the splits IN SPLIT ORDER (runs of consecutive splits folded left to right side by side, then the runs in order),
// divides by l, rounds ONCE to the activation type, stores, and re-arms the counter: the same bits on every call.  With one live split
// the block stores directly.
//
// Launch shape.  Splits and grid follow (B, Hkv, L_max) and the CU count only (attn_decode_geom), never kv_len: a captured launch serves
// every length.  A block whose split lies beyond the length leaves at once: every block computes the number of live splits from the
// length, and the arrival counter counts those only.  kv_len is a host integer or an int64 in device
// memory.  Positions >= kv_len are NEVER loaded.
//
// Sliding window (window = W >= 1; 0: none; the WIN instantiations of the kernel, compiled in attn_decode_window.hip).  With n the
// number of counted positions (an append included) the query sits at n - 1 and sees positions lo = max(0, n - W) .. n - 1, W keys
// with its own, in addition to the length and the mask.  Positions < lo are NEVER
// loaded either: a split wholly below lo leaves at once like one beyond the length, the split that holds lo starts its walk AT lo, and
// the last block combines the splits from that one on in split order.  lo follows the length, so one captured launch serves lengths on
// both sides of the window; grid and splits do not depend on it.  A row whose keys inside the window are all masked stores zeros.
//
// Append.  With k_new / v_new, position kv_len is the new token: the lane group that owns that position reads the two rows from k_new /
// v_new, stores them into the caches and uses them; no other block touches that position.  If kv_len + 1 > L_max (only possible with the
// length on the device: the entry refuses it on the host) nothing is stored and the first L_max positions are attended.
//
// Mask: one row per batch entry, bool (true = visible) or additive in the activation type; an additive value <= the type's lowest finite
// number hides the key as false does.  A row with no visible key stores zeros.  The running maximum starts at the finite floor kNoMax, so
// a bf16 bias that is finite, above the lowest finite number and below about -7e29 has exp2(s - kNoMax) = 0: a row whose visible keys ALL
// carry such a bias stores zeros instead of a softmax among them (fp16 has no such value; transformers masks with finfo.min).
//
// Here position j lives in slot j; a ring-buffer cache (position j in slot j mod C) is attn_decode_ring.hip's.  Not built: chunked attention, quantized caches, paged caches, per-sequence lengths
// other than through the mask, head_dim other than 64 / 128, rotary inside the kernel, an fp8 cache, P.V on MFMA.  More than one query
// token: attn_prefill.hip.
#include "attn_decode_kernel.hpp"

namespace qllm {

// tile: positions per block step; splits: blocks per (batch, kv head), about two blocks per compute unit in all, at most kAttnDecodeMaxSplits
// and one per tile; chunk: positions per split, a multiple of the tile.  A function of the shapes and the CU count alone.
AttnDecodeGeom attn_decode_geom(int batch, int q_heads, int kv_heads, int head_dim, int64_t max_len) {
  AttnDecodeGeom g;
  g.tile = head_dim == 128 ? 64 : 128;
  const int64_t bh = (int64_t)batch * kv_heads, tiles = (max_len + g.tile - 1) / g.tile;
  int64_t want = (2 * (int64_t)compute_units() + bh - 1) / bh;
  if (want > kAttnDecodeMaxSplits) want = kAttnDecodeMaxSplits;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  g.chunk = (tiles + want - 1) / want * g.tile;
  g.splits = (int)((max_len + g.chunk - 1) / g.chunk);
  // the workspace: a bound on bh * splits that grows with the batch and with max_len (the split count itself shrinks as the batch grows)
  const int64_t most = tiles < kAttnDecodeMaxSplits ? tiles : kAttnDecodeMaxSplits;
  const int64_t rows = bh * most < 2 * (int64_t)compute_units() + bh ? bh * most : 2 * (int64_t)compute_units() + bh;
  g.partial_bytes = (size_t)rows * (q_heads / kv_heads) * (head_dim + 4) * sizeof(float);
  return g;
}

// the kernels without a window are this unit's, those with one attn_decode_window.hip's
int launch_attn_decode(const AttnDecodeParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  if (p.window > 0) return launch_attn_decode_window(p, head_dim, act_bf16, stream);
  return launch_attn_decode_variant<false>(p, head_dim, act_bf16, stream);
}

}  // namespace qllm
