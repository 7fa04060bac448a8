// out[b, i, h, :] = softmax_j(scaling * q[b, h, i, :] . K[b, h / G, j, :] + mask[b, i, j]) V[b, h / G, j, :] for a FEW query rows per sequence
// (S = q_len >= 2, G * S <= kAttnChunkMaxRows = 128) behind a long cache: the verify step of assisted generation, a continuation chunk.
// The call is attn_prefill.hip's without a window, to the letter: caches [B, Hkv, L_max, D] that ALREADY hold the S new rows, of which the
// first kv_len positions count; query row i at absolute position q_start + i, q_start = kv_len - S; `causal`; a mask that is none, bool
// or additive in the activation type at (b, i, j), applied in addition to causality; q with batch / head / row strides; the caches'
// three shared strides; kv_len from the host or an int64 on the device, clamped to S..L_max.  What differs is who does the work.
//
// attn_prefill launches B * Hq * ceil(S / 128) blocks: at batch 1, (32, 8, 128), that is 32 blocks on 256 compute units, each walking the
// whole cache alone, and the G heads of a kv head read the same K / V G times.  Here:
//
// Rows.  A block owns one (batch entry, kv head, split of the key positions) and ALL R = G * S query rows of that kv head, packed into one
// row space TOKEN-MAJOR: row r = i * G + g is token i of query head kvh * G + g.  The causal limit kv_len - S + i is then monotone in r, so
// a wave's 32 consecutive rows have one diagonal region and a wave skips the key tiles above the diagonal of its LAST row.  Rows are
// padded to 32: NT = ceil(R / 32) <= 4 row tiles, wave w < NT owns row tile w; padding rows compute on zeros and are never stored.
// Waves >= NT only stage.  The block stages each K / V tile ONCE for all G heads (the first saving).
//
// Data flow: attn_prefill.hip's frame.  All 256 threads load a 64-key K tile and V tile with 16-byte loads into registers (the next tile
// in flight while this one is computed) and write them as [key][D + 8] rows into LDS; rows at positions >= kv_len are written as zeros
// and never loaded.  Per wave S^T = K Q^T with mfma_f32_32x32x16, Q in registers for the whole walk, the row on the lane; fp32 scores; an
// fp32 online softmax in the log2 domain with per-lane statistics (one exchange with lane ^ 32 per key tile for the maximum, the two
// halves of the sum added once at the end); P rounded ONCE to the activation type and used, register for register, as the B operand of
// O^T = V^T P^T, V^T through ds_read_b64_tr_b16; O^T accumulates in fp32.
//
// Split over the keys (the second saving).  attn_chunk_geom: key tile 64; about two blocks per compute unit over B * Hkv, at most
// kAttnDecodeMaxSplits, at most one per tile; the chunk a multiple of the tile.  A function of (B, Hq, Hkv, D, S, L_max) and the CU count
// only, never of kv_len: a captured launch serves every length.  Every block computes the number of live splits, ceil(kv_len / chunk),
// from the length; a block whose split starts at or beyond the length leaves at once.
//
// Hand-off and combine: attn_decode_body.inc's protocol.  Per row (m, l) and the unnormalised fp32 O[D] go to the workspace in 16-byte
// vector stores; every wave drains its stores; one lane issues an agent-scope release and a relaxed agent-scope atomicAdd on the (batch
// entry, kv head)'s counter in the counter page; the last block to arrive issues an agent-scope acquire, combines the live splits IN
// SPLIT ORDER (a thread folds one row's 8 columns from left to right), divides by l, rounds ONCE, stores into the contiguous
// [B, S, Hq, D] output and re-arms the counter to zero: the same bits on every call.  With one live split the block stores directly.  A
// split in which a row sees no key (it lies above the row's diagonal, or the mask hides it) hands over m = kNoMax, l = 0, O = 0 and
// combines as weight 0; a row with no visible key anywhere stores zeros.  Every store is a plain vector store.
//
// Keys hidden only by the mask or by causality ARE loaded (their weight is exactly 0): their K and V rows are assumed finite.
//
// Not built: a sliding window; ring and sliding caches read directly (a quantized one: attn_chunk_quant.hip); the cache append inside the kernel; a 16-row MFMA tile
// for R <= 16 (a 32-row tile is then at least half padding); R > 128; waves over key sub-ranges when NT = 1 (three of the four waves
// then only stage); skipping, in the combine, the splits above a row's diagonal.
#include "attn_chunk_kernel.hpp"

namespace qllm {

// rows: G * q_len; row_tiles: ceil(rows / 32); splits: blocks per (batch, kv head), about two blocks per compute unit in all, at most
// kAttnDecodeMaxSplits and one per key tile; chunk: positions per split, a multiple of the tile.  A function of the shapes and the CU
// count alone (attn_decode_geom's manner).
AttnChunkGeom attn_chunk_geom(int batch, int q_heads, int kv_heads, int head_dim, int q_len, int64_t max_len) {
  AttnChunkGeom g;
  g.rows = q_heads / kv_heads * q_len;
  g.row_tiles = (g.rows + 31) / 32;
  const int64_t bh = (int64_t)batch * kv_heads, tiles = (max_len + kAttnChunkKvTile - 1) / kAttnChunkKvTile;
  int64_t want = (2 * (int64_t)compute_units() + bh - 1) / bh;
  if (want > kAttnDecodeMaxSplits) want = kAttnDecodeMaxSplits;
  if (want > tiles) want = tiles;
  if (want < 1) want = 1;
  g.chunk = (tiles + want - 1) / want * kAttnChunkKvTile;
  g.splits = (int)((max_len + g.chunk - 1) / g.chunk);
  // the workspace: a bound on bh * splits that grows with the batch and with max_len (the split count itself shrinks as the batch grows)
  const int64_t most = tiles < kAttnDecodeMaxSplits ? tiles : kAttnDecodeMaxSplits;
  const int64_t blocks = bh * most < 2 * (int64_t)compute_units() + bh ? bh * most : 2 * (int64_t)compute_units() + bh;
  g.partial_bytes = (size_t)blocks * g.rows * (head_dim + 4) * sizeof(float);
  return g;
}

int launch_attn_chunk(const AttnChunkParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  return launch_attn_chunk_kernels(p, head_dim, act_bf16, stream);
}

}  // namespace qllm
