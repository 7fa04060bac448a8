// out[b, i, h, :] = softmax_j(scaling * q[b, h, i, :] . K[b, h / G, j, :] + mask[b, i, j]) V[b, h / G, j, :] for S = q_len >= 2 query rows per
// sequence against caches [B, Hkv, L_max, D] that ALREADY hold the S new rows and of which the first kv_len positions count: the attention
// core of a prompt, a continuation chunk or a padded batch (flash attention forward).  Query row i sits at absolute position
// q_start + i, q_start = kv_len - S.  There is no append form: the modules call `update` first, as the decode route does.
//
// Work split.  A block of 4 waves owns one (batch entry, query head, tile of kAttnPrefillQTile = 128 query rows), each wave 32 of the
// rows, and walks the keys in tiles of kAttnPrefillKvTile = 64.  There are B * Hq * ceil(S / 128) blocks, no split over the keys and no
// workspace.  The grid's x index counts the query tiles from the LAST one down, so the heavy tiles of a causal call are scheduled first.
//
// Data flow.  The 256 threads load a K tile and a V tile with 16-byte loads into registers (the next tile's loads are in flight while
// this one is computed: register staging) and write them as [key][D + 8] rows into LDS; rows at positions >= kv_len are written as
// zeros and never loaded.  Q stays in registers for the whole block as the B operand of S^T = K Q^T (mfma_f32_32x32x16: A = 32 keys x 16
// of D read by rows from LDS, B = 16 of D x 32 queries), so the 32 x 32 score tile has its QUERY on the lane and 16 of its keys in the
// lane's 16 registers (the other 16 in lane ^ 32).  The softmax statistics therefore live on the lane: the maximum needs one exchange
// with lane ^ 32 per key tile, the sum is kept per lane and the two halves are added once at the end.  Scores are fp32; the softmax is
// online, fp32, in the log2 domain.  P is rounded ONCE to the activation type and is, register for register, the B operand of
// O^T = V^T P^T: registers 8s .. 8s+7 are k-step s, and element j of lane half h is key 16s + 8(j >> 2) + 4h + (j & 3) of the tile.  V^T
// comes out of the row-major LDS image in exactly that key order with transposed reads (ds_read_b64_tr_b16: a 16-lane group reads 4 keys
// x 16 columns, lane i gets column i of the 4 keys), two per k-step.  O^T accumulates in fp32 with D on the registers and the query on the
// lane; at the end it is divided by the sum, rounded ONCE to the activation type and stored with 8-byte vector stores into the
// contiguous [B, S, Hq, D] output (what reshape turns into the o_proj input with no copy).
//
// Causality (causal = 1): key j is visible to row i only if j <= q_start + i.  A block reads no key tile wholly above its diagonal, and a
// wave skips the 32-key halves wholly above its own.  causal = 0: every j < kv_len counts.
// Mask (optional, in addition to causality): element (b, i, j) at mask + b * mask_batch + i * mask_row + j, bool bytes (non-zero =
// visible) or additive in the activation type; an additive value <= the type's lowest finite number hides the key exactly as a zero byte
// does.  It is read on every tile that is computed, at positions below kv_len only.  A row with no visible key stores zeros.  The running
// maximum starts at the finite floor kNoMax (attn_decode.hip's convention, with its bf16 caveat).
// Length: a host kv_len or an int64 read from device memory, clamped to S..L_max.  The launch shape never depends on it.  Positions >=
// kv_len are never loaded and count as zeros.  Keys hidden only by the mask or by causality ARE loaded (their weight is exactly 0): their
// K and V rows are assumed finite.
//
// Sliding window (window = W >= 1, causal only; 0: none; a variant of the kernel compiled beside the one without): row i sees key j only if
// q_start + i - W < j <= q_start + i, in addition to the length and the mask.  A block reads no key tile wholly below the window of its
// FIRST row (the mirror of `kend`), a wave skips the halves wholly below the window of its own first row, and inside computed tiles a key
// below a row's window gets weight exactly 0.  Later rows of a block meet tiles that are all hidden for them before their first visible
// key: the running maximum is then still kNoMax, every score is -inf, exp2(-inf - kNoMax) = 0 and the rescale factor is exp2(0) = 1,
// exactly as under a left-padding mask.  Keys hidden by the window inside a computed tile are loaded and assumed finite.
//
// Not built: a split over the keys for short q_len behind long caches, a ring-buffer cache, chunked attention, quantized and paged
// caches, rotary or the cache append inside the kernel, head_dim other than 64 / 128, dropout, the attention weights as an output, backward.
#include "attn_prefill_kernel.hpp"

namespace qllm {

// the kernels without a window are this unit's, those with one attn_prefill_window.hip's
int launch_attn_prefill(const AttnPrefillParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  if (p.window > 0) return launch_attn_prefill_window(p, head_dim, act_bf16, stream);
  return launch_attn_prefill_variant<false>(p, head_dim, act_bf16, stream);
}

}  // namespace qllm
