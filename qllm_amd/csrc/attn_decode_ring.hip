// The decode attention kernel over a RING-BUFFER cache (attn_decode.hip has the text of the kernel, attn_decode_kernel.hpp the code): what
// a sliding-window layer needs once its window is full, without moving a row.  A unit of its own, and kernels of a name of their own
// (attn_decode_ring_kernel): the other two units hold only the kernels they held before.
//
// The cache has C = slots positions per (batch entry, kv head) and position j lives in slot j mod C.  `total` tokens were counted before
// the call (p.kv_len, or the int64 at p.kv_len_dev): clamped below at 0, NOT above -- it grows for as long as the generation runs -- and
// 64-bit throughout.  With k_new / v_new the call appends, n = total + 1; without, n = total.  The query sits at n - 1 and sees positions
// lo = max(0, n - W) .. n - 1: v = n - lo <= W of them (W = window, 1 <= W <= C).
//
// The block works on the RELATIVE index r = j - lo in 0 .. v - 1 exactly as the linear kernel works on positions 0 .. n - 1 of a cache of
// W positions: split s owns r in [s * chunk, (s + 1) * chunk), first = 0, live = ceil(v / chunk), the same lanes, tiles and merge order,
// and the geometry is attn_decode_geom(.., W) -- a function of the shapes alone, so one captured launch serves every total.  Only a cache
// address differs: slot = slot0 + r, minus C once if it reaches C (r < W <= C: once is enough), with slot0 = lo mod C ONE wave-uniform
// 64-bit modulo per block; no division per position.  The mask's columns are indexed by r (the order of the mask transformers builds for
// a sliding layer: its kv_offset is lo).  So a call gives, bit for bit, what the kernel without a window gives on a linear copy
// [B, Hkv, W, D] that holds positions lo .. n - 1 in slots 0 .. v - 1.
//
// r >= v is never loaded, neither by the tile walk nor by the prefetch of the next tile, and so is no slot that holds no visible position.
//
// Append.  The row goes to slot (n - 1) mod C, stored by the lane group that owns r = v - 1, as the linear kernel stores position kv_len.
// C >= W makes that race-free: the slot held position n - 1 - C < lo, which no block of this launch reads.  (The entry refuses C < W.)
//
// The fields of AttnDecodeParams as the ring reads them: kv_len / kv_len_dev the total, max_len the slots C, window W (always >= 1),
// chunk / splits / partials for max_len = W.  No field is added: the struct is part of the other kernels' argument layout.
#include "attn_decode_kernel.hpp"

namespace qllm {

int launch_attn_decode_ring(const AttnDecodeParams &p, int head_dim, int act_bf16, hipStream_t stream) {
  return launch_attn_decode_variant<false, true>(p, head_dim, act_bf16, stream);
}

}  // namespace qllm
