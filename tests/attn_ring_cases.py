"""What tests/test_attn_ring_cpu.py and tests/test_attn_ring_gpu.py share: the ring-buffer form of the decode attention call
(qllm_attn_decode_ring / ops.attn_decode_ring: position j lives in slot j mod C) -- the shapes, the totals, rings built directly from a
synthetic stream (nobody steps through 2^40 tokens), the linearised copy that defines the call's bits, the masks indexed by the relative
position, the exact selection inputs, a torch restatement of the op for the CPU module tests, and fake argument sets for the C entry.

Semantics: `total` tokens were counted before the call; with an append n = total + 1, else n = total; the query at n - 1 sees positions
lo = max(0, n - W) .. n - 1, v = n - lo of them; r = j - lo is the relative index the splits and the mask's columns are counted in."""
import torch

import attn_decode_cases as AD
import attn_prefill_cases as AP

from qllm_amd import _lib

GROUPS = ((8, 2), (7, 1))
DIMS = (64, 128)
BATCHES = (1, 3)
DTYPES = (torch.float16, torch.bfloat16)
EXTRA_SLOTS = 37
NAN = float("nan")


def tile_of(d):
    return 64 if d == 128 else 128


def window_of(d):
    """3 tiles + 5: several splits and a ragged last one."""
    return 3 * tile_of(d) + 5


def geometry(b, hq, hk, d):
    """(W, {tile, splits, chunk, group}) of a ring call: the launch of a linear call whose max_len is the window."""
    from qllm_amd import ops
    w = window_of(d)
    g = AD.parse_describe(ops.attn_decode_describe(b, hq, hk, d, w))
    assert g["tile"] == tile_of(d) and g["chunk"] % g["tile"] == 0 and (g["splits"] - 1) * g["chunk"] < w <= g["splits"] * g["chunk"], g
    return w, g


def totals(w, chunk, tile):
    """The totals of the issue: around the fill, the first wraps, split edges, a tile across the seam, and past 2^40."""
    return sorted({0, 1, w - 1, w, w + 1, w + chunk - 1, w + chunk, 2 * w - 1, 2 * w, 2 * w + tile // 2 + 3, (1 << 40) + 7})


def view(total, append, w):
    """(n, lo, v) of a call."""
    n = total + (1 if append else 0)
    lo = max(0, n - w)
    return n, lo, n - lo


def stream(b, hq, hk, d, w, dtype, seed):
    """q [B, Hq, 1, D] and W rows of K and V [B, Hkv, W, D]: row r is what the stream holds at position lo + r, whatever lo is."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    return r(b, hq, 1, d), r(b, hk, w, d), r(b, hk, w, d)


def ring_of(rows, lo, count, slots, fill=NAN):
    """[B, Hkv, slots, D]: rows[:, :, r] in slot (lo + r) mod slots for r < count, `fill` in every other slot."""
    b, hk, _, d = rows.shape
    ring = torch.full((b, hk, slots, d), fill, dtype=rows.dtype)
    if count:
        ring[:, :, (lo + torch.arange(count)) % slots] = rows[:, :, :count]
    return ring


def linear_of(rows, count, w, fill=NAN):
    """[B, Hkv, W, D]: the linearised copy, rows[:, :, r] in slot r for r < count, `fill` behind."""
    lin = torch.full(rows.shape[:2] + (w, rows.shape[3]), fill, dtype=rows.dtype)
    lin[:, :, :count] = rows[:, :, :count]
    return lin


def mask_of(kind, b, w, v, dtype, seed=5):
    """None, or [B, 1, 1, W] indexed by r: left padding (row i hides r < 3 i, never the newest) plus scattered holes (r % 11 == 5); bool, or
    additive in `dtype` with finite biases on the visible keys.  -> the mask and the [B, W] bool of what it shows."""
    if kind is None:
        return None, torch.ones(b, w, dtype=torch.bool)
    r = torch.arange(w)[None, :]
    vis = (r >= 3 * torch.arange(b)[:, None]) & (r % 11 != 5) | (r == v - 1)
    if kind == "bool":
        return vis[:, None, None, :].clone(), vis
    bias = (torch.randn(b, w, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.5).to(dtype)
    return torch.where(vis, bias, torch.full((), torch.finfo(dtype).min, dtype=dtype))[:, None, None, :], vis


# ---- exact selection ---------------------------------------------------------------------------------------------------------------------------
SEL_Q, SEL_DECOY, SEL_SCALING = 64.0, 128.0, 0.125


def selection(b, hq, hk, d, w, slots, total, target_r, dtype):
    """An appending call whose answer is V[target] bit for bit.  q = 64 e_0 (scaling 0.125); the key at r = target_r is 64 e_0 (score
    512), every other visible key zero (score 0: 512 below, weight exactly 0 in fp32 and below 1e-220 in float64); V rows encode r
    (attn_prefill_cases.value_rows).  Every hidden slot that physically holds a position (n - C .. lo - 1, the slots a ring of C > W
    keeps behind the window) carries the decoy key 128 e_0 (score 1024) and V = NaN; a slot that holds nothing is NaN in both.
    -> q, k_ring, v_ring, k_new, v_new [B, Hkv, 1, D], expected [B, Hq, D]."""
    n, lo, v = view(total, True, w)
    assert 0 <= target_r < v
    k = torch.zeros(b, hk, v, d, dtype=dtype)
    k[:, :, target_r, 0] = SEL_Q
    vals = AP.value_rows(b, hk, v, d, dtype)
    k_ring, v_ring = ring_of(k, lo, v - 1, slots), ring_of(vals, lo, v - 1, slots)
    hidden = torch.arange(max(0, n - slots), lo)
    if len(hidden):
        k_ring[:, :, hidden % slots] = 0
        k_ring[:, :, hidden % slots, 0] = SEL_DECOY
    q = torch.zeros(b, hq, 1, d, dtype=dtype)
    q[..., 0] = SEL_Q
    want = vals[:, :, target_r].repeat_interleave(hq // hk, dim=1)
    return q, k_ring, v_ring, k[:, :, v - 1:v].contiguous(), vals[:, :, v - 1:v].contiguous(), want


def selection_targets(w, slots, total, chunk):
    """r of: lo, n - 1 (the appended row), the first position of each split, the positions in slot C - 1 and in slot 0."""
    n, lo, v = view(total, True, w)
    rs = {0, v - 1} | set(range(0, v, chunk))
    rs |= {r for r in (((slots - 1 - lo) % slots), ((0 - lo) % slots)) if r < v}
    return sorted(rs)


# ---- the op restated in torch ------------------------------------------------------------------------------------------------------------------
def ring_restated(q, k_cache, v_cache, total, window, k_new=None, v_new=None, mask=None, scaling=None, *, out=None, plan=None):
    """ops.attn_decode_ring restated (any device): the append into slot (n - 1) mod C, then attn_decode_cases.restated over the linearised
    visible positions with the mask's first v columns.  Same signature."""
    slots = k_cache.shape[2]
    n, lo, v = view(int(total), k_new is not None, window)
    if k_new is not None:
        k_cache[:, :, (n - 1) % slots] = k_new.squeeze(2 if k_new.shape[2] == 1 else 1)
        v_cache[:, :, (n - 1) % slots] = v_new.squeeze(2 if v_new.shape[2] == 1 else 1)
    idx = torch.arange(lo, n, device=k_cache.device) % slots
    m = None if mask is None else mask.reshape(mask.shape[0], -1)[:, :v]
    return AD.restated(q, k_cache.index_select(2, idx), v_cache.index_select(2, idx), v, mask=m, scaling=scaling)


# ---- the C entry with fake pointers ----------------------------------------------------------------------------------------------------------------
RING_PTRS = {n: 4096 * (i + 1) for i, n in enumerate(("q", "k_new", "v_new", "k_cache", "v_cache", "mask", "out", "total_dev", "ws"))}
RING_STRIDE_NAMES = ("q_row", "q_head", "kn_row", "kn_head", "vn_row", "vn_head", "c_batch", "c_head", "c_pos")
RING_STRIDES = (256, 64, 128, 64, 128, 64, 12800, 6400, 64)        # 4 query heads, 2 kv heads of 64, 100 slots


def ring_call(lib, b=2, hq=4, hk=2, d=64, total=10, slots=100, window=60, strides=RING_STRIDES, mask_kind=_lib.ATTN_MASK_BOOL, mask_len=60, mask_batch=60,
              dt=_lib.DT_F16, ws_bytes=1 << 30, **kw):
    """qllm_attn_decode_ring with an append and a bool mask; `kw`: pointers by name (None: NULL; `total_dev` and `ws` are NULL unless given)
    and single strides by name.  Never dereferenced: a call made with these must be refused before any device work -- the base set ends
    at the workspace rule."""
    strides = [kw.pop(n, s) for n, s in zip(RING_STRIDE_NAMES, strides)]
    p = dict(dict(RING_PTRS, total_dev=None, ws=None), **kw)
    assert set(p) == set(RING_PTRS), sorted(kw)
    return lib.qllm_attn_decode_ring(p["q"], p["k_new"], p["v_new"], p["k_cache"], p["v_cache"], p["mask"], p["out"], b, hq, hk, d, total, p["total_dev"], slots,
                                     window, *strides, mask_kind, mask_len, mask_batch, 0.125, dt, p["ws"], ws_bytes, None)
