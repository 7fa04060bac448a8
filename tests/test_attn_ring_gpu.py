"""-m gpu: ops.attn_decode_ring (qllm_attn_decode_ring, csrc/attn_decode_ring.hip) on the device, and q_layers/fused_attention.py on tiny
Mistral and Qwen2 models whose sliding layers are ring layers (modeling/ring_cache.py; tests/attn_ring_cases.py).

1. A ring call is, bit for bit, ops.attn_decode without a window on the linearised copy [B, Hkv, W, D] of the visible positions: W = 3
   tiles + 5 (several splits, a ragged last one), C = W and W + 37, totals around the fill, the first wraps, the split edges, a tile across
   the seam and 2^40 + 7; host and device total, with and without the append, no mask, bool and additive masks indexed by the relative
   position; NaN in every slot that holds no visible position; the append's one slot; the workspace's counter page.
2. Without the linear kernel: the same cases per element within attn_decode_cases.bound of the float64 oracle over the visible
   positions, and exact selection of one key with a better match in every hidden slot the ring still holds.
3. ONE captured launch (the appending call with the total on the device, then add_(1)) replayed from total 0 to 2 W + 3.
4. Refusals before any device work.
5. The modules: a ring cache against a plain StaticCache, both fused -- the ring op at every decode step, the bound against the float64
   model, the plain cache's bits.  6. The fallbacks: the kill switch, prompts and chunks."""
import pytest
import torch

import attn_decode_cases as AD
import attn_ring_cases as R
import attn_sliding_cases as S
import decode_loop_cases as D

from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope
from qllm_amd.modeling.ring_cache import RingSlidingWindowLayer, ring_static_cache

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def tag(dtype):
    return str(dtype)[6:]


def bits(t):
    return t.contiguous().view(torch.int16)


def dev_int(n):
    return torch.tensor(n, dtype=torch.int64, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV)


def counters_are_zero():
    return int(ops.workspace(torch.device(DEV), 0)[:16384].count_nonzero()) == 0


CONFIGS = [(hq, hk, d, dtype) for hq, hk in R.GROUPS for d in R.DIMS for dtype in R.DTYPES]
CONFIG_IDS = [f"{hq}x{hk}-{d}-{tag(dtype)}" for hq, hk, d, dtype in CONFIGS]
configs = pytest.mark.parametrize("hq,hk,d,dtype", CONFIGS, ids=CONFIG_IDS)
slots_of = pytest.mark.parametrize("extra", [0, R.EXTRA_SLOTS], ids=["C=W", "C=W+37"])
batches = pytest.mark.parametrize("b", R.BATCHES, ids=["B1", "B3"])


# ---- 1. and 2. the direct calls ----------------------------------------------------------------------------------------------------------------------
@slots_of
@batches
@configs
def test_a_ring_call_is_the_linear_call_on_the_visible_positions(hq, hk, d, dtype, b, extra):
    w, geo = R.geometry(b, hq, hk, d)
    slots, scaling = w + extra, d ** -0.5
    assert geo["splits"] >= 2 and w % geo["tile"] == 5
    q, rows_k, rows_v = R.stream(b, hq, hk, d, w, dtype, 7 * hq + d + b)
    qd = q.to(DEV)
    worst = 0.0
    for total in R.totals(w, geo["chunk"], geo["tile"]):
        for append in (False, True):
            n, lo, v = R.view(total, append, w)
            cached = v - append
            k_ring, v_ring = R.ring_of(rows_k, lo, cached, slots), R.ring_of(rows_v, lo, cached, slots)          # NaN wherever no visible position lives
            k_lin, v_lin = R.linear_of(rows_k, cached, w).to(DEV), R.linear_of(rows_v, cached, w).to(DEV)
            k_new, v_new = (rows_k[:, :, v - 1:v].to(DEV), rows_v[:, :, v - 1:v].to(DEV)) if append else (None, None)
            for kind in (None, "bool", "additive"):
                mask, vis = R.mask_of(kind, b, w, v, dtype)
                md = dev(mask)
                want = ops.attn_decode(qd, k_lin.clone(), v_lin.clone(), cached, k_new, v_new, mask=md, scaling=scaling).cpu()      # the bits that define the call
                if v:
                    bias = None if kind != "additive" else mask[:, 0, 0]
                    ref = AD.oracle(q[:, :, 0], rows_k, rows_v, v, scaling, visible=vis, bias=bias)
                    e32, _ = AD.fp32_error(q[:, :, 0], rows_k, rows_v, v, scaling, ref, mask=None if kind is None else mask[:, 0, 0])
                    tol = AD.bound(ref, e32, dtype)
                for where in ("host", "device"):
                    kd, vd = k_ring.to(DEV), v_ring.to(DEV)
                    got = ops.attn_decode_ring(qd, kd, vd, total if where == "host" else dev_int(total), w, k_new, v_new, mask=md, scaling=scaling).cpu()
                    case = (total, append, kind, where)
                    assert counters_are_zero(), case
                    assert bool(torch.isfinite(got.float()).all()), case
                    assert torch.equal(bits(got), bits(want)), case
                    changed = ((bits(kd.cpu()) != bits(k_ring)) | (bits(vd.cpu()) != bits(v_ring))).any(dim=-1).any(dim=0).any(dim=0).nonzero().flatten().tolist()
                    if append:                                                                       # exactly the new token's slot, and it holds the new rows
                        slot = (n - 1) % slots
                        assert changed == [slot], (case, changed)
                        assert torch.equal(bits(kd[:, :, slot].cpu()), bits(rows_k[:, :, v - 1])) and torch.equal(bits(vd[:, :, slot].cpu()), bits(rows_v[:, :, v - 1])), case
                    else:
                        assert changed == [], (case, changed)
                    if v:
                        err = (got.double() - ref).abs()
                        worst = max(worst, (err / tol).max().item())
                        assert bool((err <= tol).all()), (case, (err / tol).max().item())
                    else:
                        assert not bool(got.any()), case                                              # no visible key: zeros
    print(f"ring decode {hq}x{hk} D{d} {tag(dtype)} B{b} C=W+{extra}: W {w} chunk {geo['chunk']} splits {geo['splits']} worst error / bound {worst:.3f}")


@slots_of
@batches
@configs
def test_a_ring_call_selects_one_key_bit_for_bit(hq, hk, d, dtype, b, extra):
    """attn_ring_cases.selection: the answer is V[target]; every hidden slot the ring still holds would win outright."""
    w, geo = R.geometry(b, hq, hk, d)
    slots = w + extra
    for total in (w - 1, 2 * w + geo["tile"] // 2 + 3, (1 << 40) + 7):
        n, lo, v = R.view(total, True, w)
        targets = R.selection_targets(w, slots, total, geo["chunk"])
        assert {0, v - 1} | set(range(0, v, geo["chunk"])) <= set(targets)
        for target in targets:
            q, k_ring, v_ring, k_new, v_new, want = R.selection(b, hq, hk, d, w, slots, total, target, dtype)
            got = ops.attn_decode_ring(q.to(DEV), k_ring.to(DEV), v_ring.to(DEV), dev_int(total), w, k_new.to(DEV), v_new.to(DEV), scaling=R.SEL_SCALING).cpu()
            wrong = (bits(got) != bits(want)).any(dim=-1)
            assert not bool(wrong.any()), (total, target, "slot", (lo + target) % slots, "first wrong (b, h)", wrong.nonzero()[:4].tolist())


# ---- 3. one captured launch ----------------------------------------------------------------------------------------------------------------------------
@slots_of
@pytest.mark.parametrize("hq,hk,d,dtype,b", [c + (b,) for c, b in zip(CONFIGS[:2] + CONFIGS[-2:], (1, 3, 3, 1))],
                         ids=[f"{i}-B{b}" for i, b in zip(CONFIG_IDS[:2] + CONFIG_IDS[-2:], (1, 3, 3, 1))])
def test_one_captured_step_serves_every_length(hq, hk, d, dtype, b, extra):
    """The appending call with the total on the device and the add_(1) behind it, captured ONCE at total 0 and replayed with a new q, k and
    v up to total 2 W + 3: through the fill, the first wrap and the second.  Against the linearised call at every seventh step and at
    every step around W and 2 W."""
    w, geo = R.geometry(b, hq, hk, d)
    slots, steps, scaling = w + extra, 2 * w + 4, d ** -0.5
    gen = torch.Generator().manual_seed(3 * hq + d)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype).to(DEV)
    q_all, k_all, v_all = r(steps, b, hq, 1, d), r(b, hk, steps, d), r(b, hk, steps, d)
    kc, vc = torch.full((b, hk, slots, d), R.NAN, dtype=dtype, device=DEV), torch.full((b, hk, slots, d), R.NAN, dtype=dtype, device=DEV)
    qs, ks, vs, out = q_all[0].clone(), k_all[:, :, :1].clone(), v_all[:, :, :1].clone(), torch.empty(b, hq, d, dtype=dtype, device=DEV)
    total = dev_int(0)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_decode_ring(qs, kc.clone(), vc.clone(), total, w, ks, vs, scaling=scaling, out=out)      # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.attn_decode_ring(qs, kc, vc, total, w, ks, vs, scaling=scaling, out=out)
            total.add_(1)
    torch.cuda.current_stream().wait_stream(side)
    checked = 0
    for t in range(steps):
        qs.copy_(q_all[t]), ks.copy_(k_all[:, :, t:t + 1]), vs.copy_(v_all[:, :, t:t + 1])
        graph.replay()
        if t % 7 == 0 or abs(t - w) <= 2 or abs(t - 2 * w) <= 2 or t == steps - 1:
            n, lo, v = R.view(t, True, w)
            k_lin, v_lin = torch.zeros(b, hk, w, d, dtype=dtype, device=DEV), torch.zeros(b, hk, w, d, dtype=dtype, device=DEV)
            k_lin[:, :, :v - 1], v_lin[:, :, :v - 1] = k_all[:, :, lo:n - 1], v_all[:, :, lo:n - 1]
            want = ops.attn_decode(q_all[t], k_lin, v_lin, v - 1, k_all[:, :, t:t + 1], v_all[:, :, t:t + 1], scaling=scaling)
            assert torch.equal(bits(out), bits(want)), t
            checked += 1
    torch.cuda.synchronize()
    assert int(total) == steps and counters_are_zero() and checked >= steps // 7 + 10
    last = torch.arange(steps - min(slots, steps), steps, device=DEV)                                   # the ring holds the last C positions in their slots
    assert torch.equal(bits(kc[:, :, last % slots]), bits(k_all[:, :, last])) and torch.equal(bits(vc[:, :, last % slots]), bits(v_all[:, :, last]))
    assert bool(torch.isfinite(out.float()).all())


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_come_before_any_device_work():
    b, hq, hk, d, slots = 2, 8, 2, 64, 40
    g = torch.Generator().manual_seed(1)
    r = lambda *shape: torch.randn(shape, generator=g).to(torch.float16).to(DEV)
    q, k, v, kn, vn = r(b, hq, 1, d), r(b, hk, slots, d), r(b, hk, slots, d), r(b, hk, 1, d), r(b, hk, 1, d)
    poison = torch.full((b, hq, d), 1234.0, dtype=torch.float16, device=DEV)
    out, k0, v0 = poison.clone(), k.clone(), v.clone()
    short = torch.ones(b, 1, 1, 29, dtype=torch.bool, device=DEV)
    for call, text in ((lambda: ops.attn_decode_ring(q, k, v, 7, slots + 1, kn, vn, out=out), "window"),              # slots < window
                       (lambda: ops.attn_decode_ring(q, k, v, 7, 0, kn, vn, out=out), "window"),
                       (lambda: ops.attn_decode_ring(q, k, v, 100, 30, kn, vn, mask=short, out=out), "cover 30"),
                       (lambda: ops.attn_decode_ring(q, k, v, dev_int(3), 30, kn, vn, mask=short, out=out), "cover 30")):
        with pytest.raises(ops.QllmUnsupported, match=text):
            call()
    # the entry itself, with real pointers and a real workspace: the op's plan never lets these through
    lib = _lib.load()
    ws = ops.workspace(torch.device(DEV), lib.qllm_attn_decode_workspace_bytes(b, hq, hk, d, 30))

    def entry(window, slots_arg, mask=None, mask_len=0):
        return lib.qllm_attn_decode_ring(q.data_ptr(), kn.data_ptr(), vn.data_ptr(), k.data_ptr(), v.data_ptr(), None if mask is None else mask.data_ptr(), out.data_ptr(),
                                         b, hq, hk, d, 100, None, slots_arg, window, hq * d, d, hk * d, d, hk * d, d, hk * slots * d, slots * d, d,
                                         _lib.ATTN_MASK_NONE if mask is None else _lib.ATTN_MASK_BOOL, mask_len, mask_len, 0.125, _lib.DT_F16, ws.data_ptr(), ws.numel(), None)

    for args, text in (((slots + 1, slots), "1 <= window <= slots"), ((0, slots), "1 <= window <= slots"), ((30, slots, short, 29), "cover 30")):
        rc = entry(*args)
        assert rc == _lib.QLLM_ERR_INVALID and text in _lib.last_error(), (rc, _lib.last_error())
    torch.cuda.synchronize()
    assert torch.equal(out, poison) and torch.equal(k, k0) and torch.equal(v, v0) and counters_are_zero()
    assert entry(30, slots) == _lib.QLLM_OK                                                        # and the valid call runs
    torch.cuda.synchronize()
    assert not torch.equal(out, poison) and bool(torch.isfinite(out.float()).all())


# ---- 5. and 6. the modules ---------------------------------------------------------------------------------------------------------------------------------
_models = {}


def tier_a(name):
    if name not in _models:
        model, slides, window = S.sliding_model(name, device=DEV)
        _models[name] = (model, D.float64_copy(model), slides, window)
    return _models[name]


def recorded(monkeypatch):
    """-> (S.record's list for ops.attn_decode / ops.attn_prefill, the ring calls: total, on the device, window, slots, appending)."""
    calls, ring, real = S.record(monkeypatch, ops.attn_decode, ops.attn_prefill), [], ops.attn_decode_ring

    def op(q, k_cache, v_cache, total, window, *a, **kw):
        ring.append((int(total), isinstance(total, torch.Tensor), window, k_cache.shape[2], kw.get("k_new") is not None and kw.get("v_new") is not None))
        return real(q, k_cache, v_cache, total, window, *a, **kw)

    monkeypatch.setattr(ops, "attn_decode_ring", op)
    return calls, ring


def sizes(name, window):
    """(max_cache_len, decode steps): at least 3 W tokens behind the 5-token prompt; the full layer of qwen2-4 holds them all."""
    return 32, max(3 * window, 12)


# E(fused) <= M_DEVICE x E(unfused), both against the float64 model: the bound of test_attn_sliding_gpu's tier A (decode_loop_cases.assert_case
# with decode_loop_cases.M_DEVICE = 2.5), restated
M_DEVICE = 2.5
assert M_DEVICE == D.M_DEVICE


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_a_ring_cache_decodes_through_the_ring_kernel_with_the_static_caches_bits(name, batch, monkeypatch):
    from transformers import StaticCache
    model, ref, slides, window = tier_a(name)
    size, steps = sizes(name, window)
    inp = D.batch_inputs(batch, steps=steps)
    assert inp.prompt + steps >= 3 * window and inp.prompt + steps <= size
    reference, unfused = D.run(ref, inp), D.run(model, inp, StaticCache(config=model.config, max_cache_len=size), DEV)
    calls, ring = recorded(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS
    try:
        static = D.run(model, inp, StaticCache(config=model.config, max_cache_len=size), DEV)
        static_calls = len(calls)
        del calls[:]
        fused = D.run(model, inp, ring_static_cache(model.config, size), DEV)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    n_slide = sum(slides)
    assert static_calls == D.LAYERS * steps and [type(layer) is RingSlidingWindowLayer for layer in fused.cache.layers] == slides
    # every decode step of a sliding layer -- before, at and well past the window -- is the ring kernel's, never ops.attn_decode's
    assert ring == [(inp.prompt + t, True, window, window, True) for t in range(steps) for _ in range(n_slide)]
    assert [c.op for c in calls] == ["decode"] * ((D.LAYERS - n_slide) * steps) and not any(c.has_window for c in calls)
    assert [int(layer.cumulative_length) for layer in fused.cache.layers] == [inp.prompt + steps] * D.LAYERS
    assert D.same_bits(fused.prefill, static.prefill), "the prefill logits differ from the plain cache's"
    D.assert_same_logits(fused.steps, static.steps, f"ring {name} {batch} against the plain StaticCache, both fused")
    D.assert_case(fused, unfused, reference, M_DEVICE, label=f"ring {name} {batch}")


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
def test_the_kill_switch_leaves_a_ring_cache_to_update(batch, monkeypatch):
    from transformers import StaticCache
    model, ref, slides, window = tier_a("mistral-4")
    size, steps = sizes("mistral-4", window)
    inp = D.batch_inputs(batch, steps=steps)
    plain = D.run(model, inp, StaticCache(config=model.config, max_cache_len=size), DEV)                 # the fusion not installed
    calls, ring = recorded(monkeypatch)
    monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "0")
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        got = D.run(model, inp, ring_static_cache(model.config, size), DEV)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert calls == [] and ring == []
    assert D.same_bits(got.prefill, plain.prefill)
    D.assert_same_logits(got.steps, plain.steps, f"ring mistral-4 {batch} under QLLM_FUSE_ATTENTION_SLIDING=0")


PIECES = ((0, 5), (5, 8), (8, 9), (9, 10))               # a prompt, a chunk of three behind it, two decode steps
LONG = ((0, 11), (11, 12))                               # a prompt longer than either window, one decode step


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("pieces", [PIECES, LONG], ids=["chunks", "long prompt"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_prompts_and_chunks_on_a_ring_cache_give_what_the_static_cache_gives(name, pieces, batch, monkeypatch):
    model, ref, slides, window = tier_a(name)
    inp = D.batch_inputs(batch)
    calls, ring = recorded(monkeypatch)
    S.open_routes(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        static, _ = S.forwards(model, inp, "static", DEV, pieces)
        want_calls = [vars(c) for c in calls if c.op == "prefill"]
        del calls[:]
        monkeypatch.setattr(D, "make_cache", lambda m, kind: ring_static_cache(m.config, D.MAX_CACHE_LEN))
        fused, cache = S.forwards(model, inp, "static", DEV, pieces)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    assert [type(layer) is RingSlidingWindowLayer for layer in cache.layers] == slides
    assert [vars(c) for c in calls if c.op == "prefill"] == want_calls and len(want_calls) == D.LAYERS * sum(e - a > 1 for a, e in pieces)
    assert len(ring) == sum(slides) * sum(e - a == 1 for a, e in pieces)
    assert bool(torch.isfinite(fused.float()).all()) and D.same_bits(fused, static)
