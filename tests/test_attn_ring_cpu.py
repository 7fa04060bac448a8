"""No GPU: the ring-buffer sliding-window cache as far as a host reaches -- modeling/ring_cache.py against transformers'
StaticSlidingWindowLayer update for update, the helpers that build ring caches, a tiny fp32 Mistral through the fill and far past it, the
host rules of qllm_attn_decode_ring through the C ABI with fake pointers, ops.attn_decode_ring_plan, the routing of
q_layers/fused_attention.py (kind "ring_sliding") with the op restated in torch in the kernel's place, and the resources of the three
decode attention units (tests/attn_ring_cases.py)."""
import ctypes as C
import os
import re

import pytest
import torch

import attn_ring_cases as R
import attn_sliding_cases as S
import decode_loop_cases as D
from test_rope_cpu import fake_op as fake_rope

import qllm_amd
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope
from qllm_amd.modeling.ring_cache import RingSlidingWindowLayer, ring_static_cache, to_ring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS, WS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_WORKSPACE


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- 7. the layer against its parent -------------------------------------------------------------------------------------------------------------
SCRIPTS = {
    "tokens through the fill": lambda w: [1] * (3 * w + 2),
    "a prompt that fills exactly": lambda w: [w, 1, 1, 2, 1],
    "a prompt one short, then the fill": lambda w: [w - 1, 1, 1, 1],
    "a prompt that overshoots": lambda w: [w + 1, 1, 3, 1],
    "a chunk across the fill": lambda w: [2, w, 1, 1],
    "chunks once full": lambda w: [1] * w + [3, 1, w, 1, w + 2, 1],
    "a prompt of three windows": lambda w: [3 * w + 1, 1, 2, 1],
    "two tokens at a time": lambda w: [2] * (w + 1) + [1],
}


def random_script(w, seed):
    g = torch.Generator().manual_seed(seed)
    return [int(torch.randint(1, 4, (1,), generator=g)) if torch.rand(1, generator=g) < 0.3 else 1 for _ in range(4 * w)]


def side_by_side(w, sizes, max_cache_len=32, b=2, h=2, d=8, seed=0):
    """Feed the same rows to a ring layer and to transformers' layer; after every update the returned states, the mask sizes and the
    length are equal, the ring's device counter is the total and its storage holds position j in slot j mod C."""
    from transformers.cache_utils import StaticSlidingWindowLayer
    ring, ref = RingSlidingWindowLayer(max_cache_len=max_cache_len, sliding_window=w), StaticSlidingWindowLayer(max_cache_len=max_cache_len, sliding_window=w)
    size = min(w, max_cache_len)
    g = torch.Generator().manual_seed(seed)
    history_k, history_v = torch.empty(b, h, 0, d), torch.empty(b, h, 0, d)
    for step, q in enumerate(sizes):
        k, v = torch.randn(b, h, q, d, generator=g), torch.randn(b, h, q, d, generator=g)
        for query in (1, q, 3):
            assert ring.get_mask_sizes(query) == ref.get_mask_sizes(query), (step, query)
        got, want = ring.update(k.clone(), v.clone()), ref.update(k.clone(), v.clone())
        history_k, history_v = torch.cat((history_k, k), 2), torch.cat((history_v, v), 2)
        total = history_k.shape[2]
        for a, e in zip(got, want):
            assert a.shape == e.shape and torch.equal(a, e), (step, q, a.shape, e.shape)
        assert ring.get_seq_length() == ref.get_seq_length() == total and ring.cumulative_length_int == ref.cumulative_length_int
        assert ring.get_mask_sizes(1) == ref.get_mask_sizes(1)
        assert ring.cumulative_length.dtype == torch.int64 and int(ring.cumulative_length) == total, (step, int(ring.cumulative_length), total)
        assert ring.keys.shape == ref.keys.shape == (b, h, size, d)
        for j in range(max(0, total - size), total):
            assert torch.equal(ring.keys[:, :, j % size], history_k[:, :, j]) and torch.equal(ring.values[:, :, j % size], history_v[:, :, j]), (step, j)
    return ring, ref


@pytest.mark.parametrize("w", [4, 8, 13])
@pytest.mark.parametrize("script", list(SCRIPTS))
def test_a_ring_layer_returns_what_the_static_sliding_layer_returns(script, w):
    side_by_side(w, SCRIPTS[script](w))


@pytest.mark.parametrize("w", [4, 8, 13])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_update_sequences_agree_too(seed, w):
    side_by_side(w, random_script(w, seed), seed=seed)


def test_a_layer_bounded_by_max_cache_len_and_a_counter_kept_past_the_overflow():
    ring, ref = side_by_side(13, [5, 1, 1, 1, 4, 1], max_cache_len=6)
    assert ring.max_cache_len == 6 and int(ring.cumulative_length) == 13
    assert int(ref.cumulative_length) < 13                          # the parent's stops at the overflow: the tensor the ring kernel could not use


def test_advance_reset_and_reorder():
    ring, ref = side_by_side(4, [3, 1, 1, 1])
    keys = ring.keys.clone()
    ring.advance(2)
    assert int(ring.cumulative_length) == 8 and ring.cumulative_length_int == 8 and torch.equal(ring.keys, keys)     # counts, copies nothing
    assert ring.get_mask_sizes(1) == (4, 5)
    order = torch.tensor([1, 0])
    want_k, want_v = ring.keys[order].clone(), ring.values[order].clone()
    ring.reorder_cache(order)
    ref.reorder_cache(order)
    assert torch.equal(ring.keys, want_k) and torch.equal(ring.values, want_v)
    addr = ring.keys.data_ptr()                                                                                      # (a reorder makes new tensors, as the parent's)
    ring.reset()
    ref.reset()
    assert int(ring.cumulative_length) == 0 == ring.cumulative_length_int and ring.get_seq_length() == ref.get_seq_length() == 0
    assert not ring.keys.any() and not ring.values.any() and ring.keys.data_ptr() == addr                            # static addresses
    assert ring.get_mask_sizes(1) == ref.get_mask_sizes(1)
    k = torch.randn(2, 2, 1, 8)
    assert all(torch.equal(a, e) for a, e in zip(ring.update(k, k), ref.update(k, k)))


def configs():
    import transformers
    kw = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=4, num_attention_heads=4, num_key_value_heads=2, vocab_size=64)
    mistral = transformers.MistralConfig(sliding_window=8, **kw)
    qwen = transformers.Qwen2Config(use_sliding_window=True, sliding_window=8, max_window_layers=2, **kw)
    assert qwen.layer_types == ["full_attention"] * 2 + ["sliding_attention"] * 2
    return mistral, qwen


def test_the_helpers_replace_exactly_the_sliding_layers():
    from transformers import DynamicCache, StaticCache
    from transformers.cache_utils import StaticLayer, StaticSlidingWindowLayer
    assert qllm_amd.RingSlidingWindowLayer is RingSlidingWindowLayer and qllm_amd.ring_static_cache is ring_static_cache and qllm_amd.to_ring is to_ring
    mistral, qwen = configs()
    for cfg, slides in ((mistral, [True] * 4), (qwen, [False, False, True, True])):
        for max_cache_len, size in ((32, 8), (5, 5)):
            plain = StaticCache(config=cfg, max_cache_len=max_cache_len)
            for cache in (ring_static_cache(cfg, max_cache_len), to_ring(StaticCache(config=cfg, max_cache_len=max_cache_len))):
                assert type(cache) is StaticCache and len(cache.layers) == 4
                for layer, was, s in zip(cache.layers, plain.layers, slides):
                    assert type(layer) is (RingSlidingWindowLayer if s else StaticLayer) and type(was) is (StaticSlidingWindowLayer if s else StaticLayer)
                    assert layer.max_cache_len == was.max_cache_len == (size if s else max_cache_len) and not layer.is_initialized
                    assert layer.is_sliding == was.is_sliding
    cache = to_ring(StaticCache(config=mistral, max_cache_len=32))
    assert to_ring(cache) is cache and all(type(layer) is RingSlidingWindowLayer for layer in cache.layers)          # nothing left to replace
    used = StaticCache(config=mistral, max_cache_len=32)
    used.update(torch.zeros(1, 2, 3, 16), torch.zeros(1, 2, 3, 16), 0)
    with pytest.raises(ValueError, match="initialised"):
        to_ring(used)
    offloading = StaticCache(config=mistral, max_cache_len=32)
    offloading.offloading = True                                   # (the constructor's flag opens a device stream: not on a host without one)
    with pytest.raises(ValueError, match="offload"):
        to_ring(offloading)
    assert all(type(layer) is StaticSlidingWindowLayer for layer in offloading.layers)
    dynamic = DynamicCache(config=mistral)
    before = list(dynamic.layers)
    assert to_ring(dynamic) is dynamic and dynamic.layers == before                                                     # no static sliding layer: untouched


# ---- 8. a tiny CPU Mistral -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["mistral-4", "mistral-8", "qwen2-4"])
def test_a_cpu_model_on_a_ring_cache_is_the_model_on_a_static_cache(name):
    """fp32 on the CPU: the kernel is never eligible, with or without the fusion installed; only `update` runs."""
    from transformers import StaticCache
    model, slides, window = S.sliding_model(name, dtype=torch.float32)
    steps = 2 * window + 4 if name != "qwen2-4" else 11                                # (the full layer of qwen2-4 holds 16 positions)
    inp = D.batch_inputs("padded", steps=steps)
    want = D.run(model, inp, StaticCache(config=model.config, max_cache_len=32 if name != "qwen2-4" else 16))
    got = D.run(model, inp, ring_static_cache(model.config, 32 if name != "qwen2-4" else 16))
    assert [type(layer) is RingSlidingWindowLayer for layer in got.cache.layers] == slides
    assert torch.equal(got.prefill, want.prefill) and torch.equal(got.steps, want.steps)
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused = D.run(model, inp, ring_static_cache(model.config, 32 if name != "qwen2-4" else 16))
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert torch.equal(fused.prefill, want.prefill) and torch.equal(fused.steps, want.steps)
    assert [int(layer.cumulative_length) for layer in fused.cache.layers] == [inp.prompt + steps] * D.LAYERS


# ---- 9. the entry's host rules ---------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bqllm_attn_decode_ring\s*\(", header)
    assert "qllm_attn_decode_ring" in _lib.EXPORTS and C.cast(lib.qllm_attn_decode_ring, C.c_void_p).value
    ring, window = lib.qllm_attn_decode_ring.argtypes, lib.qllm_attn_decode_window.argtypes
    assert len(ring) == 32 and ring == window                                      # total, total_dev, slots, window where it has kv_len, kv_len_dev, max_len, window
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    not_built = open(os.path.join(ROOT, "qllm_amd", "csrc", "attn_decode.hip")).read().split("Not built")[1]
    assert "ring" not in not_built.split("\n#include")[0]
    doc = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    assert "Not built: a ring-buffer cache" not in doc and "Not built: chunked attention" in doc


def answer(lib, **kw):
    return R.ring_call(lib, **kw), _lib.last_error()


RULES = [
    # (overrides, status, what the text says)
    (dict(q=None), INV, "must not be NULL"),
    (dict(out=None), INV, "must not be NULL"),
    (dict(b=0), INV, "must be >= 1"),
    (dict(slots=0), INV, "must be >= 1"),
    (dict(hk=3), INV, "kv_heads must divide q_heads"),
    (dict(window=-1), INV, "window must be 0 (none) or >= 1 (got -1)"),
    (dict(dt=7), INV, "act_dtype"),
    (dict(mask_kind=3), INV, "mask_kind"),
    (dict(mask=None), INV, "mask must be NULL exactly"),
    (dict(window=0), INV, "1 <= window <= slots (got window=0 slots=100)"),
    (dict(window=101), INV, "1 <= window <= slots (got window=101 slots=100)"),
    (dict(slots=59), INV, "1 <= window <= slots (got window=60 slots=59)"),
    (dict(v_new=None), INV, "k_new and v_new must be given together"),
    (dict(k_new=None), INV, "k_new and v_new must be given together"),
    (dict(k_cache=R.RING_PTRS["k_cache"] + 8), INV, "16-byte aligned"),
    (dict(total_dev=R.RING_PTRS["total_dev"] + 4), INV, "8-byte aligned"),
    (dict(c_pos=4), INV, "multiples of 8"),
    (dict(kn_row=-8), INV, "multiples of 8"),
    (dict(total=-1), INV, "total must be >= 0 (got -1)"),
    (dict(mask_len=10), INV, "the mask must cover 11 positions"),                           # total 10 + the append
    (dict(total=59, mask_len=59), INV, "the mask must cover 60 positions"),                 # the step that fills
    (dict(total=1 << 40, mask_len=59), INV, "the mask must cover 60 positions"),            # never more than the window
    (dict(total_dev=R.RING_PTRS["total_dev"], mask_len=59), INV, "the mask must cover 60 positions (the window: the total is on the device)"),
    (dict(mask_batch=-60), INV, "non-negative batch stride"),
    (dict(d=96), UNS, "head_dim 64 and 128"),
    (dict(hq=18, hk=2), UNS, "query heads per kv head"),
    (dict(b=3000, hq=2, hk=2), UNS, "batch * kv_heads <= 4096"),
    (dict(), WS, "qllm_attn_decode_ring needs a 16-byte aligned workspace"),
    (dict(ws=R.RING_PTRS["ws"], ws_bytes=16384), WS, "(got 16384)"),
    (dict(ws=R.RING_PTRS["ws"] + 8), WS, "16-byte aligned workspace"),
    # what passes every rule but the workspace's: no upper end of the total, the mask of min(n, W) columns, no append
    (dict(total=(1 << 62)), WS, "workspace"),
    (dict(total=0, mask_len=1), WS, "workspace"),
    (dict(total=10, mask_len=11), WS, "workspace"),
    (dict(k_new=None, v_new=None, mask_len=10), WS, "workspace"),
    (dict(k_new=None, v_new=None, kn_row=4), WS, "workspace"),                              # the append's strides count with an append only
    (dict(slots=60), WS, "workspace"),                                                       # C = W
    (dict(total_dev=R.RING_PTRS["total_dev"], total=-5), WS, "workspace"),                   # the host total is not read then
    (dict(mask=None, mask_kind=_lib.ATTN_MASK_NONE, mask_len=0), WS, "workspace"),
]


@pytest.mark.parametrize("over,status,text", RULES, ids=[f"{i}-{'-'.join(o) or 'base'}" for i, (o, _, _) in enumerate(RULES)])
def test_every_rule_of_the_entry(lib, over, status, text):
    rc, msg = answer(lib, **over)
    assert rc == status and text in msg, (rc, msg)


PAIRS = [
    # (the fault that wins, the fault that loses): the order of the rules
    (dict(q=None), dict(b=0)),
    (dict(slots=0), dict(window=-1)),
    (dict(window=-1), dict(dt=7)),
    (dict(mask_kind=3), dict(window=0)),
    (dict(mask=None), dict(slots=59)),
    (dict(window=0), dict(v_new=None)),
    (dict(slots=59), dict(k_cache=R.RING_PTRS["k_cache"] + 8)),
    (dict(v_new=None), dict(c_pos=4)),
    (dict(q_row=4), dict(total=-1)),
    (dict(total=-1), dict(mask_len=5)),
    (dict(mask_len=5), dict(d=96)),
    (dict(d=96), dict(ws=R.RING_PTRS["ws"] + 8)),
    (dict(b=3000, hq=2, hk=2), dict(ws_bytes=0)),
]


@pytest.mark.parametrize("first,second", PAIRS, ids=[f"{'-'.join(a)}-over-{'-'.join(b)}" for a, b in PAIRS])
def test_which_rule_wins(lib, first, second):
    alone, both = answer(lib, **first), answer(lib, **dict(first, **second))
    assert both == alone and answer(lib, **second) != alone, (alone, both)


def test_the_messages_shared_with_the_decode_entry_are_its_own(lib):
    """The helpers are the decode entry's: the same fault gives the same status and text there, with slots where it has max_len."""
    import attn_entry_cases as E
    shared = (dict(q=None), dict(b=0), dict(hk=3), dict(window=-1), dict(dt=7), dict(mask_kind=3), dict(mask=None), dict(v_new=None), dict(c_pos=4), dict(d=96),
              dict(hq=18, hk=2), dict(b=3000, hq=2, hk=2))
    for over in shared:
        rc = E.decode_call(lib, **dict(E.BASE["decode"], window=over.get("window", 0), **{k: v for k, v in over.items() if k != "window"}))
        assert (rc, _lib.last_error()) == answer(lib, **over), over


@pytest.mark.parametrize("b,hq,hk,d,w", [(2, 4, 2, 64, 60), (1, 32, 8, 128, 4096), (3, 7, 1, 128, 197), (1, 8, 2, 64, 389), (64, 32, 32, 128, 4096)])
def test_the_ring_workspace_is_the_linear_call_of_max_len_w(lib, b, hq, hk, d, w):
    """Geometry, workspace and describe text are those of a linear call whose max_len is the window, whatever the slots: one byte short is
    refused with that very figure, and the linear entry asks the same of a cache of W positions."""
    import attn_entry_cases as E
    need = lib.qllm_attn_decode_workspace_bytes(b, hq, hk, d, w)
    assert need > 16384
    strides = (hq * d, d, hk * d, d, hk * d, d, 0, 0, d)
    for slots in (w, w + 37, 4 * w):
        rc, msg = answer(lib, b=b, hq=hq, hk=hk, d=d, window=w, slots=slots, strides=strides, mask_len=w, mask_batch=w, ws=R.RING_PTRS["ws"], ws_bytes=need - 1)
        assert rc == WS and f"workspace of {need} bytes (got {need - 1})" in msg, msg
    rc = E.decode_call(lib, b=b, hq=hq, hk=hk, d=d, kv_len=0, max_len=w, strides=strides, mask_len=w, mask_batch=w, ws=E.DECODE_PTRS["ws"], ws_bytes=need - 1)
    assert rc == WS and f"workspace of {need} bytes (got {need - 1})" in _lib.last_error()


# ---- the op's plan -----------------------------------------------------------------------------------------------------------------------------------------
def tensors(b=2, hq=8, hk=2, d=64, slots=40, dtype=torch.float16, seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=g).to(dtype)
    return r(b, 1, hq, d).transpose(1, 2), r(b, hk, slots, d), r(b, hk, slots, d), r(b, 1, hk, d).transpose(1, 2), r(b, 1, hk, d).transpose(1, 2)


def test_the_plan_and_what_the_op_refuses():
    q, k, v, kn, vn = tensors()
    plan = ops.attn_decode_ring_plan(q, k, v, 7, 30)
    assert plan == (2, 8, 2, 64, 40, 30, 512, 64, 0, 0, 0, 0, 2 * 40 * 64, 40 * 64, 64, 0, 0, 0)
    linear = ops.attn_decode_plan(q, k, v, 7)
    assert plan[:5] + plan[6:] == linear                                                   # the linear plan, with the window behind the slots
    assert ops.attn_decode_ring_plan(q, k, v, 10 ** 15, 40, kn, vn)[8:12] == (128, 64, 128, 64)          # no upper end; W = C
    mask = torch.ones(2, 1, 1, 30, dtype=torch.bool)
    assert ops.attn_decode_ring_plan(q, k, v, torch.tensor(5), 30, mask=mask)[-3:] == (_lib.ATTN_MASK_BOOL, 30, 30)
    assert ops.attn_decode_ring_plan(q, k, v, 4, 30, kn, vn, mask=mask[..., :5])[-3:] == (_lib.ATTN_MASK_BOOL, 5, 30)
    assert ops.attn_decode_ring_plan(q, k, v, 1000, 30, kn, vn, mask=mask)[-2] == 30
    refused = [
        (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 41), "window"), (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 0), "window"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, 7, None), "window"), (lambda: ops.attn_decode_ring_plan(q, k, v, 7, True), "window"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 4.0), "window"), (lambda: ops.attn_decode_ring_plan(q, k, v, -1, 30), "total"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 30, kn), "together"), (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 30, mask=mask[..., :6]), "cover 7"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 30, kn, vn, mask=mask[..., :7]), "cover 8"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, 100, 30, mask=mask[..., :29]), "cover 30"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, torch.tensor(5), 30, mask=mask[..., :29]), "cover 30"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, torch.tensor(5, dtype=torch.int32), 30), "0-d int64"),
        (lambda: ops.attn_decode_ring_plan(q.float(), k, v, 7, 30), "one type"), (lambda: ops.attn_decode_ring_plan(q, k, v[:, :, :39], 7, 30), "caches"),
        (lambda: ops.attn_decode_ring_plan(q[:, :5], k, v, 7, 30), "divide"), (lambda: ops.attn_decode_ring_plan(q[..., :32], k[..., :32], v[..., :32], 7, 30), "head_dim"),
        (lambda: ops.attn_decode_ring_plan(q, k, v, 7, 30, kn[:, :1], vn[:, :1]), "one token of"),
    ]
    for call, text in refused:
        with pytest.raises(ops.QllmUnsupported, match=text):
            call()
    with pytest.raises(RuntimeError, match="HIP/CUDA tensors"):                           # a served call reaches the device check: no CPU path
        ops.attn_decode_ring(q, k, v, 7, 30)
    import inspect
    assert list(inspect.signature(ops.attn_decode_ring).parameters) == ["q", "k_cache", "v_cache", "total", "window", "k_new", "v_new", "mask", "scaling", "out", "plan"]
    assert [p.kind for p in inspect.signature(ops.attn_decode_ring).parameters.values()][-2:] == [inspect.Parameter.KEYWORD_ONLY] * 2


def test_the_restatement_is_the_linear_restatement_over_the_visible_positions():
    import attn_decode_cases as AD
    b, hq, hk, d, w, slots = 2, 4, 2, 64, 9, 12
    q, rows_k, rows_v = R.stream(b, hq, hk, d, w, torch.float16, 3)
    for total in (0, 1, 8, 9, 10, 23, (1 << 40) + 7):
        n, lo, v = R.view(total, True, w)
        k_ring, v_ring = R.ring_of(rows_k, lo, v - 1, slots), R.ring_of(rows_v, lo, v - 1, slots)
        mask, _ = R.mask_of("bool", b, w, v, torch.float16)
        got = R.ring_restated(q, k_ring, v_ring, total, w, rows_k[:, :, v - 1:v], rows_v[:, :, v - 1:v], mask=mask)
        want = AD.restated(q, R.linear_of(rows_k, v, w), R.linear_of(rows_v, v, w), v, mask=mask)
        assert torch.equal(got, want) and bool(torch.isfinite(got.float()).all()), total
        assert torch.equal(k_ring[:, :, (n - 1) % slots], rows_k[:, :, v - 1])


@pytest.mark.parametrize("extra", [0, R.EXTRA_SLOTS])
def test_the_premises_of_the_selection_inputs(extra):
    """The target scores 512, every other visible key 0, every hidden slot the ring still holds 1024 with V = NaN; the targets name lo,
    the appended row, each split's first position and the two slots of the seam; the restatement returns V[target] bit for bit."""
    b, hq, hk, d, dtype = 2, 7, 1, 128, torch.bfloat16
    w, chunk = R.window_of(d), 64
    slots = w + extra
    for total in (w - 1, 2 * w + 35, (1 << 40) + 7):
        n, lo, v = R.view(total, True, w)
        targets = R.selection_targets(w, slots, total, chunk)
        assert {0, v - 1} | set(range(0, v, chunk)) <= set(targets) and all(0 <= r < v for r in targets)
        if total >= slots:
            assert {(lo + r) % slots for r in targets} >= {0, slots - 1} or extra                     # C = W: both seam slots are visible
        for target in targets:
            q, k_ring, v_ring, k_new, v_new, want = R.selection(b, hq, hk, d, w, slots, total, target, dtype)
            k_all = k_ring.clone()
            k_all[:, :, (n - 1) % slots] = k_new[:, :, 0]
            scores = torch.einsum("d,sd->s", q[0, 0, 0].double(), k_all[0, 0].double()) * R.SEL_SCALING
            seen = {(lo + r) % slots: r for r in range(v)}
            held = {j % slots for j in range(max(0, n - slots), lo)}
            assert len(held) == min(extra, max(0, n - w)) and not held & set(seen)
            for slot in range(slots):
                if slot in seen:
                    assert scores[slot] == (512 if seen[slot] == target else 0)
                elif slot in held:
                    assert scores[slot] == 1024 and bool(torch.isnan(v_ring[:, :, slot]).all())
                else:
                    assert bool(torch.isnan(scores[slot])) and bool(torch.isnan(v_ring[:, :, slot]).all())
            got = R.ring_restated(q, k_ring, v_ring, total, w, k_new, v_new, scaling=R.SEL_SCALING)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)) and bool(torch.isfinite(want.float()).all())


# ---- 10. the modules -----------------------------------------------------------------------------------------------------------------------------------------
def test_the_ring_kind_is_the_ring_class_alone(monkeypatch):
    from types import SimpleNamespace
    from transformers.cache_utils import DynamicLayer, DynamicSlidingWindowLayer, StaticLayer, StaticSlidingWindowLayer

    class Sub(RingSlidingWindowLayer):
        pass

    def kind(layer, sliding, offloading=False, **kw):
        return fused_attention._layer_of(SimpleNamespace(layers=[layer], offloading=offloading), 0, sliding=sliding, **kw)[1]

    def ring(max_cache_len=16, sliding_window=4, cls=RingSlidingWindowLayer, init=False):
        layer = cls(max_cache_len=max_cache_len, sliding_window=sliding_window)
        if init:
            layer.update(torch.zeros(1, 2, 1, 8), torch.zeros(1, 2, 1, 8))
        return layer

    assert kind(ring(init=True), 4) == "ring_sliding" and kind(ring(), 4, uninitialized=True) == "ring_sliding"
    assert kind(ring(max_cache_len=3, init=True), 4) == "ring_sliding"                                               # holds 3 <= 4
    assert kind(ring(), 4) is None                                                                                   # not initialised: prefill only
    assert kind(ring(cls=Sub, init=True), 4) is None and kind(ring(sliding_window=6, init=True), 4) is None          # a subclass; holds 6 > 4
    assert kind(ring(init=True), None) is None and kind(ring(init=True), True) is None and kind(ring(init=True), 0) is None
    assert kind(ring(init=True), 4, offloading=True) is None
    # the four kinds there were
    assert kind(DynamicLayer(), None) == "dynamic" and kind(StaticLayer(max_cache_len=16), None, uninitialized=True) == "static"
    assert kind(DynamicSlidingWindowLayer(sliding_window=4), 4) == "dynamic_sliding"
    assert kind(StaticSlidingWindowLayer(max_cache_len=16, sliding_window=4), 4, uninitialized=True) == "static_sliding"
    routed = fused_attention._prefill_routed
    assert {k for k, _ in fused_attention.PREFILL_ROUTES} == {"dynamic", "static", "dynamic_sliding", "static_sliding"}    # the table has no ring entry:
    for masked in (False, True):                                                                                            # the ring is looked up as static_sliding
        for q_len in (2, 3, 8, 9, 2048, 2049, 8192):
            for behind in (False, True):
                for window in (4, 4096):
                    assert routed("ring_sliding", masked, q_len, behind, window) == routed("static_sliding", masked, q_len, behind, window)
    monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "0")
    assert kind(ring(init=True), 4) is None and kind(DynamicLayer(), None) == "dynamic"


def ring_restatements(monkeypatch):
    """The three ops replaced by recorders around their torch restatements; -> (the sliding recorder's calls, the ring calls)."""
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    fake_rope(monkeypatch)
    calls, ring = S.record(monkeypatch, S.decode_restated, S.prefill_restated), []

    def op(q, k_cache, v_cache, total, window, *a, **kw):
        ring.append((int(total), isinstance(total, torch.Tensor), window, k_cache.shape[2], kw.get("k_new") is not None and kw.get("v_new") is not None,
                     None if kw.get("mask") is None else kw["mask"].shape[-1]))
        return R.ring_restated(q, k_cache, v_cache, total, window, *a, **kw)

    monkeypatch.setattr(ops, "attn_decode_ring", op)
    return calls, ring


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_a_ring_cache_decodes_through_the_ring_op(name, batch, monkeypatch):
    """Every decode step of a sliding layer -- before, at and far past the fill -- is ONE call of ops.attn_decode_ring over the layer's
    own buffers with the total on the device and the append, never ops.attn_decode; full layers go as they did.  With the restatements
    in the kernels' place the logits are those of the plain StaticCache under the fusion, bit for bit, and within the CPU bound of the
    float64 model."""
    from transformers import StaticCache
    model, slides, window = S.sliding_model(name)
    ref = D.float64_copy(model)
    size = 16 if name == "qwen2-4" else 32
    inp = D.batch_inputs(batch, steps=11 if name == "qwen2-4" else 3 * window)
    reference, unfused = D.run(ref, inp), D.run(model, inp, StaticCache(config=model.config, max_cache_len=size))
    calls, ring = ring_restatements(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS
    try:
        static = D.run(model, inp, StaticCache(config=model.config, max_cache_len=size))
        del calls[:]
        fused = D.run(model, inp, ring_static_cache(model.config, size))
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    n_slide = sum(slides)
    assert [c.op for c in calls] == ["decode"] * ((D.LAYERS - n_slide) * inp.steps) and not any(c.has_window for c in calls)
    assert [c[:5] for c in ring] == [(inp.prompt + t, True, window, window, True) for t in range(inp.steps) for _ in range(n_slide)]
    assert all(c[5] in (None, window) for c in ring) and (inp.mask is None or all(c[5] == window for c in ring))       # the mask's W columns, indexed by r
    assert [int(layer.cumulative_length) for layer in fused.cache.layers] == [inp.prompt + inp.steps] * D.LAYERS
    assert D.same_bits(fused.prefill, static.prefill) and D.same_bits(fused.steps, static.steps)
    D.assert_case(fused, unfused, reference, D.M_CPU, label=f"cpu ring {name} {batch}")


def test_the_kill_switch_and_a_refusing_plan_leave_the_ring_to_update(monkeypatch):
    from transformers import StaticCache
    model, slides, window = S.sliding_model("mistral-4")
    inp = D.batch_inputs("padded", steps=12)
    unfused = D.run(model, inp, StaticCache(config=model.config, max_cache_len=32))
    calls, ring = ring_restatements(monkeypatch)
    S.open_routes(monkeypatch)
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "0")
        off = D.run(model, inp, ring_static_cache(model.config, 32))
        assert calls == [] and ring == [] and D.same_bits(off.prefill, unfused.prefill) and D.same_bits(off.steps, unfused.steps)
        monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "1")

        def refuse(*a, **kw):
            raise ops.QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "attn_decode_ring: refused by the test")

        monkeypatch.setattr(ops, "attn_decode_ring_plan", refuse)
        monkeypatch.setattr(fused_attention, "PREFILL_ROUTES", {})
        refused = D.run(model, inp, ring_static_cache(model.config, 32))
        assert calls == [] and ring == [] and D.same_bits(refused.steps, unfused.steps)                # `update` once, the family's route
        assert [int(layer.cumulative_length) for layer in refused.cache.layers] == [inp.prompt + inp.steps] * D.LAYERS
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS


PIECES = ((0, 5), (5, 8), (8, 9), (9, 10))               # a prompt longer than a window of 4, a chunk behind it, two decode steps
LONG = ((0, 11), (11, 12))                               # a prompt longer than either window


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("pieces", [PIECES, LONG], ids=["chunks", "long prompt"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_prompts_and_chunks_on_a_ring_cache_are_the_static_sliding_layers_calls(name, pieces, batch, monkeypatch):
    """Prefill on a ring layer: `update` as on a static sliding layer, and the very call of ops.attn_prefill -- length, where it comes
    from, what `update` returned, the window -- that the static sliding layer's route makes; the logits are its bits."""
    model, slides, window = S.sliding_model(name)
    inp = D.batch_inputs(batch)
    calls, ring = ring_restatements(monkeypatch)
    S.open_routes(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        static, _ = S.forwards(model, inp, "static", "cpu", pieces)
        want_calls = [vars(c) for c in calls if c.op == "prefill"]
        del calls[:]
        monkeypatch.setattr(D, "make_cache", lambda m, kind: ring_static_cache(m.config, D.MAX_CACHE_LEN))
        fused, cache = S.forwards(model, inp, "static", "cpu", pieces)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    assert [type(layer) is RingSlidingWindowLayer for layer in cache.layers] == slides
    assert [vars(c) for c in calls if c.op == "prefill"] == want_calls and len(want_calls) == D.LAYERS * sum(b - a > 1 for a, b in pieces)
    assert len(ring) == sum(slides) * sum(b - a == 1 for a, b in pieces)
    assert D.same_bits(fused, static)


# ---- 11. kernel resources ----------------------------------------------------------------------------------------------------------------------------------
def test_the_ring_kernels_use_no_scratch_spill_nothing_and_add_no_lds():
    """attn_decode_ring.hip holds 32 kernels of a name of their own; kernel for kernel no scratch, no spills and the LDS of the kernel
    without a window.  The other two units hold the 32 kernels they held, under their pinned names."""
    from kernel_resources import resources
    ring, plain, win = resources("attn_decode_ring.hip"), resources("attn_decode.hip"), resources("attn_decode_window.hip")
    assert len(ring) == len(plain) == len(win) == 32, (sorted(ring), sorted(plain), sorted(win))
    assert all("attn_decode_ring_kernel" in n for n in ring) and not any("ring" in n for n in list(plain) + list(win))
    assert all("attn_decode_kernel" in n and n.endswith("Lb0EEEvNS_16AttnDecodeParamsE") for n in plain)
    assert all("attn_decode_kernel" in n and n.endswith("Lb1EEEvNS_16AttnDecodeParamsE") for n in win)
    for n, r in sorted(ring.items()):
        bf16, d, g = re.search(r"ILb(\d)ELi(\d+)ELi(\d+)E", n).groups()
        base = [v for k, v in plain.items() if f"ILb{bf16}ELi{d}ELi{g}ELb0E" in k]
        assert len(base) == 1, n
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert r["group_segment_fixed_size"] == base[0]["group_segment_fixed_size"] > 0, (n, r, base[0])
