"""No GPU: the sliding window of qllm_attn_decode_window / qllm_attn_prefill_window as far as a host reaches -- the symbols, their
validation, the `window` keyword of the ops -- the torch restatements against the float64 oracles with the band handed in as a mask, and
the routing of q_layers/fused_attention.py on tiny Mistral and Qwen2 models whose layers slide, with the restatements in the kernels'
place (tests/attn_sliding_cases.py).  The ratios are printed per case (pytest -s) and recorded in profiles/attn_sliding.md."""
import ctypes as C
import os
import re

import pytest
import torch

import attn_decode_cases as AD
import attn_prefill_cases as AP
import attn_sliding_cases as S
import decode_loop_cases as D
from test_rope_cpu import fake_op as fake_rope

from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS, WS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_WORKSPACE


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


# ---- symbols and validation ------------------------------------------------------------------------------------------------------------------------
def test_the_two_symbols_are_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read(), flags=re.S)
    for name in ("qllm_attn_decode_window", "qllm_attn_prefill_window"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and C.cast(getattr(lib, name), C.c_void_p).value, name
    # the entries without a window keep their parameter lists; the new ones have `int64_t window` behind max_len
    assert len(lib.qllm_attn_decode.argtypes) == 31 and len(lib.qllm_attn_prefill.argtypes) == 27
    dw, pw = lib.qllm_attn_decode_window.argtypes, lib.qllm_attn_prefill_window.argtypes
    assert dw[:14] + dw[15:] == lib.qllm_attn_decode.argtypes and dw[14] is C.c_int64
    assert pw[:13] + pw[14:] == lib.qllm_attn_prefill.argtypes and pw[13] is C.c_int64
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    for text in ("attn_decode.hip", "attn_prefill.hip"):
        assert "sliding-window" not in open(os.path.join(ROOT, "qllm_amd", "csrc", text)).read().split("Not built:")[1]


def test_a_negative_window_is_invalid_and_a_window_without_causality_unsupported(lib):
    buf = torch.zeros(1 << 14, dtype=torch.float16)
    p = buf.data_ptr()

    def decode(window):
        return lib.qllm_attn_decode_window(p, None, None, p, p, None, p, 2, 8, 2, 64, 10, None, 100, window, 512, 64, 0, 0, 0, 0, 12800, 6400, 64, 0, 0, 0,
                                           0.125, 0, None, 0, None)

    def prefill(window, causal=1):
        return lib.qllm_attn_prefill_window(p, p, p, None, p, 2, 8, 2, 64, 5, 10, None, 100, window, 2560, 64, 512, 12800, 6400, 64, 0, 0, 0, 0, causal,
                                            0.125, 0, None)

    assert decode(-1) == INV and "window" in _lib.last_error() and "-1" in _lib.last_error()
    assert prefill(-1) == INV and "window" in _lib.last_error()
    assert prefill(-1, causal=0) == INV                                                     # the sign first
    # valid windows get as far as the calls without one: the missing workspace (decode), and for prefill -- which needs none -- the launch
    # itself, so only its refusal is asked for here
    assert decode(0) == WS and decode(1) == WS and decode(1 << 40) == WS
    assert prefill(3, causal=0) == UNS and "causal" in _lib.last_error()
    assert lib.qllm_attn_decode(p, None, None, p, p, None, p, 2, 8, 2, 64, 10, None, 100, 512, 64, 0, 0, 0, 0, 12800, 6400, 64, 0, 0, 0, 0.125, 0, None, 0, None) == WS


def tensors(b=2, hq=8, hk=2, d=64, L=40, s=1, dtype=torch.float16, seed=1):
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, s, hq, d, generator=g).to(dtype).transpose(1, 2)
    return q, torch.randn(b, hk, L, d, generator=g).to(dtype), torch.randn(b, hk, L, d, generator=g).to(dtype)


@pytest.mark.parametrize("bad", [0, -1, 2.0, "4", True, torch.tensor(4)], ids=repr)
def test_the_ops_refuse_an_invalid_window_before_a_launch(bad):
    """On CPU tensors: a served window would reach the device check (RuntimeError); a refused one never does."""
    q, k, v = tensors()
    with pytest.raises(ops.QllmUnsupported, match="window"):
        ops.attn_decode(q, k, v, 7, window=bad)
    with pytest.raises(ops.QllmUnsupported, match="window"):
        ops.attn_prefill(tensors(s=5)[0], k, v, 7, window=bad)


def test_a_valid_window_reaches_the_device_check_and_the_plans_do_not_know_it():
    q, k, v = tensors()
    q5 = tensors(s=5)[0]
    for window in (None, 1, 4, 10 ** 12):
        with pytest.raises(RuntimeError, match="HIP/CUDA tensors"):
            ops.attn_decode(q, k, v, 7, window=window)
        with pytest.raises(RuntimeError, match="HIP/CUDA tensors"):
            ops.attn_prefill(q5, k, v, 7, window=window)
    with pytest.raises(ops.QllmUnsupported, match="causal"):
        ops.attn_prefill(q5, k, v, 7, causal=False, window=4)
    assert ops.attn_decode_plan(q, k, v, 7) == (2, 8, 2, 64, 40, 512, 64, 0, 0, 0, 0, 2 * 40 * 64, 40 * 64, 64, 0, 0, 0)
    assert ops.attn_prefill_plan(q5, k, v, 7) == (2, 8, 2, 64, 5, 40, 5 * 512, 64, 512, 2 * 40 * 64, 40 * 64, 64, 0, 0, 0, 0)
    import inspect
    assert "window" not in inspect.signature(ops.attn_decode_plan).parameters and "window" not in inspect.signature(ops.attn_prefill_plan).parameters
    for f in (ops.attn_decode, ops.attn_prefill):
        par = inspect.signature(f).parameters["window"]
        assert par.kind is par.KEYWORD_ONLY and par.default is None


# ---- the restatements --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", [1, 2, 5, 17, 18, 40])
def test_the_decode_restatement_with_a_window_is_the_oracle_behind_a_band(window):
    q, k, v = tensors()
    n = 17
    pad = torch.ones(2, 40, dtype=torch.bool)
    pad[1, :14] = False
    for mask in (None, pad, AP.as_mask(pad, "additive", torch.float16)):
        vis = S.decode_band(n, window, 40).expand(2, 40) & (pad if mask is not None else True)
        ref = AD.oracle(q[:, :, 0], k, v, n, 0.125, visible=vis)
        got = S.decode_restated(q, k, v, n, mask=mask, window=window)
        assert (got.double() - ref).abs().max() <= (AD.eager(q[:, :, 0], k, v, n, 0.125, AP.as_mask(vis, "additive", torch.float16)).double() - ref).abs().max()
    # the appended token counts inside the window
    kn, vn = k[:, :, 17:18].clone(), v[:, :, 17:18].clone()
    assert torch.equal(S.decode_restated(q, k.clone(), v.clone(), 17, kn, vn, window=window), S.decode_restated(q, k, v, 18, window=window))
    if window >= n:
        assert torch.equal(S.decode_restated(q, k, v, n, window=window), AD.restated(q, k, v, n))


@pytest.mark.parametrize("window", [1, 2, 5, 12, 40])
def test_the_prefill_restatement_with_a_window_is_the_oracle_behind_a_band(window):
    q, k, v = tensors(s=7)
    n = 12
    pad = AP.left_padded(2, 7, n - 7, 40, (0, 6), "bool", torch.float16)
    for mask in (None, pad, AP.as_mask(pad, "additive", torch.float16)):
        band = S.prefill_band(7, n, window, 40)
        vis = (band[:, None] & pad) if mask is not None else band[:, None].expand(2, 1, 7, 40)
        ref = AP.oracle(q, k, v, n, 0.125, mask=vis)
        got = S.prefill_restated(q, k, v, n, mask=mask, scaling=0.125, window=window)
        assert (got.double() - ref).abs().max() <= (AP.eager(q, k, v, n, 0.125, mask=vis).double() - ref).abs().max()
    if window >= n:
        assert torch.equal(S.prefill_restated(q, k, v, n, window=window), AP.restated(q, k, v, n))


@pytest.mark.parametrize("s,q_start,window", [(129, 5, 63), (300, 100, 64), (2, 0, 1), (200, 64, 269), (127, 100, 1), (128, 0, 129)])
def test_the_premises_of_the_window_selection_inputs(s, q_start, window):
    """The best match of every row sits at p - W, 256 above the row's target p - W + 1, which leads every other key by 256 and more
    (369 in the log2 domain: weight exactly 0); the restatement returns the target's V row bit for bit."""
    q, k, v, target, scaling = S.window_selection(1, 2, 1, 64, s, q_start, window, torch.bfloat16)
    n = q_start + s
    scores = torch.einsum("sd,nd->sn", q[0, 0].double(), k[0, 0].double()) * scaling
    p, j = q_start + torch.arange(s), torch.arange(n)
    for i in range(s):
        row = scores[i]
        if p[i] - window >= 0:
            assert int(row.argmax()) == p[i] - window and row[p[i] - window] - row[target[i]] == 256
        seen = row.masked_fill(~((j <= p[i]) & (j > p[i] - window)), float("-inf"))
        assert int(seen.argmax()) == target[i] == max(0, p[i] - window + 1)
        seen[target[i]] = float("-inf")
        assert row[target[i]] - seen.max() >= 256
    assert torch.equal(S.prefill_restated(q, k, v, n, scaling=scaling, window=window), S.window_selection_expected(v, target, 2))


# ---- the modules ---------------------------------------------------------------------------------------------------------------------------------------
def restatements(monkeypatch):
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    fake_rope(monkeypatch)
    return S.record(monkeypatch, S.decode_restated, S.prefill_restated)


def check_decode_calls(calls, cache, slides, window, inp):
    """One call per layer and decode step, none at the prompt; `window` passed on sliding layers and absent on full ones; the length the
    valid positions of what `update` returned -- after a static sliding layer overflows, all of them, as a host int."""
    assert [c.op for c in calls] == ["decode"] * (D.LAYERS * inp.steps), [c.op for c in calls]
    for t in range(inp.steps):
        for layer in range(D.LAYERS):
            c = calls[t * D.LAYERS + layer]
            assert (c.has_window, c.window) == ((True, window) if slides[layer] else (False, None)), (t, layer, c)
            assert (c.length, c.on_device, c.returned) == S.expected_decode_call(cache, slides[layer], window, inp.prompt + t + 1), (t, layer, c)
            if slides[layer] and cache == "static" and inp.prompt + t + 1 > window:
                assert not c.on_device and c.length == c.returned == window


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_sliding_layers_decode_through_the_op_with_their_window(name, cache, batch, monkeypatch):
    model, slides, window = S.sliding_model(name)
    ref = D.float64_copy(model)
    inp = D.batch_inputs(batch)
    reference, unfused = D.run(ref, inp), D.run(model, inp, cache)
    calls = restatements(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS
    try:
        fused = D.run(model, inp, cache)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    check_decode_calls(calls, cache, slides, window, inp)
    D.assert_case(fused, unfused, reference, D.M_CPU, label=f"cpu sliding {name} {cache} {batch}")
    if cache == "static" and inp.prompt > window:       # what the issue records: a 5-token prompt into a window of 4 leaves the counter at 0
        assert [int(layer.cumulative_length) for layer, s in zip(fused.cache.layers, slides) if s] == [0] * sum(slides)


PIECES = ((0, 5), (5, 8), (8, 9), (9, 10))               # a prompt, a chunk of three behind it, two decode steps


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_prompts_and_chunks_on_sliding_layers_go_through_the_prefill_op(name, cache, batch, monkeypatch):
    model, slides, window = S.sliding_model(name)
    ref = D.float64_copy(model)
    inp = D.batch_inputs(batch)
    reference, _ = S.forwards(ref, inp, "dynamic", "cpu", PIECES)
    unfused, _ = S.forwards(model, inp, cache, "cpu", PIECES)
    calls = restatements(monkeypatch)
    S.open_routes(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused, _ = S.forwards(model, inp, cache, "cpu", PIECES)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    # one call per layer and forward: the prompt, the chunk, then the decode steps
    assert [(c.op, c.q_len) for c in calls] == [("prefill", 5)] * D.LAYERS + [("prefill", 3)] * D.LAYERS + [("decode", 1)] * (2 * D.LAYERS), calls
    for i, c in enumerate(calls):
        assert (c.has_window, c.window) == ((True, window) if slides[i % D.LAYERS] else (False, None)), (i, c)
        if slides[i % D.LAYERS] and not c.on_device:
            assert c.length == c.returned                                        # every position `update` returned is valid
    for i, (c, tokens) in enumerate(zip(calls[:2 * D.LAYERS], (5, 5, 8, 8))):      # the prompt and the chunk of a sliding layer
        if slides[i % D.LAYERS]:
            before = tokens - c.q_len
            if cache == "dynamic":
                want = (min(before, window - 1) + c.q_len, False)
            else:
                want = (tokens, True) if tokens <= window else ((before if before < window else window - 1) + c.q_len, False)
            assert (c.length, c.on_device) == want, (c, want)
    assert bool(torch.isfinite(fused.float()).all())
    e_unfused, e_fused = (unfused.double() - reference).abs().max().item(), (fused.double() - reference).abs().max().item()
    print(f"cpu sliding prefill {name} {cache} {batch}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    assert e_unfused > 0 and e_fused <= D.M_CPU * e_unfused


@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_the_kill_switch_restores_the_family_route(cache, monkeypatch):
    model, slides, window = S.sliding_model("mistral-4")
    inp = D.batch_inputs("padded")
    unfused = D.run(model, inp, cache)
    calls = restatements(monkeypatch)
    S.open_routes(monkeypatch)
    monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "0")
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused = D.run(model, inp, cache)
        assert calls == [] and D.same_bits(fused.prefill, unfused.prefill) and D.same_bits(fused.steps, unfused.steps)
        monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "1")
        D.run(model, inp, cache)
        assert len(calls) == D.LAYERS * (1 + inp.steps)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS


def test_what_stays_on_the_family_route(monkeypatch):
    """A subclass of a sliding layer, and a sliding layer met without a window: no call, the family's bits.  (The family's own route
    does not run a window on full layers, a layer of another window or one that records its past -- its mask has another width --, so
    those are held at `_layer_of`: `test_the_layers_the_core_accepts`.)"""
    from transformers import DynamicCache
    from transformers.cache_utils import DynamicSlidingWindowLayer
    model, slides, window = S.sliding_model("mistral-4")
    inp = D.batch_inputs("padded")
    calls = restatements(monkeypatch)
    S.open_routes(monkeypatch)

    class Sub(DynamicSlidingWindowLayer):
        pass

    def cache():
        c = DynamicCache(config=model.config)
        c.layers = [Sub(sliding_window=4) for _ in range(D.LAYERS)]
        return c

    want = D.run(model, inp, cache(), steps=2)
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        got = D.run(model, inp, cache(), steps=2)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert calls == []
    assert D.same_bits(got.prefill, want.prefill) and D.same_bits(got.steps, want.steps)
    # a sliding layer met without a window: a Mistral whose config has none, handed a cache of sliding layers
    from test_attn_decode_cpu import tiny_model
    plain = tiny_model("mistral")
    assert install_fused_attention(plain, prefill=True) == D.LAYERS
    c = DynamicCache(config=plain.config)
    c.layers = [DynamicSlidingWindowLayer(sliding_window=4) for _ in range(D.LAYERS)]
    D.run(plain, inp, c, steps=2)
    assert calls == []
    D.run(plain, inp, "dynamic", steps=2)
    assert [c.has_window for c in calls] == [False] * (D.LAYERS * 3)                  # its own full layers are served, without the keyword


def test_the_layers_the_core_accepts(monkeypatch):
    from transformers.cache_utils import DynamicLayer, DynamicSlidingWindowLayer, StaticLayer, StaticSlidingWindowLayer

    class SubD(DynamicSlidingWindowLayer):
        pass

    class SubS(StaticSlidingWindowLayer):
        pass

    def kind(layer, sliding, offloading=False, **kw):
        from types import SimpleNamespace
        return fused_attention._layer_of(SimpleNamespace(layers=[layer], offloading=offloading), 0, sliding=sliding, **kw)[1]

    recording = DynamicSlidingWindowLayer(sliding_window=4)
    recording.activate_past_recording()
    assert kind(DynamicSlidingWindowLayer(sliding_window=4), 4) == "dynamic_sliding"
    assert kind(StaticSlidingWindowLayer(max_cache_len=16, sliding_window=4), 4, uninitialized=True) == "static_sliding"
    assert kind(StaticSlidingWindowLayer(max_cache_len=3, sliding_window=4), 4, uninitialized=True) == "static_sliding"     # holds 3 <= 4
    assert kind(StaticSlidingWindowLayer(max_cache_len=16, sliding_window=4), 4) is None                                   # not initialised: prefill only
    for layer, sliding in ((DynamicSlidingWindowLayer(sliding_window=5), 4), (SubD(sliding_window=4), 4), (recording, 4),
                           (StaticSlidingWindowLayer(max_cache_len=16, sliding_window=6), 4), (SubS(max_cache_len=16, sliding_window=4), 4),
                           (DynamicLayer(), 4), (StaticLayer(max_cache_len=16), 4), (DynamicSlidingWindowLayer(sliding_window=4), None),
                           (StaticSlidingWindowLayer(max_cache_len=16, sliding_window=4), None), (DynamicSlidingWindowLayer(sliding_window=4), True),
                           (DynamicSlidingWindowLayer(sliding_window=0), 0)):
        assert kind(layer, sliding, uninitialized=True) is None, (layer, sliding)
    assert kind(DynamicSlidingWindowLayer(sliding_window=4), 4, offloading=True) is None
    assert kind(DynamicLayer(), None) == "dynamic" and kind(StaticLayer(max_cache_len=16), None, uninitialized=True) == "static"
    monkeypatch.setenv("QLLM_FUSE_ATTENTION_SLIDING", "0")
    assert kind(DynamicSlidingWindowLayer(sliding_window=4), 4) is None and kind(DynamicLayer(), None) == "dynamic"


def test_generate_on_sliding_layers_is_judged_by_the_reference(monkeypatch):
    model, slides, window = S.sliding_model("mistral-4")
    ref = D.float64_copy(model)
    inp = D.batch_inputs("padded")
    e_unfused = D.error(D.run(model, inp), D.run(ref, inp))
    restatements(monkeypatch)
    calls = D.count_calls(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS
    for cache in ("dynamic", "static"):
        D.assert_generation(model, ref, inp, cache, e_unfused, D.M_CPU, calls, label=f"cpu sliding mistral-4 {cache}")


def test_the_routes_name_the_two_sliding_kinds_and_the_docstring_the_capture_limit():
    assert {k for k, _ in fused_attention.PREFILL_ROUTES} == {"dynamic", "static", "dynamic_sliding", "static_sliding"}
    for key in (("dynamic", False), ("dynamic", True), ("static", False), ("static", True)):
        assert fused_attention.PREFILL_ROUTES[key] == {("dynamic", True): (2, 128, False)}.get(key, (2, None, True))   # the full layers' as they were
    assert "captured" in fused_attention.__doc__ and "QLLM_FUSE_ATTENTION_SLIDING" in fused_attention.__doc__


def test_the_sliding_routes_are_written_in_windows():
    """Measured at W = 4096 only: with a mask, first prompts inside half a window up to the measured row counts, and from two windows on;
    no chunk behind cached tokens; one window (which loses) and everything between one and two (not measured) stay on the family's route,
    at every window."""
    routed = fused_attention._prefill_routed
    for window in (4, 1024, 4096, 32768, 131072):
        for kind, most in (("dynamic_sliding", 128), ("static_sliding", 2048)):
            inside = min(most, window // 2)
            for q_len, want in ((2, True), (inside, True), (inside + 1, False), (window, False), (2 * window - 1, False), (2 * window, True), (5 * window, True)):
                assert routed(kind, True, q_len, False, window) == (want and q_len >= 2), (kind, window, q_len)
                assert not routed(kind, True, q_len, True, window)
        assert routed("dynamic_sliding", False, 2, False, window) and routed("dynamic_sliding", False, window - 1, False, window)
        assert not routed("static_sliding", False, 2, False, window)
    assert not routed("static_sliding", True, 8192, False, 32768) and routed("static_sliding", True, 8192, False, 4096)   # 8192 rows win only past the window
    assert routed("dynamic", False, 5, True) and routed("static", True, 4096, True) and not routed("dynamic", True, 129, False)   # the full layers' as they were


def test_the_windowed_kernels_use_no_scratch_spill_nothing_and_add_no_lds():
    """The windowed variants are units of their own (the units without a window hold the kernels they held before: test_attn_decode_cpu,
    test_attn_prefill_cpu).  Kernel for kernel: no scratch, no spills, and the LDS of the kernel without a window."""
    from kernel_resources import resources
    for unit, plain, count, name in (("attn_decode_window.hip", "attn_decode.hip", 32, "attn_decode_kernel"),
                                     ("attn_prefill_window.hip", "attn_prefill.hip", 12, "attn_prefill_kernel")):
        res, base = resources(unit), resources(plain)
        assert len(res) == len(base) == count, sorted(res)
        for (n, r), (bn, br) in zip(sorted(res.items()), sorted(base.items())):
            assert name in n and n.replace("Lb1EEE", "Lb0EEE") == bn, (n, bn)                       # the same instantiation but for WIN
            assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
            assert r["group_segment_fixed_size"] == br["group_segment_fixed_size"] > 0, (n, r, br)
