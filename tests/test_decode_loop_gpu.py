"""-m gpu: the whole decode loop on the device -- prompt, then token after token through a KV cache, the fusions switched on together --
against a float64 copy of the same weights (tests/decode_loop_cases.py has the models, inputs, error and bound).

1. accuracy: E(fused) <= M x E(unfused), both against float64; the kernel-call counts; the prefill's bits.
2. a decode step through a StaticCache makes no host sync (torch's sync debug mode).
3. one captured step of the all-fusions model, replayed for the whole generation, gives the bits of stepping without capture.
4. a cache used again: after reset(), after zeroing the lengths only, after crop() -- over a tail of NaN.
5. generate(): the chosen tokens, judged by the float64 reference.
The figures are printed per case (pytest -s) and recorded in profiles/decode_loop.md."""
import pytest
import torch

import decode_loop_cases as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TIER_A = [("llama", torch.float16), ("mistral", torch.float16), ("qwen2", torch.float16), ("llama", torch.bfloat16)]
TIER_A_IDS = [f"{f}-{str(dt)[6:]}" for f, dt in TIER_A]
DTYPES = [torch.float16, torch.bfloat16]
DTYPE_IDS = ["float16", "bfloat16"]
FLAGS = dict(fuse_mlp=True, fuse_norm=True, fuse_residual=True, fuse_rope=True, fuse_attention=True)


# ---- the models, loaded once ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """(the directory of the saved tier (b) model, the CPU model it was saved from)."""
    from qllm_amd.modeling import base
    qmodel = D.quantized_llama()
    d = str(tmp_path_factory.mktemp("decode_loop") / "ckpt")
    base.save_quantized(qmodel, d)
    return d, qmodel


@pytest.fixture(scope="module")
def tier_b(checkpoint):
    """dtype -> (the plain load, the load with all five fusions, the dense float64 reference)."""
    from qllm_amd.modeling import base
    d, qmodel = checkpoint
    loaded = {}

    def get(dtype):
        if dtype not in loaded:
            kw = {} if dtype == torch.float16 else dict(torch_dtype=torch.bfloat16)
            plain = base.load_quantized(d, device=DEV, **kw)
            fused = base.load_quantized(d, device=DEV, **kw, **FLAGS)
            assert (fused.fused_mlps, fused.fused_norms, fused.fused_residuals, fused.fused_ropes, fused.fused_attentions) == (2, 4, 2, 2, 2)
            assert fused.quant_norms == 1 and not any(hasattr(plain, "fused_" + n) for n in ("mlps", "norms", "residuals", "ropes", "attentions"))
            assert plain.dtype == dtype and fused.dtype == dtype and plain.config.num_key_value_heads == 2
            loaded[dtype] = (plain, fused, D.dense_reference(qmodel, dtype))
        return loaded[dtype]

    return get


_tier_a = {}


def tier_a(family, dtype, attn="sdpa"):
    """(the tiny model on the device, its float64 copy), built once."""
    from test_attn_decode_cpu import tiny_model
    key = (family, dtype, attn)
    if key not in _tier_a:
        model = tiny_model(family, attn, dtype, DEV)
        _tier_a[key] = (model, D.float64_copy(model))
    return _tier_a[key]


_e_unfused = {}


def e_unfused(key, model, ref, inp, cache):
    """E(unfused) of a model on the padded batch, measured once."""
    if key not in _e_unfused:
        _e_unfused[key] = D.error(D.run(model, inp, cache, DEV), D.run(ref, inp))
    return _e_unfused[key]


def fused_tier_a(model):
    from qllm_amd.modeling.q_layers import install_fused_attention, install_fused_rope
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS


def unfused_tier_a(model):
    from qllm_amd.modeling.q_layers import uninstall_fused_attention, uninstall_fused_rope
    assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS


def lengths(cache):
    return [int(layer.cumulative_length) for layer in cache.layers]


# ---- 1. accuracy against float64 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("family,dtype", TIER_A, ids=TIER_A_IDS)
def test_tier_a_decodes_within_the_bound(family, dtype, attn, cache, monkeypatch):
    model, ref = tier_a(family, dtype, attn)
    D.tier_a_case(model, ref, D.batch_inputs("padded"), cache, D.M_DEVICE, monkeypatch, DEV, label=f"{family} {str(dtype)[6:]} {attn} {cache} padded")


@pytest.mark.parametrize("batch", ["padded", "unpadded", "single"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_all_five_fusions_decode_within_the_bound(dtype, cache, batch, tier_b, monkeypatch):
    """E(unfused) is the plain load's.  The prefill is compared with the same load without its attention core: the other four fusions'
    kernels serve the prefill too (their own tests hold them to the plain route), the attention core must not."""
    from qllm_amd.modeling.q_layers import install_fused_attention, uninstall_fused_attention
    plain, fused, ref = tier_b(dtype)
    inp = D.batch_inputs(batch)
    reference, unfused = D.run(ref, inp), D.run(plain, inp, cache, DEV)
    assert uninstall_fused_attention(fused) == D.LAYERS
    try:
        without_core = D.run(fused, inp, cache, DEV, steps=0)
    finally:
        assert install_fused_attention(fused) == D.LAYERS
    calls = D.count_calls(monkeypatch)
    got = D.run(fused, inp, cache, DEV, calls)
    D.assert_case(got, unfused, reference, D.M_DEVICE, calls, prefill=without_core, label=f"five fusions {str(dtype)[6:]} {cache} {batch}")


# ---- 2. no host sync in a static-cache step ----------------------------------------------------------------------------------------------------------
def step_without_sync(model, inp, mask=None):
    """The prefill, then one decode step through a StaticCache under sync debug mode "error": any host sync raises."""
    ids, pos = inp.ids.to(DEV), inp.pos.to(DEV)
    tok, at = ids[:, inp.prompt:inp.prompt + 1].contiguous(), pos[:, inp.prompt:inp.prompt + 1].contiguous()
    cache = D.make_cache(model, "static")
    with torch.no_grad():
        model(ids[:, :inp.prompt], attention_mask=None if mask is None else mask[:, :inp.prompt], position_ids=pos[:, :inp.prompt], past_key_values=cache, use_cache=True)
        torch.cuda.synchronize()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            logits = model(tok, attention_mask=mask, position_ids=at, past_key_values=cache, use_cache=True).logits
        finally:
            torch.cuda.set_sync_debug_mode(before)
    assert lengths(cache) == [inp.prompt + 1] * D.LAYERS and bool(torch.isfinite(logits.float()).all())


def test_the_sync_debug_mode_is_honoured():
    x = torch.ones(4, device=DEV)
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError, match="synchroniz"):
            x.sum().item()
    finally:
        torch.cuda.set_sync_debug_mode(before)


@pytest.mark.parametrize("batch", ["unpadded", "single"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_a_static_cache_step_of_the_five_fusions_makes_no_host_sync(dtype, batch, tier_b):
    step_without_sync(tier_b(dtype)[1], D.batch_inputs(batch))


def test_a_padded_step_behind_a_static_mask_makes_no_host_sync(tier_b):
    """What lets the padded batch into the captured-step test: transformers' own mask code does not sync on a [B, 16] mask either."""
    inp = D.batch_inputs("padded")
    mask = torch.zeros(inp.ids.shape[0], D.MAX_CACHE_LEN, dtype=torch.long)
    mask[:, :inp.prompt + 1] = inp.mask[:, :inp.prompt + 1]
    step_without_sync(tier_b(torch.float16)[1], inp, mask.to(DEV))


def test_a_static_cache_step_of_tier_a_makes_no_host_sync():
    model, _ = tier_a("llama", torch.float16)
    fused_tier_a(model)
    try:
        step_without_sync(model, D.batch_inputs("unpadded"))
    finally:
        unfused_tier_a(model)


# ---- 3. one captured step serves the whole generation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["unpadded", "padded"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_one_captured_step_serves_the_whole_generation(dtype, batch, tier_b):
    """A static token buffer, position ids from the cache's length on the device (position_ids=None) and, for the padded batch, a static
    [B, 16] mask that gains a one per step: the replays launch what stepping launches, with the same arguments -- the same bits.  (The
    padded variant is here because a step with such a mask makes no host sync either: transformers' mask code does not.)"""
    _, fused, _ = tier_b(dtype)
    inp = D.batch_inputs(batch)
    ids, p = inp.ids.to(DEV), inp.prompt
    first = None if inp.mask is None else inp.mask[:, :p].to(DEV)

    def prefill():
        cache = D.make_cache(fused, "static")
        fused(ids[:, :p], attention_mask=first, past_key_values=cache, use_cache=True)
        if first is None:
            return cache, None
        mask = torch.zeros(ids.shape[0], D.MAX_CACHE_LEN, dtype=torch.long, device=DEV)
        mask[:, :p] = first
        return cache, mask

    def feed(tok, mask, i):
        tok.copy_(ids[:, i:i + 1])
        if mask is not None:
            mask[:, i] = 1

    with torch.no_grad():
        cache, mask = prefill()
        tok, want = ids[:, p:p + 1].clone(), []
        for i in range(p, p + inp.steps):
            feed(tok, mask, i)
            want.append(fused(tok, attention_mask=mask, past_key_values=cache, use_cache=True).logits[:, -1].clone())
        assert lengths(cache) == [p + inp.steps] * D.LAYERS
        cache, mask = prefill()
        feed(tok, mask, p)
        graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):                                                              # this stream's workspace exists before the capture
                fused(tok, attention_mask=mask, past_key_values=cache, use_cache=True)
            torch.cuda.synchronize()
            for layer in cache.layers:
                layer.cumulative_length.fill_(p)
            with torch.cuda.graph(graph, stream=side):
                out = fused(tok, attention_mask=mask, past_key_values=cache, use_cache=True).logits
        torch.cuda.current_stream().wait_stream(side)
        got = []
        for i in range(p, p + inp.steps):
            feed(tok, mask, i)
            graph.replay()
            got.append(out[:, -1].clone())
        torch.cuda.synchronize()
    D.assert_same_logits(torch.stack(got).cpu(), torch.stack(want).cpu(), f"captured step {str(dtype)[6:]} {batch}")
    assert lengths(cache) == [p + inp.steps] * D.LAYERS


# ---- 4. a cache used again -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("how", ["reset", "lengths zeroed"])
def test_a_static_cache_serves_a_second_request(how, batch, tier_b):
    """Request A (7 + 6 tokens), then request B (5 + 4) in the same cache.  After B's prefill every position >= 5 -- A's keys where only
    the lengths were zeroed -- is NaN: B's decode steps must not read them and must give the bits of B in a fresh cache."""
    _, fused, _ = tier_b(torch.float16)
    a, b = D.batch_inputs(batch, prompt=7, steps=6, seed=5), D.batch_inputs(batch, prompt=5, steps=4, seed=7)
    fresh = D.run(fused, b, "static", DEV)
    first = D.run(fused, a, "static", DEV)
    assert lengths(first.cache) == [13] * D.LAYERS
    if how == "reset":
        first.cache.reset()
    else:
        for layer in first.cache.layers:
            layer.cumulative_length.zero_()
        assert all(bool(layer.keys[:, :, 5:13].abs().sum() > 0) for layer in first.cache.layers)         # A's keys are still there
    again = D.run(fused, b, first.cache, DEV, poison=True)
    D.assert_same_logits(again.steps, fresh.steps, f"second request, {how}, {batch}")
    assert same_prefill(again, fresh) and lengths(first.cache) == [9] * D.LAYERS


def same_prefill(a, b):
    return D.same_bits(a.prefill, b.prefill)


def test_a_cropped_dynamic_cache_decodes_the_same_tokens_to_the_same_bits(monkeypatch):
    model, _ = tier_a("llama", torch.float16)
    inp = D.batch_inputs("padded", steps=4)
    ids, pos, mask = inp.ids.to(DEV), inp.pos.to(DEV), inp.mask.to(DEV)
    calls = D.count_calls(monkeypatch)
    fused_tier_a(model)
    try:
        first = D.run(model, inp, "dynamic", DEV)
        cache = first.cache
        assert cache.get_seq_length() == 9
        cache.crop(-2)
        assert cache.get_seq_length() == 7
        with torch.no_grad():
            again = torch.stack([model(ids[:, i:i + 1], attention_mask=mask[:, :i + 1], position_ids=pos[:, i:i + 1], past_key_values=cache, use_cache=True).logits[:, -1]
                                 for i in (7, 8)]).cpu()
    finally:
        unfused_tier_a(model)
    assert calls["attn"] == D.LAYERS * 6
    D.assert_same_logits(again, first.steps[2:], "after crop(-2)")


# ---- 5. generate() -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_generate_with_tier_a_chooses_tokens_the_reference_accepts(cache, monkeypatch):
    model, ref = tier_a("llama", torch.float16)
    inp = D.batch_inputs("padded")
    eps = e_unfused(("a", cache), model, ref, inp, cache)
    calls = D.count_calls(monkeypatch)
    fused_tier_a(model)
    try:
        D.assert_generation(model, ref, inp, cache, eps, D.M_DEVICE, calls, DEV, label=f"llama float16 {cache}")
    finally:
        unfused_tier_a(model)


@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("dtype", DTYPES, ids=DTYPE_IDS)
def test_generate_with_all_five_fusions_chooses_tokens_the_reference_accepts(dtype, cache, tier_b, monkeypatch):
    plain, fused, ref = tier_b(dtype)
    inp = D.batch_inputs("padded")
    eps = e_unfused(("b", dtype, cache), plain, ref, inp, cache)
    calls = D.count_calls(monkeypatch)
    D.assert_generation(fused, ref, inp, cache, eps, D.M_DEVICE, calls, DEV, label=f"five fusions {str(dtype)[6:]} {cache}")
