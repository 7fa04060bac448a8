"""No GPU: the harness of tests/decode_loop_cases.py with the torch restatements of the attention and rope ops (test_attn_decode_cpu.fake_op,
test_rope_cpu.fake_op) in the kernels' place -- every tier (a) case within M = 2 of the unfused model's own error against float64 -- and
the proof that the harness's assertions fail when the op drops the newest key, drops the mask, or reads the whole of a static cache whose
tail is poisoned.  The figures are printed per case (pytest -s) and recorded in profiles/decode_loop.md."""
import pytest
import torch

import decode_loop_cases as D
from attn_decode_cases import restated
from test_attn_decode_cpu import fake_op, tiny_model
from test_rope_cpu import fake_op as fake_rope

from qllm_amd.modeling.q_layers import fused_attention

MODELS = [("llama", torch.float16), ("mistral", torch.float16), ("qwen2", torch.float16), ("llama", torch.bfloat16)]
MODEL_IDS = [f"{f}-{str(dt)[6:]}" for f, dt in MODELS]


def restatements(monkeypatch):
    return fake_op(monkeypatch), fake_rope(monkeypatch)


@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("family,dtype", MODELS, ids=MODEL_IDS)
def test_tier_a_decodes_within_twice_the_unfused_error(family, dtype, attn, cache, monkeypatch):
    model = tiny_model(family, attn, dtype)
    ref = D.float64_copy(model)
    restatements(monkeypatch)
    D.tier_a_case(model, ref, D.batch_inputs("padded"), cache, D.M_CPU, monkeypatch, label=f"cpu {family} {str(dtype)[6:]} {attn} {cache} padded")


def test_tier_a_unpadded_batch_without_a_mask(monkeypatch):
    model = tiny_model("llama", "sdpa")
    ref = D.float64_copy(model)
    restatements(monkeypatch)
    for cache in ("dynamic", "static"):
        D.tier_a_case(model, ref, D.batch_inputs("unpadded"), cache, D.M_CPU, monkeypatch, label=f"cpu llama float16 sdpa {cache} unpadded")


# ---- the assertions can fail ---------------------------------------------------------------------------------------------------------------------
def broken(monkeypatch, how):
    """The restated op with one defect, in the place `fake_op` put the sound one."""
    def attn_decode(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None, *, out=None, plan=None):
        n = int(length)
        if how == "newest key":
            n -= 1
        elif how == "mask":
            mask = None
        elif how == "tail":
            n = k_cache.shape[2]
        return restated(q, k_cache, v_cache, n, k_new, v_new, mask, scaling)

    monkeypatch.setattr(fused_attention.ops, "attn_decode", attn_decode)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])
@pytest.mark.parametrize("how", ["newest key", "mask"])
def test_a_dropped_key_or_mask_breaks_the_bound(how, dtype, monkeypatch):
    """With M = 4, the most any case may ever be given."""
    model = tiny_model("llama", "sdpa", dtype)
    ref = D.float64_copy(model)
    restatements(monkeypatch)
    broken(monkeypatch, how)
    for cache in ("dynamic", "static"):
        with pytest.raises(AssertionError, match="bound: E"):
            D.tier_a_case(model, ref, D.batch_inputs("padded"), cache, 4.0, monkeypatch, label=f"{how} {cache}")


def test_reading_a_static_cache_to_its_end_is_hidden_by_the_mask_and_shown_by_a_poisoned_tail(monkeypatch):
    model = tiny_model("llama", "sdpa")
    ref = D.float64_copy(model)
    restatements(monkeypatch)
    broken(monkeypatch, "tail")
    inp = D.batch_inputs("padded")
    D.tier_a_case(model, ref, inp, "static", D.M_CPU, monkeypatch, label="tail, clean")           # the mask hides the zeros behind the length
    with pytest.raises(AssertionError, match="not finite"):
        D.tier_a_case(model, ref, inp, "static", D.M_CPU, monkeypatch, poison=True, label="tail, poisoned")
    with pytest.raises(AssertionError, match="not finite"):                                          # the assertion of the cache-reuse tests
        fresh = D.run(model, inp, "static")
        from qllm_amd.modeling.q_layers import install_fused_attention, uninstall_fused_attention
        assert install_fused_attention(model) == D.LAYERS
        try:
            got = D.run(model, inp, "static", poison=True)
        finally:
            uninstall_fused_attention(model)
        D.assert_same_logits(got.steps, fresh.steps, "tail, poisoned")


def test_the_sound_op_passes_over_a_poisoned_tail(monkeypatch):
    model = tiny_model("llama", "sdpa")
    ref = D.float64_copy(model)
    restatements(monkeypatch)
    D.tier_a_case(model, ref, D.batch_inputs("padded"), "static", D.M_CPU, monkeypatch, poison=True, label="cpu llama float16 sdpa static padded, poisoned tail")


def test_a_wrong_call_count_or_prefill_is_caught(monkeypatch):
    model = tiny_model("llama", "sdpa")
    inp = D.batch_inputs("padded")
    reference, unfused = D.run(D.float64_copy(model), inp), D.run(model, inp)
    calls = {"attn": D.LAYERS * inp.steps, "rope": D.LAYERS * (inp.steps + 1)}
    unfused.at_prefill = {"attn": 0, "rope": D.LAYERS}
    D.assert_case(unfused, unfused, reference, 1.0, calls)
    with pytest.raises(AssertionError, match="attention kernel calls, expected"):
        D.assert_case(unfused, unfused, reference, 1.0, dict(calls, attn=calls["attn"] - 1))
    with pytest.raises(AssertionError, match="rope kernel calls"):
        D.assert_case(unfused, unfused, reference, 1.0, dict(calls, rope=calls["rope"] + D.LAYERS))
    unfused.at_prefill = {"attn": D.LAYERS, "rope": D.LAYERS}
    with pytest.raises(AssertionError, match="at the prefill"):
        D.assert_case(unfused, unfused, reference, 1.0, calls)
    unfused.at_prefill = {"attn": 0, "rope": D.LAYERS}
    other = D.run(model, inp)
    other.prefill[0, 0, 0] += 2 ** -10
    with pytest.raises(AssertionError, match="prefill logits differ"):
        D.assert_case(unfused, unfused, reference, 1.0, calls, prefill=other)


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def test_the_float64_reference_needs_sdpa_on_a_left_padded_batch():
    """eager in float64: the mask's dtype-min plus a negative score overflows to -inf, a fully masked query row is all -inf, its softmax
    NaN; the NaN reaches the later layers' keys and from there every row that holds padding."""
    model = tiny_model("llama", "eager")
    inp = D.batch_inputs("padded")
    good = D.run(D.float64_copy(model, "sdpa"), inp)
    assert bool(torch.isfinite(good.steps).all()) and bool(torch.isfinite(good.prefill[0]).all())
    bad = D.run(D.float64_copy(model, "eager"), inp)
    assert not bool(torch.isfinite(bad.steps).all())
    plain = D.batch_inputs("unpadded")                  # without padding the two routes agree as far as eager's fp32 softmax lets them
    a, b = D.run(D.float64_copy(model, "sdpa"), plain), D.run(D.float64_copy(model, "eager"), plain)
    assert (a.steps - b.steps).abs().max().item() < 1e-6


def test_the_dense_reference_holds_the_integers_times_the_scales():
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    qmodel = D.quantized_llama()
    layer = qmodel.model.layers[1].self_attn.k_proj
    assert isinstance(layer, QuantLinearGPTQ) and (layer.infeatures, layer.outfeatures) == (256, 128)      # 2 kv heads of 64
    for dtype in (torch.float16, torch.bfloat16):
        ref = D.dense_reference(qmodel, dtype)
        w = ref.model.layers[1].self_attn.k_proj.weight
        assert w.dtype == torch.float64 and w.shape == (128, 256)
        rounded = layer.unpack()[0].double()                                                                # W [N, K], rounded to fp16 per operation
        # q * s, z * s and their difference are each rounded to fp16 below 0.125: three half ulps of 2^-14; a bf16 scale below 2^-7 moves by
        # at most half of 2^-15, under codes - zeros of at most 15
        assert 0 < (w.detach() - rounded).abs().max().item() <= 1.5 * 2.0 ** -14 + (0 if dtype == torch.float16 else 15 * 2.0 ** -16)
        assert torch.equal(ref.lm_head.weight, qmodel.lm_head.weight.to(dtype).double())
    out = D.run(D.dense_reference(qmodel), D.batch_inputs("padded"))
    assert bool(torch.isfinite(out.steps).all()) and out.steps.abs().max().item() < 8


def test_a_float16_checkpoint_loads_in_the_type_asked_for(tmp_path):
    """load_quantized(torch_dtype=torch.bfloat16) of a checkpoint whose config says float16: every floating tensor is bfloat16 -- the
    checkpoint's values rounded once -- and the default load stays float16.  (It used to come back in float16 without a word, so the
    bf16 cases of the device file would have measured fp16 twice.)"""
    from qllm_amd.modeling import base
    qmodel = D.quantized_llama()
    d = str(tmp_path / "ckpt")
    base.save_quantized(qmodel, d)
    want = qmodel.state_dict()
    for dtype, kw in ((torch.float16, {}), (torch.bfloat16, dict(torch_dtype=torch.bfloat16))):
        loaded = base.load_quantized(d, device=None, **kw)
        assert loaded.dtype == dtype and loaded.model.layers[0].self_attn.q_proj.dtype == dtype
        state = loaded.state_dict()
        assert set(state) == set(want)
        for name, t in state.items():
            assert t.dtype == (dtype if want[name].is_floating_point() else want[name].dtype), name
            assert torch.equal(t, want[name].to(t.dtype)), name


def test_generation_is_judged_by_the_reference(monkeypatch):
    """`assert_generation` on the CPU with the restated op: the shortfall of the chosen tokens stays inside 2 M E(unfused) with both caches,
    and a sequence with one token replaced falls outside."""
    from qllm_amd.modeling.q_layers import install_fused_attention, install_fused_rope
    model = tiny_model("llama", "sdpa")
    ref = D.float64_copy(model)
    inp = D.batch_inputs("padded")
    e_unfused = D.error(D.run(model, inp), D.run(ref, inp))
    restatements(monkeypatch)
    calls = D.count_calls(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS
    for cache in ("dynamic", "static"):
        out = D.assert_generation(model, ref, inp, cache, e_unfused, D.M_CPU, calls, label=f"cpu llama {cache}")
    worst = D.generated_shortfall(ref, out, inp.mask, inp.prompt)
    with torch.no_grad():
        logits = ref(out, attention_mask=torch.cat((inp.mask[:, :inp.prompt], torch.ones_like(out[:, inp.prompt:])), 1)).logits
    out[1, inp.prompt + 3] = logits[1, inp.prompt + 2].argmin()
    assert D.generated_shortfall(ref, out, inp.mask, inp.prompt)[1, 3].item() > 100 * max(worst.max().item(), 2 * D.M_CPU * e_unfused)
