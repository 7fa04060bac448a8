"""-m gpu: the modules of q_layers/fused_attention.py with the prefill core on the device (install_fused_attention(model, prefill=True),
load_quantized(..., fuse_attention_prefill=True)), on the harness of tests/decode_loop_cases.py and tests/test_attn_decode_cpu.py.

E(run) here is the largest |logit - float64 reference| over the PROMPT's real positions (a left-padded row's pad positions attend to
nothing and are compared nowhere).  Every accuracy case holds E(fused) <= M_PREFILL * E(unfused), both against float64, never against
each other; M_PREFILL and the ratios of one run: profiles/attn_prefill.md."""
import pytest
import torch

import decode_loop_cases as D
from test_attn_decode_cpu import FAMILIES, tiny_model

from qllm_amd import ops
from qllm_amd.modeling.q_layers import install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# E(fused) <= M_PREFILL * E(unfused): twice the largest ratio measured (profiles/attn_prefill.md, "Modules"), rounded up to one decimal; the
# harness's own ceiling is 4
M_PREFILL = 2.7
FLAGS = dict(fuse_mlp=True, fuse_norm=True, fuse_residual=True, fuse_rope=True, fuse_attention=True, fuse_attention_prefill=True)

_models = {}


def tier_a(family, attn):
    key = (family, attn)
    if key not in _models:
        model = tiny_model(family, attn, torch.float16, DEV)
        _models[key] = (model, D.float64_copy(model))
    return _models[key]


def count(monkeypatch):
    calls = D.count_calls(monkeypatch)
    calls.update(prefill=0, shapes=[])
    real = ops.attn_prefill

    def attn_prefill(q, *a, **kw):
        calls["prefill"] += 1
        calls["shapes"].append(q.shape[2])
        return real(q, *a, **kw)

    monkeypatch.setattr(ops, "attn_prefill", attn_prefill)
    return calls


def prompt_error(got, ref, inp):
    real = torch.ones_like(inp.ids[:, :inp.prompt], dtype=torch.bool) if inp.mask is None else inp.mask[:, :inp.prompt].bool()
    assert bool(torch.isfinite(ref.prefill[real]).all()) and bool(torch.isfinite(got.prefill[real].float()).all())
    return (got.prefill.double() - ref.prefill)[real].abs().max().item()


def held(fused, unfused, ref, inp, label):
    e_unfused, e_fused = prompt_error(unfused, ref, inp), prompt_error(fused, ref, inp)
    print(f"prefill {label}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    assert M_PREFILL <= 4.0 and e_unfused > 0 and e_fused <= M_PREFILL * e_unfused, (label, e_fused, e_unfused)


# ---- 1. the prompt of the tiny models -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("family", FAMILIES)
def test_the_prompt_of_the_tiny_models_is_within_the_bound(family, attn, cache, batch, monkeypatch):
    model, ref = tier_a(family, attn)
    inp = D.batch_inputs(batch)
    reference, unfused = D.run(ref, inp, steps=2), D.run(model, inp, cache, DEV, steps=2)
    calls = count(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused = D.run(model, inp, cache, DEV, calls, steps=2)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    assert fused.at_prefill["prefill"] == D.LAYERS and fused.at_prefill["attn"] == 0 and calls["shapes"] == [inp.prompt] * D.LAYERS   # one call per layer at the prompt
    assert calls["prefill"] == D.LAYERS and calls["attn"] == 2 * D.LAYERS                                                            # and none at the decode steps
    held(fused, unfused, reference, inp, f"{family} {attn} {cache} {batch}")
    assert D.error(fused, reference) <= M_PREFILL * D.error(unfused, reference)                # the decode steps behind the fused prompt


# ---- 2. the quantized model with every fusion ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tier_b(tmp_path_factory):
    from qllm_amd.modeling import base
    qmodel = D.quantized_llama()
    d = str(tmp_path_factory.mktemp("attn_prefill") / "ckpt")
    base.save_quantized(qmodel, d)
    plain = base.load_quantized(d, device=DEV)
    fused = base.load_quantized(d, device=DEV, **FLAGS)
    assert (fused.fused_attentions, fused.fused_attention_prefills, fused.fused_ropes) == (2, 2, 2) and not hasattr(plain, "fused_attention_prefills")
    only = base.load_quantized(d, device=DEV, fuse_attention_prefill=True)                     # the flag implies the attention install
    assert (only.fused_attentions, only.fused_attention_prefills) == (2, 2)
    return plain, fused, D.dense_reference(qmodel, torch.float16)


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_all_fusions_with_the_prefill_core_stay_within_the_bound(cache, batch, tier_b, monkeypatch):
    plain, fused, ref = tier_b
    inp = D.batch_inputs(batch)
    reference, unfused = D.run(ref, inp), D.run(plain, inp, cache, DEV)
    calls = count(monkeypatch)
    got = D.run(fused, inp, cache, DEV, calls)
    assert got.at_prefill["prefill"] == D.LAYERS and calls["prefill"] == D.LAYERS and calls["attn"] == D.LAYERS * inp.steps
    held(got, unfused, reference, inp, f"all fusions {cache} {batch}")
    e_unfused, e_fused = D.error(unfused, reference), D.error(got, reference)
    print(f"decode behind the fused prompt {cache} {batch}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    assert e_fused <= M_PREFILL * e_unfused


# ---- 3. a second chunk behind cached tokens -----------------------------------------------------------------------------------------------------
def chunked(model, inp, cache, device):
    """The prompt, then a chunk of 3 tokens in one forward: the chunk's logits [B, 3, V] on the CPU."""
    ids, pos = inp.ids.to(device), inp.pos.to(device)
    mask = None if inp.mask is None else inp.mask.to(device)
    cache = D.make_cache(model, cache)
    p = inp.prompt
    with torch.no_grad():
        model(ids[:, :p], attention_mask=None if mask is None else mask[:, :p], position_ids=pos[:, :p], past_key_values=cache, use_cache=True)
        return model(ids[:, p:p + 3], attention_mask=None if mask is None else mask[:, :p + 3], position_ids=pos[:, p:p + 3], past_key_values=cache,
                     use_cache=True).logits.cpu()


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
def test_a_chunk_of_three_behind_five_cached_tokens(attn, cache, batch, monkeypatch):
    model, ref = tier_a("llama", attn)
    inp = D.batch_inputs(batch)
    reference, unfused = chunked(ref, inp, "dynamic", "cpu"), chunked(model, inp, cache, DEV)
    calls = count(monkeypatch)
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused = chunked(model, inp, cache, DEV)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    # the chunk always carries a mask: served on a static layer; PREFILL_ROUTES keeps masked chunks on a dynamic layer on the family's route
    assert calls["shapes"] == [5] * D.LAYERS + ([3] * D.LAYERS if cache == "static" else []) and calls["attn"] == 0
    e_unfused, e_fused = (unfused.double() - reference).abs().max().item(), (fused.double() - reference).abs().max().item()
    print(f"chunk {attn} {cache} {batch}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    assert bool(torch.isfinite(fused.float()).all()) and e_unfused > 0 and e_fused <= M_PREFILL * e_unfused


# ---- 4. flag off ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_with_the_flag_off_the_prompt_is_the_family_route(cache, monkeypatch):
    model, _ = tier_a("llama", "sdpa")
    inp = D.batch_inputs("padded")
    unfused = D.run(model, inp, cache, DEV, steps=1)
    calls = count(monkeypatch)
    assert install_fused_attention(model) == D.LAYERS
    try:
        fused = D.run(model, inp, cache, DEV, calls, steps=1)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert calls["prefill"] == 0 and calls["attn"] == D.LAYERS and D.same_bits(fused.prefill, unfused.prefill)


# ---- 5. a static cache used again over NaN ------------------------------------------------------------------------------------------------------
def test_a_static_cache_used_again_over_a_tail_of_nan(monkeypatch):
    """Request A, reset(), NaN in EVERY position, then request B's padded prompt: `update` writes B's 5 rows, the kernel reads those and
    nothing behind them -- the bits of B in a fresh cache."""
    model, _ = tier_a("llama", "sdpa")
    a, b = D.batch_inputs("padded", prompt=7, steps=2, seed=5), D.batch_inputs("padded", prompt=5, steps=2, seed=7)
    calls = count(monkeypatch)
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fresh = D.run(model, b, "static", DEV)
        first = D.run(model, a, "static", DEV)
        first.cache.reset()
        D.poison_tail(first.cache, 0)
        again = D.run(model, b, first.cache, DEV)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert calls["prefill"] == 3 * D.LAYERS
    real = b.mask[:, :b.prompt].bool()
    assert bool(torch.isfinite(again.prefill[real].float()).all()) and torch.equal(again.prefill[real].view(torch.int16), fresh.prefill[real].view(torch.int16))
    D.assert_same_logits(again.steps, fresh.steps, "second request over NaN")


# ---- 6. the documented limit --------------------------------------------------------------------------------------------------------------------------
def test_a_hand_made_mask_that_shows_a_future_key_gives_mask_and_causal(monkeypatch):
    """The kernel runs with causal = 1 plus the mask.  A 4-D mask that shows row 1 the key at position 3 is honoured by the family's route
    and NOT by the prefill core, whose result is that of (mask AND causal)."""
    from transformers import DynamicCache
    model, _ = tier_a("llama", "sdpa")
    ids = D.batch_inputs("unpadded").ids[:, :5].to(DEV)
    causal = torch.ones(5, 5, dtype=torch.bool).tril()[None, None].expand(2, 1, 5, 5).contiguous().to(DEV)
    future = causal.clone()
    future[:, :, 1, 3] = True

    def logits(mask):
        with torch.no_grad():
            return model(ids, attention_mask=mask, past_key_values=DynamicCache(config=model.config), use_cache=True).logits.cpu()

    family_causal, family_future = logits(causal), logits(future)
    assert not torch.equal(family_causal[:, 1], family_future[:, 1]) and torch.equal(family_causal[:, 0], family_future[:, 0])   # the family's route honours it
    calls = count(monkeypatch)
    assert install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused_causal, fused_future = logits(causal), logits(future)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert calls["prefill"] == 2 * D.LAYERS and D.same_bits(fused_future, fused_causal)
    assert (fused_causal.double() - family_causal.double()).abs().max() <= 2e-2                     # and (mask AND causal) is the causal model
