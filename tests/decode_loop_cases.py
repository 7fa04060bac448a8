"""What tests/test_decode_loop_cpu.py and tests/test_decode_loop_gpu.py share: the whole decode loop -- a prompt, then one token after
another through a KV cache -- of a model with the fusions installed, against a float64 copy of the same weights on the CPU.

Models.  Tier (a): test_attn_decode_cpu.tiny_model (hidden 256, 2 layers, 4 heads of 64, 2 kv heads, vocab 64) with install_fused_rope and
install_fused_attention.  Tier (b): `quantized_llama`, the same shape with 4-bit / group-128 GPTQ linears, saved and loaded with all five
fuse_* flags; its reference is a dense LlamaForCausalLM whose linear weights are scales * (codes - zeros) in float64, from the integers.
Every reference runs sdpa: in float64 the eager route adds dtype-min to a negative score, overflows to -inf and returns NaN for the fully
masked query rows of a left-padded batch.

Inputs.  `batch_inputs`: fixed tokens (teacher forcing: every model sees the same prefixes), a 5-token prompt and 8 decode steps, so a
StaticCache of 16 positions is never full (an overfull index_copy_ is a device-side assert).  "padded": three rows left-padded by 0, 2 and
4; "unpadded": two rows and attention_mask=None; "single": one row, where the one-row launches of fuse_mlp / fuse_norm / fuse_residual run.
position_ids = (mask.cumsum(-1) - 1).clamp(min=0) go to every model explicitly.

Error and bound.  E(run) = max over the decode steps and the rows of |last-token logits - reference|.  `assert_case` holds
E(fused) <= M * E(unfused), both against the reference, never against each other; M: profiles/decode_loop.md.  It also holds the call counts
(attention: layers x decode steps, none at the prefill; rope: layers x forwards) and the prefill's bits."""
import copy
from types import SimpleNamespace

import torch

PROMPT, STEPS, MAX_CACHE_LEN = 5, 8, 16
LAYERS, VOCAB = 2, 64
PADS = {"padded": (0, 2, 4), "unpadded": (0, 0), "single": (0,)}
# E(fused) <= M * E(unfused).  Twice the largest ratio measured on the MI355X (1.201: profiles/decode_loop.md), rounded up to one decimal;
# the restated op on the CPU is held to 2.  A dropped key or mask measures 80 and more, so neither figure hides one.
M_DEVICE = 2.5
M_CPU = 2.0


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------------
def batch_inputs(kind="padded", prompt=PROMPT, steps=STEPS, seed=3, vocab=VOCAB):
    """ids [B, prompt + steps], the 0 / 1 mask of the same shape (None where no row is padded), position ids, and the prompt length."""
    pads = PADS[kind]
    seed = 10 * seed + list(PADS).index(kind)                                   # (one seed would give every kind the same first row)
    ids = torch.randint(0, vocab, (len(pads), prompt + steps), generator=torch.Generator().manual_seed(seed))
    mask = torch.ones_like(ids)
    for row, pad in enumerate(pads):
        mask[row, :pad] = 0
    pos = (mask.cumsum(-1) - 1).clamp(min=0)
    return SimpleNamespace(ids=ids, mask=mask if any(pads) else None, pos=pos, prompt=prompt, steps=steps, kind=kind)


def make_cache(model, kind):
    from transformers import DynamicCache, StaticCache
    return DynamicCache(config=model.config) if kind == "dynamic" else StaticCache(config=model.config, max_cache_len=MAX_CACHE_LEN)


def poison_tail(cache, start):
    """NaN in every position >= start of every layer's keys and values: what a kernel that reads past the valid length would meet."""
    for layer in cache.layers:
        layer.keys[:, :, start:] = float("nan")
        layer.values[:, :, start:] = float("nan")


def run(model, inp, cache="dynamic", device="cpu", calls=None, poison=False, steps=None):
    """The prefill of inp's prompt and `steps` (all of inp's by default) single-token decode steps through `cache` ("dynamic", "static" or
    a cache to reuse).  -> prefill logits [B, prompt, V], the decode steps' last-token logits [steps, B, V] (both on the CPU), the cache,
    and what `calls` held right after the prefill.  poison: `poison_tail` behind the prompt, after the prefill -- the family's own
    prefill route reads the whole static cache behind its mask."""
    ids, pos = inp.ids.to(device), inp.pos.to(device)
    mask = None if inp.mask is None else inp.mask.to(device)
    cache = make_cache(model, cache) if isinstance(cache, str) else cache
    steps = inp.steps if steps is None else steps

    def forward(a, b):
        return model(ids[:, a:b], attention_mask=None if mask is None else mask[:, :b], position_ids=pos[:, a:b], past_key_values=cache, use_cache=True).logits

    with torch.no_grad():
        prefill = forward(0, inp.prompt)
        at_prefill = dict(calls) if calls is not None else None
        if poison:
            poison_tail(cache, inp.prompt)
        logits = [forward(i, i + 1)[:, -1] for i in range(inp.prompt, inp.prompt + steps)]
    return SimpleNamespace(prefill=prefill.cpu(), steps=torch.stack(logits).cpu() if logits else None, cache=cache, at_prefill=at_prefill)


# ---- references --------------------------------------------------------------------------------------------------------------------------------
def float64_copy(model, attn="sdpa"):
    """The model's weights in float64 on the CPU, running `attn`.  Take it before anything is installed on the model."""
    ref = copy.deepcopy(model).cpu().double().eval()
    for m in ref.modules():
        if hasattr(m, "config"):
            m.config._attn_implementation = attn
    return ref


def llama_config(dtype="float16"):
    import transformers
    return transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=LAYERS, num_attention_heads=4, num_key_value_heads=2,
                                    vocab_size=VOCAB, max_position_embeddings=64, torch_dtype=dtype, tie_word_embeddings=False)


def quantized_llama():
    """Tier (b) on the CPU, before it is saved: tiny_model's shape (2 kv heads: an attention group of 2) with every decoder linear a 4-bit,
    group-128 GPTQ layer of synthetic integers (test_loader_repack_cpu._quantize_in_place)."""
    import transformers
    from test_loader_repack_cpu import _quantize_in_place
    torch.manual_seed(0)
    model, _ = _quantize_in_place(transformers.LlamaForCausalLM(llama_config()).half(), "GPTQ")
    return model.eval()


def dense_reference(qmodel, dtype=torch.float16):
    """A dense float64 LlamaForCausalLM with the weights a load of `qmodel` in `dtype` computes with: every quantized linear is
    scales * (codes - zeros) from its unpacked integers, in float64 -- not the rounded W of unpack() -- and the scales and every other
    tensor are what the load holds, the checkpoint's fp16 values taken to `dtype`."""
    import transformers
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    cfg = llama_config("float64")
    cfg._attn_implementation = "sdpa"
    ref = transformers.LlamaForCausalLM(cfg).double().eval()
    state = {}
    quantized = {n: m for n, m in qmodel.named_modules() if isinstance(m, QuantLinearGPTQ)}
    for name, layer in quantized.items():
        codes, zeros = layer.unpack_qweight("cpu").double(), layer.unpack_qzeros("cpu").double()          # [K, N], [G, N]
        g = layer.g_idx.long()
        assert codes.min() >= 0 and codes.max() <= 15 and zeros.min() >= 0 and zeros.max() <= 15
        state[name + ".weight"] = (layer.scales.to(dtype).double()[g] * (codes - zeros[g])).T.contiguous()
    for name, t in qmodel.state_dict().items():
        if name.rsplit(".", 1)[0] not in quantized:
            state[name] = t.to(dtype).double()
    ref.load_state_dict(state, strict=True)
    return ref


# ---- counting ----------------------------------------------------------------------------------------------------------------------------------
def count_calls(monkeypatch):
    """Counting wrappers around whatever `ops.attn_decode` and `ops.rope` are now: the kernels on the device, the restatements on the CPU."""
    from qllm_amd import ops
    calls = {"attn": 0, "rope": 0}

    def counted(name, real):
        def op(*a, **kw):
            calls[name] += 1
            return real(*a, **kw)
        return op

    monkeypatch.setattr(ops, "attn_decode", counted("attn", ops.attn_decode))
    monkeypatch.setattr(ops, "rope", counted("rope", ops.rope))
    return calls


# ---- assertions --------------------------------------------------------------------------------------------------------------------------------
def error(got, ref):
    """E(run): the largest |last-token logit - reference| over the decode steps and rows (with left padding every row's last token is real).
    The reference must be free of NaN wherever it is compared."""
    assert got.steps.shape == ref.steps.shape and ref.steps.dtype == torch.float64
    assert bool(torch.isfinite(ref.steps).all()), "the float64 reference is not finite"
    return (got.steps.double() - ref.steps).abs().max().item()


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int16), b.view(torch.int16))


def assert_case(fused, unfused, ref, m, calls=None, forwards=None, prefill=None, label=""):
    """What every accuracy case holds.  fused / unfused / ref: `run` of the model under test, of the same weights without the fusions and
    of the float64 reference, on the same inputs.  calls: `count_calls` as it stands after the fused run (which took its own snapshot
    after the prefill), the counts starting at zero before it.  prefill: the run whose prefill logits the fused run's must equal bit
    for bit (the unfused one unless given).  -> (E(unfused), E(fused))."""
    steps = fused.steps.shape[0]
    assert bool(torch.isfinite(fused.steps.float()).all()), f"{label}: the fused logits are not finite"
    assert bool(torch.isfinite(unfused.steps.float()).all()), f"{label}: the unfused logits are not finite"
    e_unfused, e_fused = error(unfused, ref), error(fused, ref)
    print(f"decode loop {label}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    if calls is not None:
        forwards = steps + 1 if forwards is None else forwards
        assert fused.at_prefill["attn"] == 0, f"{label}: {fused.at_prefill['attn']} attention kernel calls at the prefill"
        assert calls["attn"] == LAYERS * steps, f"{label}: {calls['attn']} attention kernel calls, expected {LAYERS * steps}"
        assert calls["rope"] == LAYERS * forwards, f"{label}: {calls['rope']} rope kernel calls, expected {LAYERS * forwards}"
    want = (unfused if prefill is None else prefill).prefill
    assert same_bits(fused.prefill, want), f"{label}: the prefill logits differ from the unfused model's"
    assert e_unfused > 0 and e_fused <= m * e_unfused, f"{label}: bound: E(fused) {e_fused:.3e} > {m} x E(unfused) {e_unfused:.3e}"
    return e_unfused, e_fused


def assert_same_logits(got, want, label=""):
    """The decode logits of `got` are free of NaN and the very bits of `want`'s."""
    assert bool(torch.isfinite(got.float()).all()), f"{label}: the logits are not finite"
    assert same_bits(got, want), f"{label}: the logits differ: max {(got.double() - want.double()).abs().max().item():.3e}"


def tier_a_case(model, ref, inp, cache, m, monkeypatch, device="cpu", poison=False, label=""):
    """One tier (a) case: the unfused run, install_fused_rope + install_fused_attention, the fused run, uninstall, `assert_case`.
    `monkeypatch` must hold whatever replaces the ops already (the CPU file's restatements); the counting goes on top."""
    from qllm_amd.modeling.q_layers import install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope
    reference = run(ref, inp)
    unfused = run(model, inp, cache, device)
    calls = count_calls(monkeypatch)
    assert install_fused_rope(model) == LAYERS and install_fused_attention(model) == LAYERS
    try:
        fused = run(model, inp, cache, device, calls, poison=poison)
    finally:
        assert uninstall_fused_attention(model) == LAYERS and uninstall_fused_rope(model) == LAYERS
    return assert_case(fused, unfused, reference, m, calls, label=label)


def generated_shortfall(ref, sequences, mask, prompt):
    """The generated sequences [B, prompt + new] through the float64 reference in one forward.  -> [B, new] float64: at every generated
    position, how far the reference's logit of the chosen token lies below the reference's maximum."""
    full = torch.ones_like(sequences) if mask is None else torch.cat((mask[:, :prompt], torch.ones_like(sequences[:, prompt:])), 1)
    pos = (full.cumsum(-1) - 1).clamp(min=0)
    with torch.no_grad():
        logits = ref(sequences, attention_mask=None if mask is None else full, position_ids=pos).logits[:, prompt - 1:-1]
    assert logits.dtype == torch.float64 and bool(torch.isfinite(logits).all()), "the float64 reference is not finite"
    return logits.max(-1).values - logits.gather(-1, sequences[:, prompt:, None]).squeeze(-1)


def assert_generation(model, ref, inp, cache, e_unfused, m, calls, device="cpu", label=""):
    """Greedy `generate()` of inp's prompt: steps new tokens, no stop token.  A token chosen from logits within eps of the truth cannot
    fall short of the true maximum by more than 2 eps: with eps = m * E(unfused), at every generated position."""
    new = inp.steps
    kw = dict(past_key_values=make_cache(model, "static"), disable_compile=True) if cache == "static" else {}
    mask = None if inp.mask is None else inp.mask[:, :inp.prompt].to(device)
    before = dict(calls)
    out = model.generate(input_ids=inp.ids[:, :inp.prompt].to(device), attention_mask=mask, max_new_tokens=new, do_sample=False, eos_token_id=None,
                         pad_token_id=0, **kw).cpu()
    assert out.shape == (inp.ids.shape[0], inp.prompt + new) and torch.equal(out[:, :inp.prompt], inp.ids[:, :inp.prompt])
    assert calls["attn"] - before["attn"] == LAYERS * (new - 1), f"{label}: {calls['attn'] - before['attn']} attention kernel calls"
    short = generated_shortfall(ref, out, inp.mask, inp.prompt)
    print(f"generate {label}: largest shortfall {short.max().item():.3e}, allowed {2 * m * e_unfused:.3e}")
    assert short.max().item() <= 2 * m * e_unfused, f"{label}: shortfall {short.max().item():.3e} > 2 x {m} x {e_unfused:.3e}"
    return out
