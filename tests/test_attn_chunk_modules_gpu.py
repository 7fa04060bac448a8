"""-m gpu: install_fused_attention(model, prefill="split") on the device, on the tiny llama of tests/decode_loop_cases.py: a prompt, then a
masked chunk of four tokens, then one decode step, on a DynamicCache, a StaticCache and a quant_static_cache.  The logit error against
the float64 model is held to decode_loop_cases' criterion, E(fused) <= M_DEVICE * E(unfused), the unfused run on the same kind of cache."""
import pytest
import torch

import decode_loop_cases as D
from test_attn_decode_cpu import tiny_model

import qllm_amd
from qllm_amd import ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, uninstall_fused_attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 4

_model = {}


def tier_a():
    if not _model:
        model = tiny_model("llama", "sdpa", torch.float16, DEV)
        _model["llama"] = (model, D.float64_copy(model))
    return _model["llama"]


def make_cache(model, kind):
    return qllm_amd.quant_static_cache(model.config, D.MAX_CACHE_LEN, bits=8) if kind == "quant_static" else D.make_cache(model, kind)


def pieces(model, inp, cache, device):
    """The prompt, the chunk, one decode step through `cache`: the logits of the chunk and of the step [B, CHUNK + 1, V] on the CPU."""
    ids, pos, mask = inp.ids.to(device), inp.pos.to(device), None if inp.mask is None else inp.mask.to(device)
    p, out = inp.prompt, []
    with torch.no_grad():
        for a, b in ((0, p), (p, p + CHUNK), (p + CHUNK, p + CHUNK + 1)):
            out.append(model(ids[:, a:b], attention_mask=None if mask is None else mask[:, :b], position_ids=pos[:, a:b], past_key_values=cache,
                             use_cache=True).logits.cpu())
    return torch.cat(out[1:], dim=1)


def count(monkeypatch):
    calls = D.count_calls(monkeypatch)
    calls["rows"] = []
    for name in ("attn_prefill", "attn_chunk"):
        def op(q, *a, _real=getattr(ops, name), _name=name, **kw):
            calls["rows"].append((_name, q.shape[2]))
            return _real(q, *a, **kw)
        monkeypatch.setattr(ops, name, op)
    return calls


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static", "quant_static"])
def test_the_masked_chunk_goes_through_the_op_and_stays_within_the_bound(cache, batch, monkeypatch):
    assert fused_attention.SPLIT_MAX_ROWS >= CHUNK                    # (a bound of zero would leave nothing to test here)
    model, ref = tier_a()
    inp = D.batch_inputs(batch, steps=CHUNK + 1)
    reference = pieces(ref, inp, D.make_cache(ref, "dynamic"), "cpu")
    unfused = pieces(model, inp, make_cache(model, cache), DEV)
    calls = count(monkeypatch)
    got = {}
    for prefill in (True, "split"):
        del calls["rows"][:]
        assert install_fused_attention(model, prefill=prefill) == D.LAYERS
        try:
            got[prefill] = pieces(model, inp, make_cache(model, cache), DEV)
        finally:
            assert uninstall_fused_attention(model) == D.LAYERS
        # the prompt through ops.attn_prefill either way; the chunk through ops.attn_chunk with "split", and with True where it went before:
        # the family's route on a dynamic layer, ops.attn_prefill on the static kinds
        chunk = [("attn_chunk", CHUNK)] if prefill == "split" else [] if cache == "dynamic" else [("attn_prefill", CHUNK)]
        assert calls["rows"] == [("attn_prefill", inp.prompt)] * D.LAYERS + chunk * D.LAYERS, (prefill, calls["rows"])
    assert bool(torch.isfinite(got["split"].float()).all())
    e = {k: (v.double() - reference).abs().max().item() for k, v in (("unfused", unfused), ("true", got[True]), ("split", got["split"]))}
    print(f"chunk modules {cache} {batch}: E(unfused) {e['unfused']:.3e} E(True) {e['true']:.3e} E(split) {e['split']:.3e} ratio {e['split'] / e['unfused']:.3f}")
    assert e["unfused"] > 0 and e["split"] <= D.M_DEVICE * e["unfused"] and e["true"] <= D.M_DEVICE * e["unfused"]
