"""No GPU: qllm_attn_prefill_quant as far as a host reaches -- symbols, the plan's refusals, the built kernels' resources -- and the host
routing of install_fused_attention(model, prefill="codes_all") on the tiny llama over a quant_static_cache, torch restatements as ops."""
import os

import pytest
import torch

import attn_prefill_cases as AP
import decode_loop_cases as D
from kernel_resources import resources
from test_attn_chunk_quant_cpu import ROOT, restatements, tensors
from test_attn_decode_cpu import tiny_model
from transformers import StaticCache

import qllm_amd
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, uninstall_fused_attention
from qllm_amd.modeling.quant_cache import dequantize_rows

PROMPT, CHUNK, CACHE = 20, 18, 48               # both pieces above SPLIT_MAX_ROWS: neither is the chunk route's


def test_symbols_are_declared_and_exported_within_abi_7():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    for name in ("qllm_attn_prefill_quant", "qllm_attn_prefill_quant_describe"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert all(n in ops.__all__ for n in ("attn_prefill_quant", "attn_prefill_quant_plan", "attn_prefill_quant_describe"))
    assert ops.attn_prefill_quant_describe(2, 7, 1, 64, 4, 19, 200) == "attn_prefill_quant bits=4 tile=64 grid=2x1x2 group=7"
    assert "8- and 4-bit" in ops.attn_prefill_quant_describe(1, 8, 1, 64, 3, 4, 64) and "1..8 query heads" in ops.attn_prefill_quant_describe(1, 9, 1, 64, 8, 4, 64)


@pytest.mark.parametrize("how,why", [
    (dict(s=1), "at least two rows"), (dict(hq=9, hk=1), "at most 8 query heads per kv head"), (dict(d=96), "head_dim 64 or 128"),
    (dict(bits=3), "bits must be 8 or 4"), (dict(dtype=torch.float32), "float16 or bfloat16"),
    (dict(mask=torch.ones(1, 1, 4, 199, dtype=torch.bool)), "the mask must cover 200 positions"),
    (dict(change=lambda t: t[:2] + (t[2][..., :1],) + t[3:]), r"params \[B, Hkv, L, 2\]")])
def test_the_plan_refuses_before_any_launch(how, why):
    how = dict(how)
    change, mask, bits = how.pop("change", lambda t: t), how.pop("mask", None), how.get("bits", 8)
    q, *cache = change(tensors(**dict(how, bits=8 if bits == 3 else bits)))
    for call in (ops.attn_prefill_quant_plan, ops.attn_prefill_quant):        # the op refuses through its plan: CPU tensors never reach a launch
        with pytest.raises(ops.QllmUnsupported, match=why):
            call(q, *cache, bits, 200, mask)
    q, *cache = tensors(hq=8, hk=1, s=40)                                       # 320 rows per kv head: no bound on them here
    assert ops.attn_prefill_quant_plan(q, *cache, 8, 200)[:7] == (1, 8, 1, 64, 8, 40, 300)


def test_every_instantiation_is_built_without_scratch_or_spills():
    kernels = {name: r for name, r in resources("attn_prefill_quant.hip").items() if "attn_prefill_quant_kernel" in name}
    assert len(kernels) == 24, sorted(kernels)                                 # 2 types x 2 head sizes x 2 widths x 3 mask kinds
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)


def run(model, prefill, inp, cache, calls):   # the prompt, then a chunk behind it: the chunk's logits and the calls the restated ops saw
    del calls[:]
    assert install_fused_attention(model, prefill=prefill) == D.LAYERS
    assert fused_attention.count_fused_attention_prefill(model) == D.LAYERS
    try:
        with torch.no_grad():
            for a, b in ((0, PROMPT), (PROMPT, PROMPT + CHUNK)):
                out = model(inp.ids[:, a:b], attention_mask=None if inp.mask is None else inp.mask[:, :b], position_ids=inp.pos[:, a:b],
                            past_key_values=cache, use_cache=True).logits
        return out, list(calls)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS


@pytest.mark.parametrize("batch", ("padded", "unpadded"))
@pytest.mark.parametrize("bits", (8, 4))
def test_codes_all_routes_prompt_and_chunk_to_the_new_op_only_under_its_conditions(bits, batch, monkeypatch):
    model = tiny_model("llama", "sdpa", torch.float16, "cpu")
    inp = D.batch_inputs(batch, prompt=PROMPT, steps=CHUNK)
    quant = lambda n=CACHE: qllm_amd.quant_static_cache(model.config, n, bits=bits)
    calls = restatements(monkeypatch)

    def attn_prefill_quant(q, kc, kp, vc, vp, bits, length, **kw):
        calls.append(("all", q.shape[2], int(length), isinstance(length, torch.Tensor), kw.get("mask") is not None))
        return AP.restated(q, dequantize_rows(kc, kp, bits), dequantize_rows(vc, vp, bits), length, **kw)
    monkeypatch.setattr(ops, "attn_prefill_quant", attn_prefill_quant)
    codes, codes_calls = run(model, "codes", inp, quant(), calls)
    got, got_calls = run(model, "codes_all", inp, quant(), calls)
    # the prompt on the layer it initialises (no mask where no row is padded), then the chunk (always masked), the length from the device counter
    want = [[("all", PROMPT, PROMPT, True, batch == "padded")], [("all", CHUNK, PROMPT + CHUNK, True, True)]]
    assert got_calls == want[0] * D.LAYERS + want[1] * D.LAYERS and not codes_calls
    assert D.same_bits(got, codes)                                             # the same dequantised values either way
    # a refused plan, a non-quantized cache and a cache without room (`update` raises as under "codes") each end where "codes" ends
    def refuse(*a, **kw):
        raise ops.QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "refused here")
    with monkeypatch.context() as m:
        m.setattr(ops, "attn_prefill_quant_plan", refuse)
        again, again_calls = run(model, "codes_all", inp, quant(), calls)
    assert again_calls == codes_calls and D.same_bits(again, codes)
    plain = lambda: StaticCache(config=model.config, max_cache_len=CACHE)
    other, other_calls = run(model, "codes_all", inp, plain(), calls)
    assert other_calls == [] and D.same_bits(other, run(model, "codes", inp, plain(), calls)[0])
    with pytest.raises(ValueError, match="do not fit"):
        run(model, "codes_all", inp, quant(PROMPT + CHUNK - 1), calls)
    assert [c[:2] for c in calls] == [("all", PROMPT)] * D.LAYERS               # the prompt fitted; the chunk did not and was left to `update`


def test_the_option_value_installs_its_core_and_the_others_keep_theirs():
    model = tiny_model("llama", "sdpa", torch.float16, "cpu")
    for value, core in (("codes_all", fused_attention._fused_core_codes_all), ("codes", fused_attention._fused_core_codes)):
        assert install_fused_attention(model, prefill=value) == D.LAYERS
        assert {mod.__dict__[fused_attention._CORE][3] for mod in model.modules() if fused_attention._CORE in mod.__dict__} == {core}
        assert uninstall_fused_attention(model) == D.LAYERS
    for bad in ("codes_al", "all", ("codes_all",)):
        with pytest.raises(ValueError, match="codes_all"):
            install_fused_attention(model, prefill=bad)
