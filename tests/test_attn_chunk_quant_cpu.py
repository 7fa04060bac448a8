"""No GPU: qllm_attn_chunk_quant as far as a host reaches -- symbols, the plan's refusals and tuples, the built kernels' resources -- and the
host routing of install_fused_attention(model, prefill="codes") on the tiny llama over a quant_static_cache, torch restatements as ops."""
import os

import pytest
import torch

import attn_prefill_cases as AP
import attn_sliding_cases as S
import decode_loop_cases as D
from kernel_resources import resources
from test_attn_decode_cpu import tiny_model
from test_rope_cpu import fake_op as fake_rope

import qllm_amd
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, uninstall_fused_attention
from qllm_amd.modeling.quant_cache import dequantize_rows, quantize_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tensors(b=1, hq=8, hk=2, d=64, s=4, L=300, bits=8, dtype=torch.float16):
    """q and the four cache tensors (k_codes, k_params, v_codes, v_params)."""
    nbytes, nparams = ops.kv_quant_shapes(d, bits)
    return (torch.zeros(b, hq, s, d, dtype=dtype),) + tuple(torch.zeros(b, hk, L, n, dtype=t) for n, t in ((nbytes, torch.uint8), (nparams, dtype))) * 2


def test_symbols_are_declared_and_exported_within_abi_7():
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    for name in ("qllm_attn_chunk_quant", "qllm_attn_chunk_quant_describe"):
        assert name in _lib.EXPORTS and hasattr(lib, name) and f"int {name}(" in header
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert all(n in ops.__all__ for n in ("attn_chunk_quant", "attn_chunk_quant_plan", "attn_chunk_quant_describe"))
    assert ops.attn_chunk_quant_describe(1, 8, 1, 64, 3, 4, 64).startswith("refused: ") and "8- and 4-bit" in ops.attn_chunk_quant_describe(1, 8, 1, 64, 3, 4, 64)


def misaligned(t):
    """The same tensor two bytes further on in memory."""
    return torch.zeros(t.numel() + 1, dtype=t.dtype)[1:].view(t.shape)


@pytest.mark.parametrize("how,why", [
    (dict(bits=3), "bits must be 8 or 4"), (dict(d=96), "head_dim 64 or 128"), (dict(hq=3, hk=1, s=43), "128 query rows"),
    (dict(change=lambda t: t[:3] + (t[3].transpose(1, 2).contiguous().transpose(1, 2),) + t[4:]), "one shape and layout"),
    (dict(change=lambda t: t[:2] + (misaligned(t[2]),) + t[3:]), "params 4-byte aligned"),
    (dict(mask=torch.ones(1, 1, 4, 199, dtype=torch.bool)), "the mask must cover 200 positions"), (dict(length=301), "the length must lie in 4..300")])
def test_the_plan_refuses_before_any_launch(how, why):
    how = dict(how)
    change, mask, length, bits = how.pop("change", lambda t: t), how.pop("mask", None), how.pop("length", 200), how.get("bits", 8)
    q, *cache = change(tensors(**dict(how, bits=8 if bits == 3 else bits)))
    for call in (ops.attn_chunk_quant_plan, ops.attn_chunk_quant):          # the op refuses through its plan: CPU tensors never reach a launch
        with pytest.raises(ops.QllmUnsupported, match=why):
            call(q, *cache, bits, length, mask)


def test_the_plan_tuples_of_two_served_calls():
    q, *cache = tensors()
    assert ops.attn_chunk_quant_plan(q, *cache, 8, 200) == (1, 8, 2, 64, 8, 4, 300, 0, 256, 64, 0, 19200, 64, 0, 600, 2, _lib.ATTN_MASK_NONE, 0, 0, 0)
    q, *cache = tensors(b=2, hq=4, hk=4, d=128, s=2, L=64, bits=4, dtype=torch.bfloat16)
    q = torch.zeros(2, 2, 4, 128, dtype=torch.bfloat16).transpose(1, 2)         # the view of the projection output
    mask = torch.ones(2, 1, 2, 64, dtype=torch.bool)
    assert ops.attn_chunk_quant_plan(q, *cache, 4, torch.tensor(10), mask) == (2, 4, 4, 128, 4, 2, 64, 1024, 128, 512, 16384, 4096, 64, 2048, 512, 8,
                                                                              _lib.ATTN_MASK_BOOL, 64, 128, 64)


def test_every_instantiation_is_built_without_scratch_or_spills():
    kernels = {name: r for name, r in resources("attn_chunk_quant.hip").items() if "attn_chunk_quant_kernel" in name}
    assert len(kernels) == 24, sorted(kernels)                                       # 2 types x 2 head sizes x 2 widths x 3 mask kinds
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)


# ---- the modules ------------------------------------------------------------------------------------------------------------------------------------------
PIECES = ((0, 5), (5, 9))                        # a prompt, a masked chunk of four behind it


def restatements(monkeypatch):
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    fake_rope(monkeypatch)
    calls = []

    def kv_quantize(src, codes, params, bits, pos0=0):
        at = slice(int(pos0), int(pos0) + src.shape[2])
        codes[:, :, at], params[:, :, at] = quantize_rows(src, bits)

    def attn_chunk_quant(q, kc, kp, vc, vp, bits, length, **kw):
        calls.append(("codes", q.shape[2], int(length), isinstance(length, torch.Tensor), kw.get("mask") is not None))
        return AP.restated(q, dequantize_rows(kc, kp, bits), dequantize_rows(vc, vp, bits), length, **kw)

    def attn_chunk(q, k_cache, v_cache, length, **kw):
        calls.append(("chunk", q.shape[2], int(length)))
        return AP.restated(q, k_cache, v_cache, length, **kw)

    for name, op in (("kv_quantize", kv_quantize), ("attn_chunk_quant", attn_chunk_quant), ("attn_chunk", attn_chunk), ("attn_prefill", S.prefill_restated)):
        monkeypatch.setattr(ops, name, op)
    return calls


def run(model, prefill, inp, cache, calls):
    del calls[:]
    assert install_fused_attention(model, prefill=prefill) == D.LAYERS
    assert fused_attention.count_fused_attention_prefill(model) == D.LAYERS
    ids, mask = inp.ids, inp.mask
    try:
        with torch.no_grad():
            out = [model(ids[:, a:b], attention_mask=None if mask is None else mask[:, :b], position_ids=inp.pos[:, a:b], past_key_values=cache,
                         use_cache=True).logits for a, b in PIECES]
        return out[-1], list(calls)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS


@pytest.mark.parametrize("bits", (8, 4))
def test_codes_routes_the_chunk_to_the_new_op_only_under_its_conditions(bits, monkeypatch):
    model = tiny_model("llama", "sdpa", torch.float16, "cpu")
    inp = D.batch_inputs("padded")
    quant = lambda: qllm_amd.quant_static_cache(model.config, D.MAX_CACHE_LEN, bits=bits)
    calls = restatements(monkeypatch)
    split, split_calls = run(model, "split", inp, quant(), calls)
    codes, codes_calls = run(model, "codes", inp, quant(), calls)
    assert split_calls == [("chunk", 4, 9)] * D.LAYERS
    assert codes_calls == [("codes", 4, 9, True, True)] * D.LAYERS            # the length behind `advance`, read from the device counter; the mask
    assert D.same_bits(codes, split)                                            # the same dequantised values either way
    # what keeps a call off the new route leaves it exactly where "split" takes it: a refused plan, the row bound, a cache without room
    # for the rows (`update` then raises as it does under "split"), a layer that is not quantized
    def refuse(*a, **kw):
        raise ops.QllmUnsupported(_lib.QLLM_ERR_UNSUPPORTED, "refused here")
    with monkeypatch.context() as m:
        m.setattr(ops, "attn_chunk_quant_plan", refuse)
        again, again_calls = run(model, "codes", inp, quant(), calls)
    assert again_calls == split_calls and D.same_bits(again, split)
    with monkeypatch.context() as m:
        m.setattr(fused_attention, "SPLIT_MAX_ROWS", 3)
        assert not [c for c in run(model, "codes", inp, quant(), calls)[1] if c[0] == "codes"]
    with pytest.raises(ValueError, match="do not fit"):
        run(model, "codes", inp, qllm_amd.quant_static_cache(model.config, 8, bits=bits), calls)
    assert not [c for c in calls if c[0] == "codes"]
    assert run(model, "codes", inp, D.make_cache(model, "static"), calls)[1] == split_calls


def test_the_option_value_installs_its_core_and_unknown_values_still_raise():
    model = tiny_model("llama", "sdpa", torch.float16, "cpu")
    assert install_fused_attention(model, prefill="codes") == D.LAYERS
    assert {mod.__dict__[fused_attention._CORE][3] for mod in model.modules() if fused_attention._CORE in mod.__dict__} == {fused_attention._fused_core_codes}
    assert uninstall_fused_attention(model) == D.LAYERS
    for bad in ("chunk", "code", 2, ("codes",)):
        with pytest.raises(ValueError):
            install_fused_attention(model, prefill=bad)
