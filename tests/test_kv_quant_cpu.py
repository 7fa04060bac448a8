"""Host logic of the quantized KV cache (modeling/quant_cache.py, the quant_static kind of q_layers/fused_attention.py, the C entries'
host rules), no GPU: the layer's torch path against the format's formulas, the counters, `to_quant`, `_layer_of`, the symbols, describe."""
import pytest
import torch
from transformers import StaticCache
from transformers.cache_utils import StaticLayer, StaticSlidingWindowLayer

import decode_loop_cases as DL

import qllm_amd
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention
from qllm_amd.modeling.quant_cache import QuantStaticLayer, _readable, dequantize_rows, quantize_rows, to_quant

quant = pytest.mark.parametrize("bits", [8, 4])
types = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["float16", "bfloat16"])


@types
@quant
def test_torch_path_is_the_format(bits, dtype):
    x = torch.randn((2, 2, 5, 64), generator=torch.Generator().manual_seed(bits)) * 3
    x[0, 0, 0, :32] = 1.5            # constant: s == 0 at 4 bits
    x[0, 0, 2, :32] = 0              # s == 0 at both
    x[0, 0, 1, 7] = -40              # the largest magnitude is negative
    x = x.to(dtype)
    codes, params = quantize_rows(x, bits)
    g = x.double().unflatten(-1, (2, 32))
    if bits == 8:
        s = (g.abs().amax(-1).float() / 127.0).to(dtype)
        z = torch.zeros_like(s)
        c = torch.round(g.float() / s.float()[..., None]).clamp(-127, 127)
        got_c = codes.view(torch.int8).float()
    else:
        z, s = g.amin(-1).to(dtype), ((g.amax(-1) - g.amin(-1)).float() / 15.0).to(dtype)
        c = torch.round((g.float() - z.float()[..., None]) / s.float()[..., None]).clamp(0, 15)
        got_c = torch.stack((codes & 15, codes >> 4), -1).flatten(-2).float()        # element i in nibble i, low nibble first
    c = torch.where(s[..., None] == 0, torch.zeros_like(c), c)
    assert codes.shape[-1] == 64 * bits // 8 and torch.equal(got_c, c.flatten(-2))
    assert torch.equal(params, s if bits == 8 else torch.cat((s, z), -1)) and bool(s[0, 0, 2, 0] == 0) and bool(s[0, 0, 0, 0] == 0) == (bits == 4)
    want = (z.double()[..., None] + c.double() * s.double()[..., None]).flatten(-2).float().to(dtype)
    assert torch.equal(dequantize_rows(codes, params, bits), want)
    assert (want.float() - x.float()).abs().max() <= s.float().max() * (0.5 if bits == 8 else 1.0) + 1e-6


@quant
def test_layer_counters_and_shapes(bits):
    cache = qllm_amd.quant_static_cache(DL.llama_config(), 16, bits=bits)
    assert [type(layer) for layer in cache.layers] == [QuantStaticLayer] * DL.LAYERS and cache.layers[0].scratch is cache.layers[1].scratch
    k, v = (torch.randn(2, 2, 5, 64).half() for _ in range(2))
    keys, values = cache.update(k, v, 0)
    layer = cache.layers[0]
    assert keys.shape == values.shape == (2, 2, 16, 64) and keys.dtype == torch.float16
    assert torch.equal(keys[:, :, :5], dequantize_rows(*quantize_rows(k, bits), bits)) and int(keys[:, :, 5:].count_nonzero()) == 0
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (5, 5)
    assert cache.update(k, v, 1)[0] is keys                      # one scratch pair for all layers
    keys, _ = cache.update(k[:, :, :1], v[:, :, :1], 0)
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (6, 6) and torch.equal(keys[:, :, 5], keys[:, :, 0])
    layer.advance(2)
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (8, 8)
    cache.layers[1].advance(3)                                   # (both layers at 8: Cache.crop walks them all)
    cache.crop(-3)                                               # transformers' contract: a negative value removes that many tokens
    assert [(int(x.cumulative_length), x.cumulative_length_int) for x in cache.layers] == [(5, 5), (5, 5)]
    cache.crop(0), cache.crop(7)                                 # nothing to do; the legacy absolute length, not below what is held
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (5, 5)
    cache.crop(4)                                                # the legacy absolute length
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (4, 4)
    cache.crop(-9)                                               # more than is held: empty
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (0, 0)
    layer.advance(5)
    with pytest.raises(ValueError):
        layer.batch_select_indices(torch.tensor([0]))
    layer.reset()
    assert (int(layer.cumulative_length), layer.cumulative_length_int) == (0, 0)
    with pytest.raises(ValueError):
        layer.update(torch.zeros(2, 2, 17, 64).half(), torch.zeros(2, 2, 17, 64).half())
    off = torch.zeros(1, 2, 3, 72).half()[..., 4:68]             # 8 bytes off: what kv_quantize cannot read in place is copied
    assert _readable(k) is k and _readable(k.transpose(1, 2)).data_ptr() == k.data_ptr() and _readable(off).is_contiguous() and _readable(off) is not off


def test_to_quant_refusals_and_layer_kinds():
    config = DL.llama_config()
    with pytest.raises(ValueError):
        to_quant(StaticCache(config, max_cache_len=16), bits=3)
    offloading = StaticCache(config, max_cache_len=16)
    offloading.offloading = True          # (building one needs a device stream)
    with pytest.raises(ValueError):
        to_quant(offloading)
    used = StaticCache(config, max_cache_len=16)
    used.update(torch.zeros(1, 2, 1, 64), torch.zeros(1, 2, 1, 64), 0)
    with pytest.raises(ValueError):
        to_quant(used)
    with pytest.raises(ValueError):
        to_quant(object())
    mixed = StaticCache(config, max_cache_len=16)
    mixed.layers[1] = StaticSlidingWindowLayer(max_cache_len=16, sliding_window=8)
    to_quant(mixed, 4)
    assert type(mixed.layers[0]) is QuantStaticLayer and mixed.layers[0].bits == 4 and type(mixed.layers[1]) is StaticSlidingWindowLayer
    assert fused_attention._layer_of(mixed, 0) == (None, None) and fused_attention._layer_of(mixed, 0, uninitialized=True) == (mixed.layers[0], "quant_static")
    assert fused_attention._layer_of(mixed, 0, uninitialized=True, sliding=8) == (None, None)
    plain = StaticCache(config, max_cache_len=16)
    assert type(plain.layers[0]) is StaticLayer and fused_attention._layer_of(plain, 0, uninitialized=True)[1] == "static"

    class Sub(QuantStaticLayer):
        pass
    mixed.layers[0] = Sub(16)
    assert fused_attention._layer_of(mixed, 0, uninitialized=True) == (None, None)


def test_symbols_and_describe():
    lib = _lib.load()
    for name in ("qllm_attn_decode_quant", "qllm_attn_decode_quant_describe", "qllm_kv_quantize", "qllm_kv_dequantize"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    text = ops.attn_decode_quant_describe(1, 32, 8, 128, 4, 4096)
    assert text.startswith("attn_decode_quant bits=4 tile=64 ") and text.endswith("group=4 combine=last-block")
    assert text.split(" ", 2)[2] == ops.attn_decode_describe(1, 32, 8, 128, 4096).split(" ", 1)[1]      # attn_decode's geometry: its workspace serves
    for args, why in (((1, 4, 2, 64, 3, 64), "8- and 4-bit"), ((1, 4, 2, 96, 8, 64), "head_dim 64 and 128"), ((1, 9, 1, 64, 8, 64), "query heads per kv head")):
        text = ops.attn_decode_quant_describe(*args)
        assert text.startswith("refused: ") and why in text, text
    for args in ((1, 4, 3, 64, 8, 64), (0, 4, 2, 64, 8, 64)):            # invalid, not unserved: the entry's error
        with pytest.raises(_lib.QllmError):
            ops.attn_decode_quant_describe(*args)
    q, k = torch.zeros(1, 4, 1, 64).half(), torch.zeros(1, 2, 1, 64).half()
    cache = [torch.zeros(1, 2, 16, n, dtype=t) for n, t in ((64, torch.uint8), (2, torch.float16))] * 2
    assert ops.attn_decode_quant_plan(q, *cache, 8, 3, k, k)[:6] == (1, 4, 2, 64, 8, 16)
    for bad in (dict(bits=4), dict(length=16), dict(length=-1)):
        with pytest.raises(ops.QllmUnsupported):
            ops.attn_decode_quant_plan(q, *cache, bad.get("bits", 8), bad.get("length", 3), k, k)


def quant_call(lib, bits=8, d=64, hq=8, hk=2, kv_len=10, max_len=100, q=4096, k_new=8192, v_new=12288, k_codes=16384, k_params=20480, v_codes=24576,
               v_params=28672, out=32768, codes_pos=64, params_pos=2, mask_len=100):
    """qllm_attn_decode_quant with an append and a bool mask over made-up addresses and NO workspace: a call that passes every rule ends
    in QLLM_ERR_WORKSPACE, before any device work."""
    return lib.qllm_attn_decode_quant(q, k_new, v_new, k_codes, k_params, v_codes, v_params, 36864, out, 2, hq, hk, d, bits, kv_len, None, max_len,
                                      hq * d, d, hk * d, d, hk * d, d, hk * 100 * codes_pos, 100 * codes_pos, codes_pos, hk * 100 * 2, 100 * 2, params_pos,
                                      _lib.ATTN_MASK_BOOL, mask_len, 100, 0.125, _lib.DT_F16, None, 0, None)


@pytest.mark.parametrize("how,status,why", [
    ({}, "QLLM_ERR_WORKSPACE", "workspace"),
    ({"bits": 4, "codes_pos": 32, "params_pos": 4}, "QLLM_ERR_WORKSPACE", "workspace"),
    ({"bits": 3}, "QLLM_ERR_UNSUPPORTED", "8- and 4-bit"),
    ({"d": 96}, "QLLM_ERR_UNSUPPORTED", "head_dim 64 and 128"),
    ({"hq": 18}, "QLLM_ERR_UNSUPPORTED", "query heads per kv head"),
    ({"k_params": None}, "QLLM_ERR_INVALID", "only some of the four"),
    ({"v_codes": None, "v_params": None}, "QLLM_ERR_INVALID", "only some of the four"),
    ({"k_codes": None, "k_params": None, "v_codes": None, "v_params": None}, "QLLM_ERR_INVALID", "must not be NULL"),
    ({"v_codes": 24576 + 8}, "QLLM_ERR_INVALID", "codes must be 16-byte aligned"),
    ({"k_params": 20480 + 2}, "QLLM_ERR_INVALID", "params 4-byte aligned"),
    ({"codes_pos": 60}, "QLLM_ERR_INVALID", "codes strides"),
    ({"params_pos": 3}, "QLLM_ERR_INVALID", "params strides"),
    ({"kv_len": 100}, "QLLM_ERR_INVALID", "kv_len + 1 (append)"),
    ({"mask_len": 10}, "QLLM_ERR_INVALID", "the mask must cover 11"),
    ({"bits": 3, "params_pos": 3}, "QLLM_ERR_INVALID", "params strides"),          # the decode entry's order: the layout before what is served
    ({"bits": 3, "mask_len": 10}, "QLLM_ERR_INVALID", "the mask must cover 11"),
], ids=lambda x: "-".join(x) if isinstance(x, dict) else None)
def test_the_c_entry_refuses_before_any_device_work(how, status, why):
    rc = quant_call(_lib.load(), **how)
    assert rc == getattr(_lib, status) and why in _lib.last_error(), (rc, _lib.last_error())
