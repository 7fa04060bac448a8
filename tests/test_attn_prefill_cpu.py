"""No GPU: the host side of prefill attention over the KV cache (qllm_attn_prefill, csrc/attn_prefill.hip) -- symbols and ABI, every
argument check on fake, aligned, never-dereferenced pointers, the pure describe function, the kernels' resources, ops.attn_prefill_plan,
and the modules of q_layers/fused_attention.py with ops.attn_prefill (and ops.attn_decode) replaced by counting torch restatements
(tests/attn_prefill_cases.py: fp32 softmax over the visible keys).

Module tolerance: tests/test_attn_decode_cpu.py's (the restated op rounds once where the eager route rounds scores, weights and output):
logits of the tiny fp16 models are held to 2e-2 absolute, and wherever the family's route runs, to exact equality."""
import ctypes as C
import functools
import inspect
import os
import re

import pytest
import torch

from attn_entry_cases import PREFILL_PTRS, PREFILL_STRIDES, prefill_call
from attn_prefill_cases import oracle, eager, parse_describe, restated
from kernel_resources import resources
from test_attn_decode_cpu import FAMILIES, close, fake_op, make_cache, prefill_and_decode, tiny_model
from test_rope_cpu import module_dicts

from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import (fused_attention, install_fused_attention, install_fused_rope, uninstall_fused_attention,
                                        uninstall_fused_rope)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("library not built")
    return _lib.load()


def fake_ops(monkeypatch):
    """test_attn_decode_cpu.fake_op, plus `ops.attn_prefill` replaced by the counting restatement."""
    calls = fake_op(monkeypatch)
    calls.update(prefill=0, shapes=[], masks=[], causal=[])

    def attn_prefill(q, k_cache, v_cache, length, mask=None, causal=True, scaling=None, *, out=None, plan=None):
        calls["prefill"] += 1
        calls["shapes"].append((q.shape[2], int(length)))
        calls["masks"].append(mask)
        calls["causal"].append(causal)
        assert out is None and plan == ops.attn_prefill_plan(q, k_cache, v_cache, length, mask)
        return restated(q, k_cache, v_cache, length, mask, causal, scaling)

    monkeypatch.setattr(fused_attention.ops, "attn_prefill", attn_prefill)
    return calls


# ---- symbols, validation, the pure describe function, resources ------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read(), flags=re.S)
    for name in ("qllm_attn_prefill", "qllm_attn_prefill_describe"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and C.cast(getattr(lib, name), C.c_void_p).value, name
    assert len(lib.qllm_attn_prefill.argtypes) == 27 and lib.qllm_attn_prefill.argtypes[12:19] == [C.c_int64] * 7
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert all(hasattr(ops, n) for n in ("attn_prefill", "attn_prefill_plan", "attn_prefill_describe"))
    assert "attn_prefill.hip" in open(os.path.join(ROOT, "qllm_amd", "csrc", "Makefile")).read()


def test_every_argument_check_fires_before_any_device_work(lib):
    """Every call here is refused: none reaches a launch, so the fake pointers are never dereferenced."""
    INV, UNS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED
    P, S0 = PREFILL_PTRS, PREFILL_STRIDES
    call = functools.partial(prefill_call, lib)

    def refused(status, text, **kw):
        return call(**kw) == status and text in _lib.last_error()

    for name in ("q", "k_cache", "v_cache", "out"):
        assert refused(INV, "must not be NULL", **{name: None}), name
    for bad in (dict(b=0), dict(b=-1), dict(hq=0), dict(hk=0), dict(d=0), dict(d=-64), dict(max_len=0), dict(max_len=-5)):
        assert refused(INV, "must be >= 1", **bad), bad
    for s in (1, 0, -3, 101):
        assert refused(INV, "q_len must lie in 2..max_len", s=s), s
    for hq, hk in ((8, 3), (2, 4), (7, 2)):
        assert refused(INV, "must divide", hq=hq, hk=hk), (hq, hk)
    for dt in (7, _lib.DT_F32, -1):
        assert refused(INV, "act_dtype", dt=dt), dt
    for kind in (3, -1):
        assert refused(INV, "mask_kind", mask_kind=kind), kind
    assert refused(INV, "mask must be NULL exactly", mask=None) and refused(INV, "mask must be NULL exactly", mask_kind=_lib.ATTN_MASK_NONE)
    for causal in (2, -1):
        assert refused(INV, "causal must be 0 or 1", causal=causal), causal
    for name in ("q", "k_cache", "v_cache", "out"):
        assert refused(INV, "16-byte aligned", **{name: P[name] + 8}), name
    assert refused(INV, "8-byte aligned", len_dev=P["len_dev"] + 4)
    assert refused(INV, "2-byte aligned", mask=P["mask"] + 1, mask_kind=_lib.ATTN_MASK_ADDITIVE)
    for i in range(6):
        for v in (4, 12, -8):
            st = list(S0)
            st[i] = v
            assert refused(INV, "multiples of 8", strides=tuple(st)), (i, v)
    # the host length: q_len..max_len; on the device it is not looked at, but the mask must then cover max_len
    for kv_len in (4, 0, -1, 101):
        assert refused(INV, "q_len..max_len", kv_len=kv_len), kv_len
    assert refused(INV, "mask must cover 10 ", mask_len=9) and refused(INV, "mask must cover 100 ", mask_len=99, kv_len=10 ** 6, len_dev=P["len_dev"])
    assert refused(INV, "non-negative batch and row strides", mask_batch=-100) and refused(INV, "non-negative batch and row strides", mask_row=-1)
    # what the kernel is not built for: unsupported, with the value -- the last check, so everything above was accepted to get here
    for d in (32, 96, 256):
        assert refused(UNS, "head_dim", d=d) and str(d) in _lib.last_error(), d
    assert refused(UNS, "(got 9)", hq=18, hk=2)
    assert refused(UNS, "65535", b=70000)
    # mask strides may be anything non-negative (0 and odd values included): such a call gets past the mask checks to the last one
    assert refused(UNS, "head_dim", d=96, mask_batch=0, mask_row=101, mask_len=10, kv_len=5) and refused(UNS, "head_dim", d=96, kv_len=100, s=100)


def test_describe_is_pure_and_reports_the_tiles_and_the_grid(lib):
    a = ops.attn_prefill_describe(1, 32, 8, 128, 300, 4096)
    assert a == ops.attn_prefill_describe(1, 32, 8, 128, 300, 4096) and a.startswith("attn_prefill q_tile=")
    assert all(key in a for key in ("q_tile=", "kv_tile=", "grid=")) and "kv_len" not in a      # the entry takes no length: nothing to depend on
    g = parse_describe(a)
    assert g["group"] == 4 and g["grid"] == (-(-300 // g["q_tile"]), 32, 1)
    for b, hq, hk, d, s in ((1, 1, 1, 64, 2), (3, 8, 2, 64, 2 * g["q_tile"] + 1), (3, 7, 1, 128, g["q_tile"]), (2, 8, 1, 128, g["q_tile"] + 1)):
        h = parse_describe(ops.attn_prefill_describe(b, hq, hk, d, s, s + 70))
        assert h["grid"] == (-(-s // h["q_tile"]), hq, b) and h["group"] == hq // hk and h["q_tile"] % 32 == 0 and h["kv_tile"] % 32 == 0
        assert h["grid"] == parse_describe(ops.attn_prefill_describe(b, hq, hk, d, s, 1 << 20))["grid"]    # nor on the cache's size
    assert ops.attn_prefill_describe(1, 32, 8, 96, 300, 4096).startswith("refused: ") and "96" in ops.attn_prefill_describe(1, 32, 8, 96, 300, 4096)
    with pytest.raises(_lib.QllmError):
        ops.attn_prefill_describe(1, 32, 5, 128, 300, 4096)
    with pytest.raises(_lib.QllmError):
        ops.attn_prefill_describe(1, 32, 8, 128, 1, 4096)


def test_the_kernels_use_no_scratch_and_spill_nothing():
    res = resources("attn_prefill.hip")
    assert len(res) == 12, sorted(res)                                                      # 2 types x 2 head sizes x 3 mask kinds
    for n, r in res.items():
        assert "attn_prefill_kernel" in n
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert 0 < r["group_segment_fixed_size"] <= 2 * 64 * (128 + 8) * 2, (n, r)          # a K and a V tile of [kv_tile][D + 8]


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------
def tensors(b=2, hq=8, hk=2, d=64, s=5, L=40, dtype=torch.float16):
    g = torch.Generator().manual_seed(1)
    q = torch.randn(b, s, hq, d, generator=g).to(dtype).transpose(1, 2)                     # the projection output viewed as [B, Hq, S, D]
    return q, torch.randn(b, hk, L, d, generator=g).to(dtype), torch.randn(b, hk, L, d, generator=g).to(dtype)


def test_plan_derives_sizes_and_strides():
    q, k, v = tensors()
    assert ops.attn_prefill_plan(q, k, v, 7) == (2, 8, 2, 64, 5, 40, 5 * 512, 64, 512, 2 * 40 * 64, 40 * 64, 64, 0, 0, 0, 0)
    assert ops.attn_prefill_plan(q.contiguous(), k, v, 40)[6:9] == (8 * 5 * 64, 5 * 64, 64)                   # [B, Hq, S, D] memory
    buf = torch.zeros(2, 5, (8 + 4) * 64, dtype=torch.float16)                                               # q inside a wider q/k/v row
    assert ops.attn_prefill_plan(buf[..., :512].view(2, 5, 8, 64).transpose(1, 2), k, v, 9)[6:9] == (5 * 768, 64, 768)
    kt = torch.zeros(2, 40, 2, 64, dtype=torch.float16).transpose(1, 2)                                      # [B, L, Hkv, D] memory
    assert ops.attn_prefill_plan(q, kt, kt.clone(memory_format=torch.preserve_format), 9)[9:12] == (40 * 128, 64, 128)
    mb = torch.ones(2, 1, 5, 40, dtype=torch.bool)
    assert ops.attn_prefill_plan(q, k, v, 40, mask=mb)[12:] == (_lib.ATTN_MASK_BOOL, 40, 200, 40)
    assert ops.attn_prefill_plan(q, k, v, 9, mask=mb[..., :9])[12:] == (_lib.ATTN_MASK_BOOL, 9, 200, 40)      # a view of longer rows
    assert ops.attn_prefill_plan(q, k, v, 9, mask=torch.zeros(2, 5, 40, dtype=torch.float16))[12:] == (_lib.ATTN_MASK_ADDITIVE, 40, 200, 40)
    assert ops.attn_prefill_plan(q, k, v, 9, mask=mb[:1])[12:] == (_lib.ATTN_MASK_BOOL, 40, 0, 40)            # one mask for the batch
    assert ops.attn_prefill_plan(q, k, v, 9, mask=mb[:1].expand(2, 1, 5, 40))[12:] == (_lib.ATTN_MASK_BOOL, 40, 0, 40)   # batch stride 0
    assert ops.attn_prefill_plan(q, k, v, torch.tensor(5), mask=mb)[5] == 40                                 # the length on the device
    q1, k1, v1 = tensors(b=1, hq=28, hk=4, d=128, dtype=torch.bfloat16)
    assert ops.attn_prefill_plan(q1, k1, v1, 5)[:9] == (1, 28, 4, 128, 5, 40, 0, 128, 28 * 128)


def test_plan_refuses_what_the_entry_does_not_serve():
    q, k, v = tensors()
    mb = torch.ones(2, 1, 5, 40, dtype=torch.bool)

    def refused(*a, **kw):
        with pytest.raises(ops.QllmUnsupported):
            ops.attn_prefill_plan(*a, **kw)
        return True

    assert refused(q.float(), k.float(), v.float(), 7)                                       # fp32
    assert refused(q, k.bfloat16(), v, 7)                                                    # mixed types
    assert refused(q[:, :, :1], k, v, 7)                                                     # one query token: attn_decode's
    assert refused(q[0], k, v, 7) and refused(q, k[0], v[0], 7)                              # not 4-D
    assert refused(q, k, v[:, :, :39], 7) and refused(q, k, v.transpose(1, 2).contiguous().transpose(1, 2), 7)   # caches of two shapes / layouts
    assert refused(q[:1], k, v, 7)                                                           # another batch
    assert refused(*tensors(hq=8, hk=3), 7) and refused(*tensors(hq=18, hk=2), 7)            # heads that do not divide; a group of 9
    assert refused(*tensors(d=32), 7) and refused(*tensors(d=96), 7) and refused(*tensors(d=256), 7)
    assert refused(q, k.transpose(2, 3).contiguous().transpose(2, 3), v.transpose(2, 3).contiguous().transpose(2, 3), 7)   # D not contiguous
    assert refused(q.transpose(2, 3).contiguous().transpose(2, 3), k, v, 7)                  # nor q's
    assert refused(q, k, v, 4) and refused(q, k, v, 41) and refused(q, k[:, :, :4], v[:, :, :4], 4)   # the length: S..L; caches shorter than S
    assert refused(q, k, v, torch.tensor(5, dtype=torch.int32)) and refused(q, k, v, torch.tensor([5]))   # a device length of another kind
    assert refused(q, k, v, 10, mask=mb[..., :9]) and refused(q, k, v, torch.tensor(5), mask=mb[..., :39])   # a short mask
    assert refused(q, k, v, 7, mask=mb.float()) and refused(q, k, v, 7, mask=torch.ones(3, 1, 5, 40, dtype=torch.bool))   # fp32 mask; three batch rows
    assert refused(q, k, v, 7, mask=torch.ones(2, 1, 1, 40, dtype=torch.bool)) and refused(q, k, v, 7, mask=torch.ones(2, 40, dtype=torch.bool))   # decode's forms
    assert refused(q, k, v, 7, mask=torch.ones(2, 8, 5, 40, dtype=torch.bool))               # a mask per head
    assert refused(q, k, v, 7, mask=torch.ones(2, 1, 40, 5, dtype=torch.bool).transpose(2, 3))   # inner stride not 1
    odd = torch.zeros(2 * 5 * 8 * 64 + 4, dtype=torch.float16)[4:].view(2, 5, 8, 64).transpose(1, 2)
    assert refused(odd, k, v, 7)                                                             # q off 16 bytes


def test_the_restatement_is_attention():
    q, k, v = tensors(b=2, hq=8, hk=2, d=64, s=5, L=40)
    for n, causal, mask in ((17, True, None), (5, True, None), (17, False, None), (17, True, torch.rand(2, 1, 5, 40, generator=torch.Generator().manual_seed(2)) < 0.7)):
        ref = oracle(q, k, v, n, 0.125, causal, mask)
        got = restated(q, k, v, n, mask, causal)
        assert got.shape == (2, 5, 8, 64) and got.dtype == q.dtype
        assert (got.double() - ref).abs().max() <= (eager(q, k, v, n, 0.125, causal, mask).double() - ref).abs().max()
    # row i of a causal call is the decode restatement's answer for that row over q_start + i + 1 keys, to an ulp of the type near 1
    from attn_decode_cases import restated as decode_restated
    got = restated(q, k, v, 17)
    for i in range(5):
        assert (got[:, i].float() - decode_restated(q[:, :, i:i + 1], k, v, 17 - 5 + i + 1).float()).abs().max() <= 2e-3


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------
def run(model, kind, mask=None, batch=2, chunk=0):
    """Logits of a 5-token prompt (left-padded where `mask` says), of a further chunk of `chunk` tokens, and of 2 decode steps."""
    ids = torch.randint(0, 64, (batch, 5 + chunk + 2), generator=torch.Generator().manual_seed(3))
    cache = make_cache(model, kind)
    full = None if mask is None else torch.cat((mask, torch.ones(batch, chunk + 2, dtype=mask.dtype)), 1)
    outs, at = [], 0
    with torch.no_grad():
        for step in [5] + ([chunk] if chunk else []) + [1, 1]:
            kw = {} if full is None else dict(attention_mask=full[:, :at + step])
            outs.append(model(ids[:, at:at + step], past_key_values=cache, use_cache=True, **kw).logits)
            at += step
    return outs


def padded():
    mask = torch.ones(2, 5, dtype=torch.long)
    mask[1, :2] = 0
    return mask


@pytest.mark.parametrize("kind", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("family", FAMILIES)
def test_flag_off_prefill_is_the_family_route_and_flag_on_one_call_per_layer(family, attn, kind, monkeypatch):
    model = tiny_model(family, attn)
    before = module_dicts(model)
    want, want_padded = run(model, kind), run(model, kind, padded())
    calls = fake_ops(monkeypatch)
    assert install_fused_attention(model) == 2                                                   # flag off: today's behaviour
    got = run(model, kind)
    assert calls["prefill"] == 0 and calls["attn"] == 2 * 2 and torch.equal(got[0], want[0]) and close(got, want)
    assert torch.equal(run(model, kind, padded())[0], want_padded[0]) and calls["prefill"] == 0
    assert uninstall_fused_attention(model) == 2 and module_dicts(model) == before
    calls["attn"] = 0
    assert install_fused_attention(model, prefill=True) == 2 and install_fused_attention(model, prefill=True) == 0
    assert fused_attention.count_fused_attention_prefill(model) == 2
    got = run(model, kind)                                                                       # the unpadded prompt
    if attn == "sdpa":                                                                           # mask None: the layer held nothing before
        assert calls["prefill"] == 2 and calls["shapes"] == [(5, 5)] * 2 and calls["masks"] == [None] * 2
    else:                                                                                        # eager always builds the additive mask
        assert calls["prefill"] == 2 and all(m is not None and m.dtype == torch.float16 and m.shape[1:3] == (1, 5) for m in calls["masks"])
    assert calls["attn"] == 2 * 2 and calls["causal"] == [True] * 2 and close(got, want)
    got = run(model, kind, padded())                                                             # the left-padded prompt: causal = 1 plus the mask
    assert calls["prefill"] == 4 and calls["shapes"][2:] == [(5, 5)] * 2 and calls["causal"] == [True] * 4
    assert all(m is not None and m.shape[:3] == (2, 1, 5) and m.shape[3] == (5 if kind == "dynamic" else 16) for m in calls["masks"][2:])
    assert close([g[0] for g in got], [w[0] for w in want_padded]) and close([g[1, 2:] for g in got[:1]] + [g[1] for g in got[1:]],
                                                                            [w[1, 2:] for w in want_padded[:1]] + [w[1] for w in want_padded[1:]])
    assert uninstall_fused_attention(model) == 2 and module_dicts(model) == before
    again = run(model, kind)
    assert calls["prefill"] == 4 and all(torch.equal(a, w) for a, w in zip(again, want))


@pytest.mark.parametrize("kind", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
def test_a_second_chunk_behind_cached_tokens(attn, kind, monkeypatch):
    """A chunk of 3 behind 5 cached tokens always carries a mask ([B, 1, 3, 8] or [B, 1, 3, 16], batch stride 0 under sdpa).  On a static
    layer: one call per layer with q_len 3 over 8 keys.  On a dynamic layer PREFILL_ROUTES keeps masked chunks on the family's route."""
    model = tiny_model("llama", attn)
    want = run(model, kind, chunk=3)
    calls = fake_ops(monkeypatch)
    assert install_fused_attention(model, prefill=True) == 2
    got = run(model, kind, chunk=3)
    assert calls["shapes"] == [(5, 5)] * 2 + ([(3, 8)] * 2 if kind == "static" else []) and close(got, want)
    assert all(m is not None and m.shape[2:] == (3, 16) for m in calls["masks"][2:])


def test_each_rule_takes_the_family_route(monkeypatch):
    from transformers import DynamicCache, StaticCache
    calls = fake_ops(monkeypatch)

    def zero_calls(model, kind="dynamic", **kw):
        want = run(model, kind, **kw)
        n = install_fused_attention(model, prefill=True)
        got = run(model, kind, **kw)
        assert uninstall_fused_attention(model) == n
        assert calls["prefill"] == 0 and calls["attn"] == 0 and all(torch.equal(g, w) for g, w in zip(got, want))
        return n

    assert zero_calls(tiny_model("llama", dtype=torch.float32)) == 2                             # fp32
    assert zero_calls(tiny_model("llama", num_attention_heads=8, num_key_value_heads=8)) == 2    # head_dim 32: the plan refuses
    model = tiny_model("llama")
    attn = model.model.layers[0].self_attn
    q, k = torch.randn(1, 4, 3, 64).half(), torch.randn(1, 2, 3, 64).half()

    def fresh(held=0, kind="dynamic"):
        cache = DynamicCache(config=model.config) if kind == "dynamic" else StaticCache(config=model.config, max_cache_len=16)
        if held:
            cache.update(torch.randn(1, 2, held, 64).half(), torch.randn(1, 2, held, 64).half(), 0)
        return cache

    def core(mod=attn, q=q, k=k, mask=None, cache=None, window=None, held=0, kind="dynamic", **kwargs):
        cache = fresh(held, kind) if cache is None else cache
        n = int(cache.get_seq_length(0))
        out = fused_attention._fused_core_prefill(mod, q, k, k.clone(), mask, cache, kwargs, window)
        assert (out[0] is None) == (not out[3]) and int(cache.get_seq_length(0)) == n + (q.shape[2] if out[3] else 0)
        assert out[0] is None or out[0].shape == (q.shape[0], q.shape[2], q.shape[1], q.shape[3])
        return out[0] is not None

    full = lambda n: torch.ones(1, 1, 3, n, dtype=torch.bool)
    assert core() and core(kind="static") and calls["prefill"] == 2 and calls["shapes"] == [(3, 3)] * 2    # nothing cached, no mask: served
    assert not core(held=5) and not core(held=5, kind="static")                                  # mask None with tokens already cached
    assert core(held=5, kind="static", mask=full(16)) and calls["shapes"][-1] == (3, 8) and core(mask=full(3)) and calls["shapes"][-1] == (3, 3)
    assert not core(held=5, mask=full(8))                                                        # a masked chunk on a dynamic layer: not routed
    wide = torch.cat((q,) * 43, 2), torch.cat((k,) * 43, 2)                                      # 129 rows: above the dynamic masked line
    assert not core(q=wide[0], k=wide[1], mask=torch.ones(1, 1, 129, 129, dtype=torch.bool)) and core(q=wide[0], k=wide[1]) and calls["shapes"][-1] == (129, 129)
    assert core(mask=torch.zeros(1, 1, 3, 3).half()) and not core(mask=torch.zeros(1, 1, 3, 3))  # additive in the type; fp32
    assert not core(mask=full(3)[:, :, :2]) and not core(mask=full(3)[0]) and not core(mask=torch.ones(1, 4, 3, 3, dtype=torch.bool))
    assert fused_attention._fused_core_prefill(attn, q, k, k.clone(), None, None, {}, None)[0] is None       # no cache
    assert not core(q=q.float()) and not core(k=k.bfloat16())
    assert core(position_ids=torch.zeros(1, 3), use_cache=True, output_attentions=False, softcap=None)
    assert not core(output_attentions=True) and not core(softcap=30.0) and not core(sliding_window=8)
    mistral = tiny_model("mistral", sliding_window=8)
    assert not core(mod=mistral.model.layers[0].self_attn, window="config")                      # a sliding window reaches the call
    attn.sliding_window = 8
    assert not core(window="self")
    del attn.sliding_window
    attn.train()
    assert not core()                                                                            # training
    attn.eval()
    with torch.enable_grad():
        assert not core(q=q.clone().requires_grad_())
    attn.is_causal = False
    assert not core()                                                                            # a module that is not causal
    attn.is_causal = True
    model.config._attn_implementation = "flex_attention"
    assert not core()
    model.config._attn_implementation = "sdpa"
    cache = fresh()

    class Other(type(cache.layers[0])):
        pass
    cache.layers[0].__class__ = Other                                                            # a foreign cache layer
    assert not core(cache=cache)
    cache.layers[0].__class__ = Other.__bases__[0]
    cache.offloading = True
    assert not core(cache=cache)
    cache.offloading = False
    assert core(cache=cache)
    before = calls["prefill"]
    monkeypatch.setattr(fused_attention, "PREFILL_ROUTES", {("dynamic", False): (4, None, True), ("static", True): (2, 2, True)})
    assert not core() and not core(mask=full(3)) and not core(held=5, kind="static", mask=full(16)) and not core(kind="static")
    assert core(q=torch.cat((q, q[:, :, :1]), 2), k=torch.cat((k, k[:, :, :1]), 2)) and calls["prefill"] == before + 1   # q_len 4 is routed
    monkeypatch.undo()
    calls = fake_ops(monkeypatch)
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: all(t.is_cuda for t in ts))
    assert not core() and calls["prefill"] == 0                                                  # CPU tensors
    q1 = q[:, :, :1]
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    assert fused_attention._fused_core_prefill(attn, q1, k[:, :, :1], k[:, :, :1].clone(), None, fresh(4), {}, None)[0].shape == (1, 4, 64)   # one token: the decode core
    assert calls["attn"] == 1 and calls["prefill"] == 0


@pytest.mark.parametrize("order", ["rope first", "attention first"])
def test_install_and_uninstall_compose_with_fused_rope_in_both_orders(order, monkeypatch):
    from test_rope_cpu import fake_op as fake_rope
    model = tiny_model("llama")
    before = module_dicts(model)
    want, _ = prefill_and_decode(model, "static")
    calls, rope_calls = fake_ops(monkeypatch), fake_rope(monkeypatch)
    with_prefill = lambda m: install_fused_attention(m, prefill=True)
    first, second = (install_fused_rope, with_prefill) if order == "rope first" else (with_prefill, install_fused_rope)
    assert first(model) == 2 and second(model) == 2 and first(model) == 0 and second(model) == 0
    got, _ = prefill_and_decode(model, "static")
    assert calls["prefill"] == 2 and calls["attn"] == 2 * 4 and rope_calls["rope"] == 2 * 5 and close(got, want)
    undo = (uninstall_fused_rope, uninstall_fused_attention)
    for a, b in (undo, undo[::-1]):
        assert a(model) == 2 and "forward" in model.model.layers[0].self_attn.__dict__          # the other install still works
        n_pre, n_attn, n_rope = calls["prefill"], calls["attn"], rope_calls["rope"]
        got, _ = prefill_and_decode(model, "static")
        assert close(got, want)
        assert (calls["prefill"] - n_pre, calls["attn"] - n_attn, rope_calls["rope"] - n_rope) == ((0, 0, 10) if a is uninstall_fused_attention else (2, 8, 0))
        assert b(model) == 2 and module_dicts(model) == before
        assert first(model) == 2 and second(model) == 2
    assert uninstall_fused_attention(model) == 2 and uninstall_fused_rope(model) == 2 and module_dicts(model) == before


def test_the_environment_switch_and_the_loader_default(monkeypatch):
    from qllm_amd.modeling import base
    params = inspect.signature(base.load_quantized).parameters
    assert params["fuse_attention_prefill"].default is False and params["fuse_attention"].default is False
    assert inspect.signature(install_fused_attention).parameters["prefill"].default is False
    calls = fake_ops(monkeypatch)
    monkeypatch.setenv("QLLM_FUSE_ATTENTION_PREFILL", "0")
    model = tiny_model("llama")
    want = run(model, "dynamic")
    assert install_fused_attention(model, prefill=True) == 2 and fused_attention.count_fused_attention_prefill(model) == 0
    got = run(model, "dynamic")
    assert calls["prefill"] == 0 and calls["attn"] == 2 * 2 and torch.equal(got[0], want[0])     # the decode core alone
    assert uninstall_fused_attention(model) == 2
    monkeypatch.setenv("QLLM_FUSE_ATTENTION", "0")
    assert install_fused_attention(model, prefill=True) == 0 and not any("forward" in m.__dict__ for m in model.modules())
