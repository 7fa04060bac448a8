"""No GPU: the host side of single-token attention over the KV cache (qllm_attn_decode, csrc/attn_decode.hip) -- symbols and ABI, every
argument check on fake, aligned, never-dereferenced pointers, the pure workspace and describe functions, the kernels' resources,
ops.attn_decode_plan, and the modules of q_layers/fused_attention.py with ops.attn_decode replaced by a counting torch restatement
(tests/attn_decode_cases.py: fp32 softmax over the valid keys).

Module tolerance: the restated op rounds once where the eager route rounds scores, weights and output, so hidden states differ by a few
ulps of the activation type; logits of the tiny fp16 models (magnitude below 2) are held to 2e-2 absolute, and the float32 models'
logits, which take the family's route, to exact equality."""
import ctypes as C
import functools
import os
import re

import pytest
import torch

from attn_decode_cases import eager, oracle, parse_describe, restated
from attn_entry_cases import DECODE_PTRS, DECODE_STRIDES, decode_call
from kernel_resources import resources
from test_rope_cpu import module_dicts

from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import (fused_attention, install_fused_attention, install_fused_rope, uninstall_fused_attention,
                                        uninstall_fused_rope)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("llama", "mistral", "qwen2")
TOL = 2e-2


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        pytest.skip("library not built")
    return _lib.load()


def fake_op(monkeypatch):
    """`ops.attn_decode` replaced by the counting restatement, and the core without its device test."""
    calls = {"attn": 0, "lengths": []}

    def attn_decode(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None, *, out=None, plan=None):
        calls["attn"] += 1
        calls["lengths"].append(int(length))
        assert out is None and plan == ops.attn_decode_plan(q, k_cache, v_cache, length, k_new, v_new, mask)
        return restated(q, k_cache, v_cache, length, k_new, v_new, mask, scaling)

    monkeypatch.setattr(fused_attention.ops, "attn_decode", attn_decode)
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    return calls


# ---- symbols, validation, pure functions, resources ------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read(), flags=re.S)
    for name in ("qllm_attn_decode", "qllm_attn_decode_workspace_bytes", "qllm_attn_decode_describe"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTS and C.cast(getattr(lib, name), C.c_void_p).value, name
    assert len(lib.qllm_attn_decode.argtypes) == 31 and lib.qllm_attn_decode.argtypes[14:23] == [C.c_int64] * 9
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert all(hasattr(ops, n) for n in ("attn_decode", "attn_decode_plan", "attn_decode_describe"))
    assert "attn_decode.hip" in open(os.path.join(ROOT, "qllm_amd", "csrc", "Makefile")).read()


def test_every_argument_check_fires_before_any_device_work(lib):
    INV, UNS, WS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_WORKSPACE
    P, S0 = DECODE_PTRS, DECODE_STRIDES
    call = functools.partial(decode_call, lib)   # no workspace: a call that passes every other check ends at that one, never at a launch

    for name in ("q", "k_cache", "v_cache", "out"):
        assert call(**{name: None}) == INV and "must not be NULL" in _lib.last_error(), name
    for bad in (dict(b=0), dict(b=-1), dict(hq=0), dict(hk=0), dict(d=0), dict(d=-64), dict(max_len=0), dict(max_len=-5)):
        assert call(**bad) == INV and "must be >= 1" in _lib.last_error(), bad
    for hq, hk in ((8, 3), (2, 4), (7, 2)):
        assert call(hq=hq, hk=hk) == INV and "must divide" in _lib.last_error(), (hq, hk)
    for dt in (7, _lib.DT_F32, -1):
        assert call(dt=dt) == INV and "act_dtype" in _lib.last_error(), dt
    for kind in (3, -1):
        assert call(mask_kind=kind) == INV and "mask_kind" in _lib.last_error(), kind
    assert call(mask=None) == INV and "mask must be NULL exactly" in _lib.last_error()
    assert call(mask_kind=_lib.ATTN_MASK_NONE) == INV and "mask must be NULL exactly" in _lib.last_error()
    for bad in (dict(k_new=None), dict(v_new=None)):
        assert call(**bad) == INV and "together" in _lib.last_error(), bad
    for name in ("q", "k_new", "v_new", "k_cache", "v_cache", "out"):
        assert call(**{name: P[name] + 8}) == INV and "16-byte aligned" in _lib.last_error(), name
    assert call(len_dev=P["len_dev"] + 4) == INV and "8-byte aligned" in _lib.last_error()
    assert call(mask=P["mask"] + 1, mask_kind=_lib.ATTN_MASK_ADDITIVE) == INV and "2-byte aligned" in _lib.last_error()
    for i in range(9):
        for v in (4, 12, -8):
            s = list(S0)
            s[i] = v
            assert call(strides=tuple(s)) == INV and "multiples of 8" in _lib.last_error(), (i, v)
    assert call(k_new=None, v_new=None, strides=S0[:2] + (3, -5, 1, 7) + S0[6:]) == WS  # without an append its four strides are not looked at
    # the host length: 0..max_len, one less with an append; on the device it is not looked at
    for bad in (dict(kv_len=-1), dict(kv_len=100), dict(kv_len=101, k_new=None, v_new=None)):
        assert call(**bad) == INV and "0..max_len" in _lib.last_error(), bad
    assert call(kv_len=100, k_new=None, v_new=None) == WS and call(kv_len=99) == WS and call(kv_len=0, k_new=None, v_new=None) == WS
    assert call(kv_len=10 ** 6, len_dev=P["len_dev"]) == WS
    # the mask covers what the call may reach: kv_len, + 1 with an append, max_len with the length on the device
    assert call(kv_len=10, mask_len=10) == INV and "mask must cover 11" in _lib.last_error()
    assert call(kv_len=10, mask_len=11) == WS and call(kv_len=10, mask_len=10, k_new=None, v_new=None) == WS
    assert call(kv_len=10, mask_len=99, len_dev=P["len_dev"]) == INV and "mask must cover 100" in _lib.last_error()
    assert call(mask_batch=-100) == INV and "batch stride" in _lib.last_error()
    # what the kernel is not built for: unsupported, with the value
    for d in (32, 96, 256):
        assert call(d=d) == UNS and "head_dim" in _lib.last_error() and str(d) in _lib.last_error(), d
    assert call(hq=18, hk=2) == UNS and "(got 9)" in _lib.last_error()
    assert call(b=3000, hk=2, hq=2) == UNS and "6000" in _lib.last_error()
    # the workspace: missing, small, misaligned
    need = lib.qllm_attn_decode_workspace_bytes(2, 8, 2, 64, 100)
    assert call() == WS and call(ws=P["ws"], ws_bytes=need - 1) == WS and call(ws=P["ws"] + 8) == WS and str(need) in _lib.last_error()


def test_the_workspace_function_is_pure_and_monotone(lib):
    f = lib.qllm_attn_decode_workspace_bytes
    assert f(1, 32, 8, 128, 4096) == f(1, 32, 8, 128, 4096) > 16384
    for hq, hk, d in ((32, 32, 128), (32, 8, 128), (28, 4, 128), (8, 2, 64)):
        sizes = [f(b, hq, hk, d, 4096) for b in (1, 2, 3, 8, 64)]
        assert sizes == sorted(sizes), sizes
        sizes = [f(2, hq, hk, d, n) for n in (1, 63, 64, 65, 1000, 4096, 65536, 1 << 20)]
        assert sizes == sorted(sizes), sizes
        desc = parse_describe(ops.attn_decode_describe(2, hq, hk, d, 4096))
        assert f(2, hq, hk, d, 4096) >= 16384 + 2 * hk * desc["splits"] * (hq // hk) * (d + 2) * 4         # the page, and (m, l, acc) of every split
    assert f(1, 8, 2, 96, 100) == 16384 and f(0, 8, 2, 64, 100) == 16384 and _lib.last_error() == ""   # refused shapes: the counter page


def test_describe_is_pure_and_the_launch_does_not_depend_on_the_length(lib):
    a = ops.attn_decode_describe(1, 32, 8, 128, 4096)
    assert a == ops.attn_decode_describe(1, 32, 8, 128, 4096) and a.startswith("attn_decode tile=64 ")
    g = parse_describe(a)
    assert g["group"] == 4 and g["chunk"] % g["tile"] == 0 and (g["splits"] - 1) * g["chunk"] < 4096 <= g["splits"] * g["chunk"]
    assert parse_describe(ops.attn_decode_describe(1, 8, 2, 64, 4096))["tile"] == 128
    assert "kv_len" not in a                                                                # the entry takes no length: nothing to depend on
    assert parse_describe(ops.attn_decode_describe(1, 1, 1, 128, 1 << 20))["splits"] == 32   # kAttnDecodeMaxSplits
    assert parse_describe(ops.attn_decode_describe(64, 32, 32, 128, 4096))["splits"] == 1
    assert parse_describe(ops.attn_decode_describe(1, 32, 32, 128, 1))["splits"] == 1
    assert ops.attn_decode_describe(1, 32, 8, 96, 4096).startswith("refused: ") and "96" in ops.attn_decode_describe(1, 32, 8, 96, 4096)
    with pytest.raises(_lib.QllmError):
        ops.attn_decode_describe(1, 32, 5, 128, 4096)


def test_the_split_rule_two_blocks_per_compute_unit(lib):
    """splits = ceil(2 CU / (batch x kv heads)), at most 32 and at most one per tile; chunk = the tiles dealt evenly; the splits that hold
    a position.  So batch x kv heads x splits <= 2 CU + batch x kv heads wherever more than one split runs -- what the workspace bound
    relies on -- and the workspace holds (m, l, two pads, acc[D]) of every query head of every split.  256 compute units: the MI355X, and
    what the library plans with when it reaches no device."""
    cus = 256
    for b in (1, 2, 3, 5, 8, 17, 64, 128):
        for hq, hk in ((1, 1), (4, 4), (8, 2), (28, 4), (32, 8), (32, 32)):
            for d, tile in ((64, 128), (128, 64)):
                for n in (1, tile, tile + 1, 1000, 1027, 2051, 4096, 65536, 1 << 20):
                    g = parse_describe(ops.attn_decode_describe(b, hq, hk, d, n))
                    bh, tiles = b * hk, -(-n // tile)
                    want = max(1, min(-(-2 * cus // bh), 32, tiles))
                    chunk = -(-tiles // want) * tile
                    assert (g["tile"], g["chunk"], g["splits"]) == (tile, chunk, -(-n // chunk)), (b, hq, hk, d, n, g)
                    assert g["splits"] <= want <= 32 and (g["splits"] == 1 or bh * g["splits"] <= 2 * cus + bh), (b, hq, hk, d, n, g)
                    if want == -(-2 * cus // bh) and tiles % want == 0:                       # neither cap binds, the tiles deal evenly:
                        assert 2 * cus <= bh * g["splits"]                                    # two blocks per compute unit, rounded up
                    need = lib.qllm_attn_decode_workspace_bytes(b, hq, hk, d, n)
                    assert need >= 16384 + bh * g["splits"] * (hq // hk) * (d + 4) * 4, (b, hq, hk, d, n, g, need)


def test_the_kernels_use_no_scratch_and_spill_nothing():
    res = resources("attn_decode.hip")
    assert len(res) == 32, sorted(res)                                                      # 2 types x 2 head sizes x 8 group sizes
    for n, r in res.items():
        assert "attn_decode_kernel" in n
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)
        assert 0 < r["group_segment_fixed_size"] <= 4 * 8 * 130 * 4 + 4, (n, r)


# ---- the plan --------------------------------------------------------------------------------------------------------------------------------
def tensors(b=2, hq=8, hk=2, d=64, L=40, dtype=torch.float16):
    g = torch.Generator().manual_seed(1)
    q = torch.randn(b, 1, hq, d, generator=g).to(dtype).transpose(1, 2)
    return q, torch.randn(b, hk, L, d, generator=g).to(dtype), torch.randn(b, hk, L, d, generator=g).to(dtype)


def test_plan_derives_sizes_and_strides():
    q, k, v = tensors()
    assert ops.attn_decode_plan(q, k, v, 7) == (2, 8, 2, 64, 40, 512, 64, 0, 0, 0, 0, 2 * 40 * 64, 40 * 64, 64, 0, 0, 0)
    assert ops.attn_decode_plan(q.transpose(1, 2), k, v, 40)[:7] == (2, 8, 2, 64, 40, 512, 64)                 # [B, 1, Hq, D]
    buf = torch.zeros(2, 1, (8 + 4) * 64, dtype=torch.float16)                                                # slices of one q/k/v row
    qs = buf[..., :512].view(2, 1, 8, 64).transpose(1, 2)
    ks, vs = buf[..., 512:640].view(2, 1, 2, 64).transpose(1, 2), buf[..., 640:].view(2, 1, 2, 64).transpose(1, 2)
    assert ops.attn_decode_plan(qs, k, v, 39, ks, vs)[5:11] == (768, 64, 768, 64, 768, 64)
    mb = torch.ones(2, 1, 1, 40, dtype=torch.bool)
    assert ops.attn_decode_plan(q, k, v, 40, mask=mb)[14:] == (_lib.ATTN_MASK_BOOL, 40, 40)
    assert ops.attn_decode_plan(q, k, v, 9, mask=mb[..., :9])[14:] == (_lib.ATTN_MASK_BOOL, 9, 40)             # a view of a longer row
    assert ops.attn_decode_plan(q, k, v, 9, mask=torch.zeros(2, 40, dtype=torch.float16))[14:] == (_lib.ATTN_MASK_ADDITIVE, 40, 40)
    assert ops.attn_decode_plan(q, k, v, 9, mask=mb[:1])[14:] == (_lib.ATTN_MASK_BOOL, 40, 0)                  # one row for the batch
    assert ops.attn_decode_plan(q, k, v, torch.tensor(5), mask=mb)[4] == 40                                   # the length on the device
    q1, k1, v1 = tensors(b=1, hq=28, hk=4, d=128, dtype=torch.bfloat16)
    assert ops.attn_decode_plan(q1, k1, v1, 0)[:7] == (1, 28, 4, 128, 40, 28 * 128, 128)


def test_plan_refuses_what_the_entry_does_not_serve():
    q, k, v = tensors()
    mb = torch.ones(2, 1, 1, 40, dtype=torch.bool)

    def refused(*a, **kw):
        with pytest.raises(ops.QllmUnsupported):
            ops.attn_decode_plan(*a, **kw)
        return True

    assert refused(q.float(), k.float(), v.float(), 7)                                       # fp32
    assert refused(q, k.bfloat16(), v, 7) and refused(q, k, v, 7, q[:, :2], None)            # mixed types; k_new alone
    assert refused(torch.cat((q, q), 2), k, v, 7)                                            # two query tokens
    assert refused(q[0], k, v, 7) and refused(q, k[0], v[0], 7)                              # not 4-D
    assert refused(q, k, v[:, :, :39], 7) and refused(q, k, v.transpose(1, 2).contiguous().transpose(1, 2), 7)   # caches of two shapes / layouts
    assert refused(q[:1], k, v, 7)                                                           # another batch
    assert refused(*tensors(hq=8, hk=3), 7) and refused(*tensors(hq=18, hk=2), 7)            # heads that do not divide; a group of 9
    assert refused(*tensors(d=32), 7) and refused(*tensors(d=96), 7) and refused(*tensors(d=256), 7)
    assert refused(q, k.transpose(2, 3).contiguous().transpose(2, 3), v.transpose(2, 3).contiguous().transpose(2, 3), 7)   # D not contiguous
    assert refused(q, k, v, -1) and refused(q, k, v, 41) and refused(q, k, v, 40, q[:, :2], q[:, 2:4])                     # the length
    assert refused(q, k, v, torch.tensor(5, dtype=torch.int32)) and refused(q, k, v, torch.tensor([5]))                   # a device length of another kind
    assert refused(q, k, v, 7, q[:, :4], q[:, 4:])                                           # k_new with four heads
    assert refused(q, k, v, 10, mask=mb[..., :9]) and refused(q, k, v, torch.tensor(5), mask=mb[..., :39])                 # a short mask
    assert refused(q, k, v, 7, mask=mb.float()) and refused(q, k, v, 7, mask=torch.ones(3, 1, 1, 40, dtype=torch.bool))    # fp32 mask; three rows
    assert refused(q, k, v, 7, mask=torch.ones(2, 1, 2, 40, dtype=torch.bool))                                            # a row per query token
    odd = torch.zeros(2 * 8 * 64 + 4, dtype=torch.float16)[4:].view(2, 1, 8, 64).transpose(1, 2)
    assert refused(odd, k, v, 7)                                                             # q off 16 bytes


def test_the_restatement_is_attention():
    q, k, v = tensors(b=2, hq=8, hk=2, d=64, L=40)
    ref = oracle(q[:, :, 0], k, v, 17, 0.125)
    assert (restated(q, k, v, 17).double() - ref).abs().max() <= (eager(q[:, :, 0], k, v, 17, 0.125).double() - ref).abs().max()
    kn, vn = torch.randn(2, 2, 1, 64).half(), torch.randn(2, 2, 1, 64).half()
    k2, v2 = k.clone(), v.clone()
    out = restated(q, k2, v2, 17, kn, vn)
    assert torch.equal(k2[:, :, 17], kn[:, :, 0]) and torch.equal(v2[:, :, 17], vn[:, :, 0]) and torch.equal(k2[:, :, :17], k[:, :, :17])
    assert torch.equal(out, restated(q, k2, v2, 18))


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------
def tiny_model(family, attn="sdpa", dtype=torch.float16, device="cpu", **extra):
    """hidden 256, 4 heads of 64, 2 kv heads, 2 layers."""
    import transformers
    kw = dict(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, vocab_size=64,
              max_position_embeddings=64, tie_word_embeddings=False)
    cfg_cls, cls = {"llama": (transformers.LlamaConfig, transformers.LlamaForCausalLM), "mistral": (transformers.MistralConfig, transformers.MistralForCausalLM),
                    "qwen2": (transformers.Qwen2Config, transformers.Qwen2ForCausalLM)}[family]
    if family == "mistral":
        kw["sliding_window"] = None
    cfg = cfg_cls(**dict(kw, **extra))
    cfg._attn_implementation = attn
    torch.manual_seed(11)
    return cls(cfg).to(dtype).to(device).eval()


def make_cache(model, kind, device="cpu"):
    from transformers import DynamicCache, StaticCache
    return DynamicCache(config=model.config) if kind == "dynamic" else StaticCache(config=model.config, max_cache_len=16)


def prefill_and_decode(model, kind, device="cpu", batch=1, steps=4, cache=None, **kw):
    """Logits of a 5-token prefill and `steps` single-token decode steps through a DynamicCache or a StaticCache, and the cache."""
    ids = torch.randint(0, 64, (batch, 5 + steps), generator=torch.Generator().manual_seed(3)).to(device)
    cache = make_cache(model, kind, device) if cache is None else cache
    outs = []
    with torch.no_grad():
        outs.append(model(ids[:, :5], past_key_values=cache, use_cache=True, **kw).logits)
        for i in range(5, 5 + steps):
            outs.append(model(ids[:, i:i + 1], past_key_values=cache, use_cache=True, **kw).logits)
    return outs, cache


def close(got, want, tol=TOL):
    return all(g.shape == w.shape and bool(torch.isfinite(g.float()).all()) and (g.float() - w.float()).abs().max().item() <= tol for g, w in zip(got, want))


@pytest.mark.parametrize("kind", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("family", FAMILIES)
def test_tiny_models_decode_through_the_op_and_prefill_through_the_family_route(family, attn, kind, monkeypatch):
    model = tiny_model(family, attn)
    before = module_dicts(model)
    want, want_cache = prefill_and_decode(model, kind, batch=2)
    assert max(w.float().abs().max().item() for w in want) < 2
    calls = fake_op(monkeypatch)
    assert install_fused_attention(model) == 2 and install_fused_attention(model) == 0
    got, got_cache = prefill_and_decode(model, kind, batch=2)
    assert calls["attn"] == 2 * 4 and calls["lengths"] == [6, 6, 7, 7, 8, 8, 9, 9]                # never at the prefill; the valid keys
    assert close(got, want) and torch.equal(got[0], want[0])                                      # the prefill is the family's own
    if kind == "static":
        for a, b in zip(got_cache.layers, want_cache.layers):
            assert int(a.cumulative_length) == int(b.cumulative_length) == 9
            assert torch.equal(a.keys[:, :, 9:], b.keys[:, :, 9:]) and torch.equal(a.values[:, :, 9:], b.values[:, :, 9:])
            assert (a.keys.float() - b.keys.float()).abs().max() <= TOL and (a.values.float() - b.values.float()).abs().max() <= TOL
        assert torch.equal(got_cache.layers[0].keys, want_cache.layers[0].keys)                   # the first layer sees the same inputs
    assert uninstall_fused_attention(model) == 2 and uninstall_fused_attention(model) == 0
    assert module_dicts(model) == before
    again, _ = prefill_and_decode(model, kind, batch=2)
    assert calls["attn"] == 2 * 4 and all(torch.equal(a, w) for a, w in zip(again, want))


def test_a_left_padded_batch_goes_through_the_op_with_the_mask(monkeypatch):
    model = tiny_model("llama", "sdpa")
    ids = torch.randint(0, 64, (2, 7), generator=torch.Generator().manual_seed(5))
    mask = torch.ones(2, 7, dtype=torch.long)
    mask[1, :2] = 0

    def run():
        from transformers import DynamicCache
        cache, outs = DynamicCache(config=model.config), []
        with torch.no_grad():
            outs.append(model(ids[:, :5], attention_mask=mask[:, :5], past_key_values=cache, use_cache=True).logits)
            for i in (5, 6):
                outs.append(model(ids[:, i:i + 1], attention_mask=mask[:, :i + 1], past_key_values=cache, use_cache=True).logits)
        return outs

    want = run()
    calls = fake_op(monkeypatch)
    seen = []
    plan = ops.attn_decode_plan
    monkeypatch.setattr(fused_attention.ops, "attn_decode_plan", lambda *a, **kw: ("mask" in kw and seen.append(kw["mask"])) or plan(*a, **kw))   # (the core names the mask)
    assert install_fused_attention(model) == 2
    got = run()
    assert calls["attn"] == 2 * 2 and close(got, want)
    assert len(seen) == 4 and all(m is not None and m.shape[1:3] == (1, 1) for m in seen)


def test_each_fallback_condition_takes_the_family_route(monkeypatch):
    from transformers import DynamicCache
    calls = fake_op(monkeypatch)

    def zero_calls(model, kind="dynamic", exact=True, **kw):
        want, _ = prefill_and_decode(model, kind, **kw)
        n = install_fused_attention(model)
        got, _ = prefill_and_decode(model, kind, **kw)
        assert uninstall_fused_attention(model) == n
        assert calls["attn"] == 0 and (not exact or all(torch.equal(g, w) for g, w in zip(got, want)))
        return n

    assert zero_calls(tiny_model("llama", dtype=torch.float32)) == 2                             # fp32
    assert zero_calls(tiny_model("llama", num_attention_heads=8, num_key_value_heads=8)) == 2    # head_dim 32: the plan refuses
    model = tiny_model("llama")
    model.config._attn_implementation = "flex_attention"
    attn = model.model.layers[0].self_attn
    q = torch.randn(1, 4, 1, 64).half()
    k = torch.randn(1, 2, 1, 64).half()
    cache = DynamicCache(config=model.config)
    cache.update(torch.randn(1, 2, 3, 64).half(), torch.randn(1, 2, 3, 64).half(), 0)

    def core(mod=attn, q=q, k=k, mask=None, cache=cache, window=None, **kwargs):
        n = int(cache.get_seq_length(0)) if cache is not None else 0
        out = fused_attention._fused_core(mod, q, k, k.clone(), mask, cache, kwargs, window)
        assert (out[0] is None) == (not out[3]) and (cache is None or int(cache.get_seq_length(0)) == n + (q.shape[2] if out[3] else 0))
        return out[0] is not None

    assert not core()                                                                            # flex_attention
    model.config._attn_implementation = "sdpa"
    assert core() and calls["attn"] == 1
    assert core(position_ids=torch.zeros(1, 1), use_cache=True, output_attentions=False, softcap=None)
    assert not core(q=torch.cat((q, q), 2), k=torch.cat((k, k), 2))                              # two query tokens
    assert not core(cache=None)
    assert not core(q=q.float()) and not core(k=k.bfloat16())
    assert not core(output_attentions=True) and not core(softcap=30.0) and not core(s_aux=torch.zeros(4)) and not core(sliding_window=8)
    assert not core(mask=torch.ones(1, 1, 2, 9, dtype=torch.bool)) and not core(mask=torch.zeros(1, 1, 1, 9)) and not core(mask=torch.ones(1, 9, dtype=torch.bool))
    assert core(mask=torch.ones(1, 1, 1, cache.get_seq_length(0) + 1, dtype=torch.bool))
    attn.train()
    assert not core()
    attn.eval()
    with torch.enable_grad():
        assert not core(q=q.clone().requires_grad_())
    mistral = tiny_model("mistral", sliding_window=8)
    assert not core(mod=mistral.model.layers[0].self_attn, window="config")                      # a sliding window reaches the call
    attn.sliding_window = 8
    assert not core(window="self")
    del attn.sliding_window

    class Other(type(cache.layers[0])):
        pass
    cache.layers[0].__class__ = Other                                                            # not EXACTLY a DynamicLayer
    assert not core()
    cache.layers[0].__class__ = Other.__bases__[0]
    cache.offloading = True
    assert not core()
    cache.offloading = False
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: all(t.is_cuda for t in ts))
    assert not core()                                                                            # CPU tensors
    from transformers import StaticCache
    static = StaticCache(config=model.config, max_cache_len=16)
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    assert not core(cache=static)                                                                # a static layer that is not initialised
    before = calls["attn"]
    static.update(torch.randn(1, 2, 3, 64).half(), torch.randn(1, 2, 3, 64).half(), 0)
    assert core(cache=static) and calls["attn"] == before + 1 and calls["lengths"][-1] == 4


@pytest.mark.parametrize("order", ["rope first", "attention first"])
def test_install_and_uninstall_compose_with_fused_rope_in_both_orders(order, monkeypatch):
    from test_rope_cpu import fake_op as fake_rope
    model = tiny_model("llama")
    before = module_dicts(model)
    want, _ = prefill_and_decode(model, "static")
    calls, rope_calls = fake_op(monkeypatch), fake_rope(monkeypatch)
    first, second = (install_fused_rope, install_fused_attention) if order == "rope first" else (install_fused_attention, install_fused_rope)
    assert first(model) == 2 and second(model) == 2 and first(model) == 0 and second(model) == 0
    got, _ = prefill_and_decode(model, "static")
    assert calls["attn"] == 2 * 4 and rope_calls["rope"] == 2 * 5 and close(got, want)
    undo = (uninstall_fused_rope, uninstall_fused_attention)
    for a, b in (undo, undo[::-1]):
        assert a(model) == 2 and "forward" in model.model.layers[0].self_attn.__dict__          # the other install still works
        n_attn, n_rope = calls["attn"], rope_calls["rope"]
        got, _ = prefill_and_decode(model, "static")
        assert close(got, want) and (calls["attn"] - n_attn, rope_calls["rope"] - n_rope) == ((0, 10) if a is uninstall_fused_attention else (8, 0))
        assert b(model) == 2 and module_dicts(model) == before
        assert first(model) == 2 and second(model) == 2
    assert uninstall_fused_attention(model) == 2 and uninstall_fused_rope(model) == 2 and module_dicts(model) == before


def test_install_leaves_foreign_signatures_and_other_classes_alone():
    from transformers.models.llama import modeling_llama as ML
    model = tiny_model("llama")

    def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, cache_position=None, **kwargs):
        return ML.LlamaAttention.forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)

    model.model.layers[0].self_attn.__class__ = type("LlamaAttention", (ML.LlamaAttention,), {"forward": forward})
    model.model.layers[1].self_attn.__class__ = type("OtherAttention", (ML.LlamaAttention,), {})
    before = module_dicts(model)
    assert install_fused_attention(model) == 0 and module_dicts(model) == before
    model = tiny_model("llama")
    assert install_fused_attention(model, ["MistralAttention"]) == 0 and install_fused_attention(model, [ML.LlamaAttention]) == 2


def test_the_environment_switch_and_the_loader_default(monkeypatch):
    import inspect
    from qllm_amd.modeling import base
    monkeypatch.setenv("QLLM_FUSE_ATTENTION", "0")
    model = tiny_model("llama")
    assert install_fused_attention(model) == 0 and not any("forward" in m.__dict__ for m in model.modules())
    assert inspect.signature(base.load_quantized).parameters["fuse_attention"].default is False
