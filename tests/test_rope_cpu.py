"""The rotary embedding of q and k as one kernel (qllm_rope, csrc/rope.hip; ops.rope; q_layers/fused_rope.py) without a GPU: the additive C
symbol (exported, declared, bound; ABI still 7), every argument check of the entry on fake, aligned, never-dereferenced pointers, the
compiler's resource report (no scratch, no LDS), what ops.rope_plan derives and refuses, each fallback of `apply_rotary` and the installed
attention forward on tiny random Llama / Mistral / Qwen2 models against a counting torch restatement of the kernel's three-rounding formula
in the place of `ops.rope`: bit for bit the unpatched model's logits, one call per layer and forward."""
import ctypes as C
import os
import re

import pytest
import torch

from kernel_resources import resources
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_rope, install_fused_rope, uninstall_fused_rope

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ("llama", "mistral", "qwen2")


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def eager_rope(q, k, cos, sin, unsqueeze_dim=1):
    """transformers' apply_rotary_pos_emb (modeling_llama; Mistral's and Qwen2's are the same text), expression for expression."""
    def rotate_half(x):
        x1 = x[..., : x.shape[-1] // 2]
        x2 = x[..., x.shape[-1] // 2:]
        return torch.cat((-x2, x1), dim=-1)
    cos = cos.unsqueeze(unsqueeze_dim)
    sin = sin.unsqueeze(unsqueeze_dim)
    q_embed = (q * cos) + (rotate_half(q) * sin)
    k_embed = (k * cos) + (rotate_half(k) * sin) if k is not None else None
    return q_embed, k_embed


def three_roundings(q, k, cos, sin, unsqueeze_dim=1):
    """The kernel's formula in torch: a = round(x * c), b = round(r * s), out = round(float(a) + float(b)), in the layout eager returns."""
    c, s = cos.unsqueeze(unsqueeze_dim).float(), sin.unsqueeze(unsqueeze_dim).float()

    def one(x):
        if x is None:
            return None
        half = x.shape[-1] // 2
        r = torch.cat((-x[..., half:], x[..., :half]), dim=-1)
        a, b = (x.float() * c).to(x.dtype), (r.float() * s).to(x.dtype)
        out = torch.empty_like(x)
        out.copy_((a.float() + b.float()).to(x.dtype))
        return out
    return one(q), one(k)


def fake_op(monkeypatch):
    """`ops.rope` replaced by a counting `three_roundings`, and `_kernel_applies` without its device test."""
    calls = {"rope": 0}

    def rope(q, k, cos, sin, unsqueeze_dim=1, *, out=None, plan=None):
        calls["rope"] += 1
        assert out is None and plan == ops.rope_plan(q, k, cos, sin, unsqueeze_dim)
        return three_roundings(q, k, cos, sin, unsqueeze_dim)

    monkeypatch.setattr(fused_rope.ops, "rope", rope)
    monkeypatch.setattr(fused_rope, "_kernel_applies", fused_rope._shape_applies)
    return calls


def qkcs(b=1, s=3, hq=4, hk=2, d=16, dtype=torch.float16, seed=0, cos_batch=None):
    """q, k as the attention forward makes them ([B, H, S, D] views of [B, S, H, D] memory) and cos, sin [B, S, D] of real angles."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(b, s, hq, d, generator=g).to(dtype).transpose(1, 2)
    k = torch.randn(b, s, hk, d, generator=g).to(dtype).transpose(1, 2)
    ang = torch.rand(b if cos_batch is None else cos_batch, s, d // 2, generator=g) * 6.28
    ang = torch.cat((ang, ang), -1)
    return q, k, ang.cos().to(dtype), ang.sin().to(dtype)


# ---- symbols, validation, resources --------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read(), flags=re.S)
    assert re.search(r"\bqllm_rope\s*\(", header)
    assert "qllm_rope" in _lib.EXPORTS
    assert C.cast(lib.qllm_rope, C.c_void_p).value
    assert len(lib.qllm_rope.argtypes) == 17 and lib.qllm_rope.argtypes[10:14] == [C.c_int64] * 4
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert all(hasattr(ops, n) for n in ("rope", "rope_plan"))
    assert "rope.hip" in open(os.path.join(ROOT, "qllm_amd", "csrc", "Makefile")).read()


def test_every_argument_check_fires_before_any_device_work(lib):
    INV, UNS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED
    P = {n: 4096 * (i + 1) for i, n in enumerate(("q", "k", "cos", "sin", "q_out", "k_out"))}

    def call(rows=3, hq=4, hk=2, d=64, strides=(384, 64, 128, 64), cos_rows=3, dt=_lib.DT_F16, **ptrs):
        p = dict(P, **ptrs)
        return lib.qllm_rope(p["q"], p["k"], p["cos"], p["sin"], p["q_out"], p["k_out"], rows, hq, hk, d, *strides, cos_rows, dt, None)

    for name in ("q", "cos", "sin", "q_out"):
        assert call(**{name: None}) == INV and "must not be NULL" in _lib.last_error(), name
    for bad in (dict(k=None), dict(k_out=None), dict(hk=0), dict(hk=0, k=None), dict(hk=0, k_out=None), dict(hk=-1)):
        assert call(**bad) == INV and "k_heads" in _lib.last_error(), bad
    for bad in (dict(rows=0), dict(rows=-3), dict(hq=0), dict(d=0), dict(d=-16)):
        assert call(**bad) == INV and "must be >= 1" in _lib.last_error(), bad
    assert call(dt=7) == INV and "act_dtype" in _lib.last_error()
    assert call(dt=_lib.DT_F32) == INV and "act_dtype" in _lib.last_error()
    for bad in (0, -1, 2, 6):
        assert call(cos_rows=bad) == INV and "divide rows" in _lib.last_error(), bad
    for name in P:
        assert call(**{name: P[name] + 8}) == INV and "16-byte aligned" in _lib.last_error(), name
    for i in range(4):
        for v in (4, 12, -8):
            s = [384, 64, 128, 64]
            s[i] = v
            assert call(strides=tuple(s)) == INV and "multiples of 8" in _lib.last_error(), (i, v)
    # an output that is its input, with another layout
    assert call(q_out=P["q"]) == INV and "may be its input" in _lib.last_error()          # q's row stride 384 is not 4 * 64
    assert call(k_out=P["k"], strides=(256, 64, 128, 128)) == INV and "may be its input" in _lib.last_error()
    # the head_dim rules: refused as unsupported, with the text; k's strides are not looked at without k
    for d in (8, 24, 72, 272, 512):
        assert call(d=d) == UNS and "head_dim" in _lib.last_error() and str(d) in _lib.last_error(), d
    assert call(d=24, hk=0, k=None, k_out=None, strides=(384, 64, 3, -5)) == UNS
    assert call(d=24, q_out=P["q"], strides=(96, 24, 128, 64)) == UNS                      # (in place with contiguous strides passes that check)


def test_the_kernels_use_no_scratch_and_no_lds():
    res = resources("rope.hip")
    assert len(res) == 2, sorted(res)                                                       # fp16 and bf16
    for n, r in res.items():
        assert "rope_kernel" in n
        assert r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (n, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)


# ---- the formula and the plan --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_three_roundings_are_the_eager_expression_and_transformers_function(dtype):
    from transformers.models.llama.modeling_llama import apply_rotary_pos_emb
    for ud in (1, 2):
        q, k, cos, sin = qkcs(2, 5, 4, 2, 32, dtype, seed=ud)
        if ud == 2:
            q, k = q.transpose(1, 2), k.transpose(1, 2)
        want = eager_rope(q, k, cos, sin, ud)
        theirs = apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=ud)
        got = three_roundings(q, k, cos, sin, ud)
        for w, t, g in zip(want, theirs, got):
            assert not bool(torch.isnan(w.float()).any())
            assert torch.equal(w, t) and torch.equal(w, g) and g.stride() == w.stride()


def test_plan_derives_rows_heads_and_strides():
    q, k, cos, sin = qkcs(2, 3, 4, 2, 32)
    assert q.stride() == (3 * 4 * 32, 32, 4 * 32, 1)
    assert ops.rope_plan(q, k, cos, sin) == (6, 4, 2, 32, 128, 32, 64, 32, 6)
    assert ops.rope_plan(q, k, cos[:1], sin[:1]) == (6, 4, 2, 32, 128, 32, 64, 32, 3)         # one table broadcast over the batch
    assert ops.rope_plan(q.transpose(1, 2), k.transpose(1, 2), cos, sin, 2) == (6, 4, 2, 32, 128, 32, 64, 32, 6)
    assert ops.rope_plan(q, None, cos, sin) == (6, 4, 0, 32, 128, 32, 0, 0, 6)
    # q and k as slices of one [rows, (Hq + 2 Hk) D] buffer
    buf = torch.zeros(2, 3, (4 + 2 * 2) * 32, dtype=torch.float16)
    qs, ks = buf[..., :128].view(2, 3, 4, 32), buf[..., 128:192].view(2, 3, 2, 32)
    assert ops.rope_plan(qs, ks, cos, sin, 2) == (6, 4, 2, 32, 256, 32, 256, 32, 6)
    assert ops.rope_plan(qs.transpose(1, 2), ks.transpose(1, 2), cos, sin, 1) == (6, 4, 2, 32, 256, 32, 256, 32, 6)
    # one token: the strides of dimensions of size one are not looked at
    q1, k1, c1, s1 = qkcs(1, 1, 4, 2, 32)
    assert ops.rope_plan(q1, k1, c1, s1) == (1, 4, 2, 32, 128, 32, 64, 32, 1)
    assert ops.rope_plan(q1.contiguous(), k1.contiguous(), c1, s1) == (1, 4, 2, 32, 128, 32, 64, 32, 1)


def test_plan_refuses_what_the_entry_does_not_serve():
    q, k, cos, sin = qkcs(2, 3, 4, 2, 32)

    def refused(*a, match):
        with pytest.raises(ops.QllmUnsupported, match=match):
            ops.rope_plan(*a)
    refused(q, k, cos.float(), sin.float(), match="one type")
    refused(q.float(), k.float(), cos.float(), sin.float(), match="one type")
    refused(q, k.bfloat16(), cos, sin, match="one type")
    refused(q, k, cos, sin, 0, match="unsqueeze_dim")
    refused(q[0], k[0], cos, sin, match="4-D")
    refused(q, k[:, :, :2], cos, sin, match="4-D")
    refused(q.contiguous(), k.contiguous(), cos, sin, match="one stride")                     # really [B, H, S, D] in memory
    refused(q[:1].contiguous(), k[:1].contiguous(), cos[:1], sin[:1], match="token-major")    # ... and at batch 1
    refused(q, k, cos[..., :16], sin[..., :16], match="cos and sin")                          # partial rotary
    refused(q, k, cos.transpose(0, 1).contiguous().transpose(0, 1), sin, match="contiguous")
    refused(q, k, cos, sin[:, :2], match="cos and sin")
    for d in (8, 24, 272):
        qq, kk, cc, ss = qkcs(1, 2, 2, 2, d)
        refused(qq, kk, cc, ss, match="head_dim")
    wide = torch.zeros(2 * 3 * 4 * 32 + 8, dtype=torch.float16)
    refused(wide[4:-4].view(2, 3, 4, 32).transpose(1, 2), k, cos, sin, match="16-byte")       # a misaligned view
    refused(torch.zeros(2, 3, 4, 36, dtype=torch.float16)[..., :32].transpose(1, 2), k, cos, sin, match="multiples of 8")
    refused(torch.zeros(2, 5, 4, 32, dtype=torch.float16)[:, :3].transpose(1, 2), k, cos, sin, match="one stride")
    with pytest.raises(RuntimeError, match="HIP/CUDA"):                                       # a served plan, but no CPU forward path
        ops.rope(q, k, cos, sin)


# ---- apply_rotary ---------------------------------------------------------------------------------------------------------------------------
def test_apply_rotary_falls_back_to_the_eager_function_condition_by_condition(monkeypatch):
    q, k, cos, sin = qkcs(2, 3, 4, 2, 32)
    seen = []

    def eager(*a):
        seen.append(a)
        return eager_rope(*a)

    def run(*a):
        n, m = calls["rope"], len(seen)
        out = fused_rope.apply_rotary(eager, *a)
        want = eager_rope(*a)
        assert all(torch.equal(o, w) and o.stride() == w.stride() and o.dtype == w.dtype for o, w in zip(out, want))
        return calls["rope"] - n, len(seen) - m

    # on the CPU, with the real device test: the eager function, and ops.rope is not asked
    calls = {"rope": 0}
    monkeypatch.setattr(fused_rope.ops, "rope", lambda *a, **kw: pytest.fail("ops.rope called for CPU tensors"))
    assert run(q, k, cos, sin) == (0, 1)
    calls = fake_op(monkeypatch)
    assert run(q, k, cos, sin) == (1, 0)                                                      # the kernel's place
    assert run(q.transpose(1, 2), k.transpose(1, 2), cos, sin, 2) == (1, 0)
    assert run(q.bfloat16(), k.bfloat16(), cos.bfloat16(), sin.bfloat16()) == (1, 0)
    assert run(q, k, cos.float(), sin.float()) == (0, 1)                                      # fp32 cos / sin
    assert run(q.float(), k.float(), cos.float(), sin.float()) == (0, 1)                      # an fp32 model
    assert run(q, k.bfloat16(), cos, sin) == (0, 1)                                           # mixed types
    assert run(*qkcs(1, 2, 2, 2, 24)) == (0, 1) and run(*qkcs(1, 2, 2, 2, 272)) == (0, 1)     # odd head sizes
    assert run(q.contiguous(), k.contiguous(), cos, sin) == (0, 1)                            # head-major memory
    pq, pk = torch.cat((q, q), -1), torch.cat((k, k), -1)                                     # partial rotary: cos narrower than the head
    n, m = calls["rope"], len(seen)
    with pytest.raises(RuntimeError):                                                        # (eager cannot broadcast it either: it is asked, not the op)
        fused_rope.apply_rotary(eager, pq, pk, cos, sin)
    assert (calls["rope"] - n, len(seen) - m) == (0, 1)
    qg = q.clone().requires_grad_()
    assert run(qg, k, cos, sin) == (0, 1)                                                     # an autograd graph is being recorded
    with torch.no_grad():
        assert run(qg, k, cos, sin) == (1, 0)                                                 # ... not under no_grad


# ---- tiny random models --------------------------------------------------------------------------------------------------------------------
def tiny_model(family, heads, kv_heads, attn, dtype=torch.float16, device="cpu"):
    import transformers
    kw = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=heads, num_key_value_heads=kv_heads, vocab_size=64,
              max_position_embeddings=64, tie_word_embeddings=False)
    cfg_cls, cls = {"llama": (transformers.LlamaConfig, transformers.LlamaForCausalLM), "mistral": (transformers.MistralConfig, transformers.MistralForCausalLM),
                    "qwen2": (transformers.Qwen2Config, transformers.Qwen2ForCausalLM)}[family]
    cfg = cfg_cls(**kw)
    cfg._attn_implementation = attn
    torch.manual_seed(heads * 10 + kv_heads)
    return cls(cfg).to(dtype).to(device).eval()


def prefill_and_decode(model, device="cpu"):
    """Logits of a 5-token prefill and 4 single-token decode steps through a DynamicCache."""
    from transformers import DynamicCache
    ids = torch.randint(0, 64, (1, 9), generator=torch.Generator().manual_seed(3)).to(device)
    cache = DynamicCache(config=model.config)
    outs = []
    with torch.no_grad():
        outs.append(model(ids[:, :5], past_key_values=cache, use_cache=True).logits)
        for i in range(5, 9):
            outs.append(model(ids[:, i:i + 1], past_key_values=cache, use_cache=True).logits)
    return outs


def module_dicts(model):
    return {n: {key: id(v) for key, v in m.__dict__.items()} for n, m in model.named_modules()}


@pytest.mark.parametrize("attn", ["eager", "sdpa"])
@pytest.mark.parametrize("heads,kv_heads", [(4, 4), (4, 2)])
@pytest.mark.parametrize("family", FAMILIES)
def test_tiny_models_compute_the_same_logits_with_one_op_call_per_layer_and_forward(family, heads, kv_heads, attn, monkeypatch):
    import sys
    model = tiny_model(family, heads, kv_heads, attn)
    family_module = sys.modules[type(model.model.layers[0].self_attn).__module__]
    eager_fn = family_module.apply_rotary_pos_emb
    before = module_dicts(model)
    want = prefill_and_decode(model)
    assert all(bool(torch.isfinite(w.float()).all()) for w in want)
    calls = fake_op(monkeypatch)
    assert install_fused_rope(model) == 2
    assert install_fused_rope(model) == 0                                                     # already installed
    assert all("forward" in layer.self_attn.__dict__ for layer in model.model.layers)
    assert family_module.apply_rotary_pos_emb is eager_fn                                     # no module global is touched
    got = prefill_and_decode(model)
    assert calls["rope"] == 2 * 5                                                             # once per layer per forward
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    other = tiny_model(family, heads, kv_heads, attn)                                         # another model in the process is not changed
    prefill_and_decode(other)
    assert calls["rope"] == 2 * 5
    assert uninstall_fused_rope(model) == 2 and uninstall_fused_rope(model) == 0
    assert module_dicts(model) == before
    got = prefill_and_decode(model)
    assert calls["rope"] == 2 * 5 and all(torch.equal(g, w) for g, w in zip(got, want))


def test_install_leaves_foreign_signatures_and_other_classes_alone(monkeypatch):
    from transformers.models.llama import modeling_llama as ML
    model = tiny_model("llama", 4, 2, "eager")

    def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, cache_position=None, **kwargs):
        return ML.LlamaAttention.forward(self, hidden_states, position_embeddings, attention_mask, past_key_values, **kwargs)

    foreign = type("LlamaAttention", (ML.LlamaAttention,), {"forward": forward})              # the whitelisted name, another signature
    renamed = type("OtherAttention", (ML.LlamaAttention,), {})                                # the known forward, a name not on the list
    model.model.layers[0].self_attn.__class__ = foreign
    before = module_dicts(model)
    assert install_fused_rope(model) == 1
    assert "forward" not in model.model.layers[0].self_attn.__dict__ and "forward" in model.model.layers[1].self_attn.__dict__
    assert uninstall_fused_rope(model) == 1 and module_dicts(model) == before
    model.model.layers[1].self_attn.__class__ = renamed
    assert install_fused_rope(model) == 0
    model.model.layers[1].self_attn.__class__ = ML.LlamaAttention
    assert install_fused_rope(model, attention_types=["MistralAttention"]) == 0               # narrowed by the caller
    assert install_fused_rope(model, attention_types=[ML.LlamaAttention]) == 1
    # an instance forward that was there before is what uninstall puts back
    assert uninstall_fused_rope(model) == 1
    attn = model.model.layers[1].self_attn
    mine = attn.forward = lambda *a, **kw: ML.LlamaAttention.forward(attn, *a, **kw)
    assert install_fused_rope(model) == 1 and attn.__dict__["forward"] is not mine
    assert uninstall_fused_rope(model) == 1 and attn.__dict__["forward"] is mine


def test_the_environment_switch_makes_install_a_no_op(monkeypatch):
    monkeypatch.setenv("QLLM_FUSE_ROPE", "0")
    model = tiny_model("llama", 4, 4, "eager")
    assert install_fused_rope(model) == 0
    assert not any("forward" in m.__dict__ for m in model.modules())


def test_load_quantized_keeps_the_fusion_opt_in():
    import inspect
    from qllm_amd.modeling import base
    assert inspect.signature(base.load_quantized).parameters["fuse_rope"].default is False
