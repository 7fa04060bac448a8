"""Qwen3's q_norm / k_norm and rotary embedding as one kernel (qllm_rope_qknorm, csrc/rope_qknorm.hip; ops.rope_qknorm;
q_layers/fused_rope.py) without a GPU: the additive C symbol, the entry's own checks on fake, aligned, never-dereferenced pointers, the
compiler's resource report, what ops.rope_qknorm_plan refuses, and the installed forward of a tiny random Qwen3 on CPU tensors, where
every step falls back to the eager modules."""
import re
import sys

import pytest
import torch

from kernel_resources import resources
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_rope, install_fused_rope, uninstall_fused_rope
from test_rope_cpu import ROOT, lib, prefill_and_decode, qkcs, tiny_model  # noqa: F401  (lib: a fixture)


def tiny_qwen3(dtype=torch.float16, device="cpu", layer_types=("full_attention", "full_attention")):
    """hidden 256, 2 layers, 4 heads of 64, 2 kv heads, vocab 64, random weights; the norm weights random in [0.5, 1.5] (ones would
    hide a missing or swapped weight)."""
    import transformers
    cfg = transformers.Qwen3Config(hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64,
                                   vocab_size=64, max_position_embeddings=64, tie_word_embeddings=False, layer_types=list(layer_types),
                                   use_sliding_window="sliding_attention" in layer_types, sliding_window=16)
    cfg._attn_implementation = "sdpa"
    torch.manual_seed(42)
    model = transformers.Qwen3ForCausalLM(cfg)
    for layer in model.model.layers:
        for norm in (layer.self_attn.q_norm, layer.self_attn.k_norm):
            norm.weight.data.uniform_(0.5, 1.5)
    return model.to(dtype).to(device).eval()


def test_symbol_is_declared_exported_and_public(lib):  # noqa: F811
    header = re.sub(r"/\*.*?\*/", "", open(f"{ROOT}/include/qllm_mi355x.h").read(), flags=re.S)
    assert re.search(r"\bqllm_rope_qknorm\s*\(", header) and "qllm_rope_qknorm" in _lib.EXPORTS
    assert len(lib.qllm_rope_qknorm.argtypes) == 20
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert {"rope_qknorm", "rope_qknorm_plan"} <= set(ops.__all__)


@pytest.mark.parametrize("bad,code,text", [
    (dict(q_weight=None), "INVALID", "must not be NULL"), (dict(k_weight=None), "INVALID", "must not be NULL"),
    (dict(q_weight=4096 * 7 + 8), "INVALID", "16-byte aligned"), (dict(eps=0.0), "INVALID", "eps"), (dict(eps=-1e-6), "INVALID", "eps"),
    (dict(eps=float("inf")), "INVALID", "eps"), (dict(eps=float("nan")), "INVALID", "eps"), (dict(d=96), "UNSUPPORTED", "64 and 128"),
    (dict(rows=0), "INVALID", "must be >= 1"), (dict(d=24), "UNSUPPORTED", "rope serves head_dim"),       # qllm_rope's rules, by its texts
])
def test_entry_refuses_before_any_device_work(lib, bad, code, text):  # noqa: F811
    p = {n: 4096 * (i + 1) for i, n in enumerate(("q", "k", "cos", "sin", "q_out", "k_out", "q_weight", "k_weight"))}
    a = {**p, "eps": 1e-6, "rows": 3, "d": 64, **bad}
    rc = lib.qllm_rope_qknorm(a["q"], a["k"], a["cos"], a["sin"], a["q_out"], a["k_out"], a["q_weight"], a["k_weight"], a["eps"], a["rows"], 4, 2, a["d"],
                              6 * a["d"], a["d"], 2 * a["d"], a["d"], 3, _lib.DT_F16, None)
    assert rc == getattr(_lib, "QLLM_ERR_" + code) and text in _lib.last_error(), _lib.last_error()


def test_the_kernels_are_spill_free_without_scratch_or_lds():
    res = resources("rope_qknorm.hip")
    assert len(res) == 4, sorted(res)                                                         # fp16 / bf16 x head_dim 64 / 128
    for n, r in res.items():
        assert "rope_qknorm_kernel" in n
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0 and r["private_segment_fixed_size"] == 0 and r["group_segment_fixed_size"] == 0, (n, r)


@pytest.mark.parametrize("change,text", [
    ({}, None), (dict(d=96), "head_dim must be 64 or 128"), (dict(dtype=torch.float32), "one type"), (dict(ud=0), "unsqueeze_dim"),
    (dict(wq=lambda w: w[:32]), r"q_weight must be a \[64\]"), (dict(wk=lambda w: w.bfloat16()), "k_weight must be of q's type"),
    (dict(wk=lambda w: w.repeat_interleave(2)[::2]), "k_weight must be contiguous"), (dict(wq=lambda w: w[None]), r"q_weight must be a \[64\]"),
    (dict(eps=0.0), "eps must be finite"),
])
def test_plan_refuses_with_the_reason(change, text):
    d, dtype = change.get("d", 64), change.get("dtype", torch.float16)
    q, k, cos, sin = qkcs(2, 3, 4, 2, d, dtype)
    wq, wk = (change.get(n, lambda w: w)(torch.ones(d, dtype=dtype)) for n in ("wq", "wk"))
    if not change:                                                                            # the premise: unchanged, the call is served
        assert ops.rope_qknorm_plan(q, k, wq, wk, 1e-6, cos, sin) == ops.rope_plan(q, k, cos, sin)
        return
    with pytest.raises(ops.QllmUnsupported, match=text):
        ops.rope_qknorm_plan(q, k, wq, wk, change.get("eps", 1e-6), cos, sin, change.get("ud", 1))


def test_known_takes_a_qwen3_attention_and_needs_both_norms():
    model = tiny_qwen3(layer_types=("full_attention", "sliding_attention"))
    a0, a1 = (layer.self_attn for layer in model.model.layers)
    family = sys.modules[type(a0).__module__]
    assert fused_rope._known(a0) == (family.apply_rotary_pos_emb, "self") == fused_rope._known(a1)
    assert (a0.sliding_window, a1.sliding_window) == (None, 16)
    del a1.k_norm
    a0.q_norm.weight = torch.nn.Parameter(torch.ones(32))                                     # not head_dim elements
    assert fused_rope._known(a0) is None and fused_rope._known(a1) is None
    assert install_fused_rope(model) == 0


def test_a_qwen2_forward_never_looks_for_q_norm():
    model = tiny_model("qwen2", 4, 2, "sdpa")
    want = prefill_and_decode(model)
    for layer in model.model.layers:
        cls = type(layer.self_attn)
        layer.self_attn.__class__ = type(cls.__name__, (cls,), {"__module__": cls.__module__, "q_norm": property(lambda s: pytest.fail("q_norm looked for")),
                                                                "k_norm": property(lambda s: pytest.fail("k_norm looked for"))})
    assert install_fused_rope(model) == 2
    assert all(torch.equal(g, w) for g, w in zip(prefill_and_decode(model), want))


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32], ids=["f16", "f32"])
def test_on_cpu_tensors_the_patched_qwen3_forward_returns_eager_bits(dtype, monkeypatch):
    model = tiny_qwen3(dtype)
    want = prefill_and_decode(model)
    assert all(bool(torch.isfinite(w.float()).all()) for w in want)
    monkeypatch.setattr(ops, "rope_qknorm", lambda *a, **kw: pytest.fail("ops.rope_qknorm called for CPU tensors"))
    assert install_fused_rope(model) == 2
    assert all(torch.equal(g, w) for g, w in zip(prefill_and_decode(model), want))
    assert uninstall_fused_rope(model) == 2 and not any("forward" in m.__dict__ for m in model.modules())
