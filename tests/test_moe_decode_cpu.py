"""The routed-experts entries without a device (qllm_moe_gate_up, qllm_moe_down, qllm_moe_describe; csrc/moe_decode.hip): the symbols,
every refusal of the C entries -- reached with fake pointers, before any device work -- and ops.moe_plan's reason for each unserved form."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from gpu_util import synth
from capi_fakes import BUFLEN, QWEIGHT, QZEROS, SCALES, X, Y
from qllm_amd import _lib, ops

ENTRIES = ("qllm_moe_gate_up", "qllm_moe_down", "qllm_moe_describe")
IDS, WTS, INVALID, UNSUPPORTED = 1 << 20, 2 << 20, _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED
GOOD = dict(T=1, top_k=2, E=8, H=256, I=384, azb=0, dt=_lib.DT_F16, wdt=_lib.DT_F32, x=X, ids=IDS, wts=WTS, qw=QWEIGHT, sc=SCALES, qz=QZEROS, qz2=QZEROS, out=Y)


def _call(entry, **change):
    a = dict(GOOD, **change)
    lib, sizes = _lib.load(), (a["T"], a["top_k"], a["E"], a["H"], a["I"])
    if entry == "qllm_moe_gate_up":
        rc = lib.qllm_moe_gate_up(a["x"], a["ids"], a["qw"], a["sc"], a["qz"], a["qw"], a["sc"], a["qz2"], a["out"], *sizes, a["azb"], a["dt"], None)
    elif entry == "qllm_moe_down":
        rc = lib.qllm_moe_down(a["x"], a["ids"], a["wts"], a["qw"], a["sc"], a["qz"], a["out"], *sizes, a["azb"], a["wdt"], a["dt"], None)
    else:
        buf = C.create_string_buffer(BUFLEN)
        rc = lib.qllm_moe_describe(*sizes, buf if a.get("buf", True) else None, BUFLEN)
        return rc, buf.value.decode() if rc == 0 else _lib.last_error()
    return rc, _lib.last_error()


def test_symbols_are_in_the_header_and_in_the_binding():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "qllm_mi355x.h")).read()
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\(", header) and name in _lib.EXPORTS and hasattr(_lib.load(), name)
    assert {"moe_gate_up", "moe_down", "moe_plan", "moe_describe"} <= set(ops.__all__)
    assert ops.moe_describe(1, 2, 8, 4096, 14336) == "moe_decode gate_up grid=896x2 waves=8 groups_per_wave=4 lds=9216 | down grid=256x1 waves=16 groups_per_wave=14"
    assert ops.moe_describe(4, 8, 128, 2048, 768).endswith("down grid=128x4 waves=16 groups_per_wave=3")


REFUSALS = [  # (entries it applies to, the change, status, a word of the message)
    ("AB", dict(x=None), INVALID, "NULL"), ("AB", dict(ids=None), INVALID, "NULL"), ("AB", dict(out=None), INVALID, "NULL"),
    ("B", dict(wts=None), INVALID, "NULL"), ("AB", dict(qw=None), INVALID, "NULL"), ("AB", dict(sc=None), INVALID, "NULL"),
    ("A", dict(qz2=None), INVALID, "both"), ("AB", dict(x=X + 8), INVALID, "aligned"), ("AB", dict(ids=IDS + 4), INVALID, "aligned"),
    ("AB", dict(qw=QWEIGHT + 4), INVALID, "aligned"), ("B", dict(wts=WTS + 2), INVALID, "aligned"), ("AB", dict(azb=2), INVALID, "add_zero_bias"),
    ("AB", dict(dt=_lib.DT_F32), INVALID, "act_dtype"), ("B", dict(wdt=_lib.DT_BF16), INVALID, "weights_dtype"),
    ("ABD", dict(T=0), INVALID, ">= 1"), ("ABD", dict(top_k=0), INVALID, ">= 1"), ("ABD", dict(E=0), INVALID, ">= 1"),
    ("ABD", dict(T=5), UNSUPPORTED, "tokens"), ("ABD", dict(top_k=9), UNSUPPORTED, "top_k"), ("ABD", dict(E=(1 << 24) + 1), UNSUPPORTED, "experts"),
    ("ABD", dict(H=192), UNSUPPORTED, "128"), ("ABD", dict(I=320), UNSUPPORTED, "128"), ("ABD", dict(H=16512), UNSUPPORTED, "16384"),
    ("D", dict(buf=False), INVALID, "buf"),
]


@pytest.mark.parametrize("which,change,status,word", REFUSALS, ids=lambda v: str(v) if isinstance(v, dict) else None)
def test_every_refusal_is_reached_before_any_device_work(which, change, status, word):
    for letter, entry in zip("ABD", ENTRIES):
        if letter not in which:
            continue
        rc, text = _call(entry, **change)
        if entry == "qllm_moe_describe" and status == UNSUPPORTED:   # a describe entry answers a refusal as text
            assert rc == 0 and text.startswith("refused: ") and word in text, (rc, text)
        else:
            assert rc == status and word in text, (entry, rc, text)


def _stack(e, k, n, zeros=True):
    return (torch.zeros(e, n // 16, k // 8, 16, dtype=torch.int32), torch.zeros(e, n // 16, k // 128, 16, dtype=torch.float16),
            torch.zeros(e, n // 16, k // 128, 2, dtype=torch.int32) if zeros else None)


def _plan_args(t=1, top_k=2, e=4, h=256, i=384, dtype=torch.float16, wdtype=torch.float32, **stacks):
    st = dict(gate=_stack(e, h, i), up=_stack(e, h, i), down=_stack(e, i, h))
    st.update(stacks)
    return [torch.zeros(t, h, dtype=dtype), torch.zeros(t, top_k, dtype=torch.int64), torch.zeros(t, top_k, dtype=wdtype), st["gate"], st["up"], st["down"]]


def test_plan_serves_the_decode_forms():
    assert ops.moe_plan(*_plan_args(t=4, top_k=8, e=64, dtype=torch.bfloat16, wdtype=torch.bfloat16)) == (4, 8, 64, 256, 384)
    sym = {k: _stack(4, *kn, zeros=False) for k, kn in (("gate", (256, 384)), ("up", (256, 384)), ("down", (384, 256)))}
    assert ops.moe_plan(*_plan_args(**sym)) == (1, 2, 4, 256, 384)


PLAN_REFUSALS = [
    (dict(t=5), None, "tokens"), (dict(t=4, top_k=2, e=8), None, "reads each hit expert once"), (dict(top_k=9), None, "top_k"), (dict(dtype=torch.float32), None, "float16 / bfloat16"),
    (dict(wdtype=torch.float64), None, "weights must be"), (dict(h=192), None, "multiple of 128"), (dict(h=16512), None, "H <= 16384"),
    (dict(up=_stack(4, 256, 512)), None, "one expert count"), (dict(down=_stack(3, 384, 256)), None, "one expert count"),
    (dict(gate=_stack(4, 256, 384, zeros=False)), None, "all have packed zero points"), ({}, (1, lambda t: t.to(torch.int32)), "int64"),
    ({}, (0, lambda t: t.t().contiguous().t() if t.shape[0] > 1 else t[:, ::2]), "contiguous"), ({}, (3, lambda s: (s[0].to(torch.int64),) + s[1:]), "int32"),
    ({}, (4, lambda s: (s[0], s[1].float(), s[2])), "scales must be float16"),
]


@pytest.mark.parametrize("kw,edit,word", PLAN_REFUSALS, ids=[r[2] for r in PLAN_REFUSALS])
def test_plan_gives_the_reason_it_refuses(kw, edit, word):
    args = _plan_args(**kw)
    if edit is not None:
        args[edit[0]] = edit[1](args[edit[0]])
    with pytest.raises(ops.QllmUnsupported, match=re.escape(word)):
        ops.moe_plan(*args)


def tiny_checkpoint(path, family):
    """A two-layer model from config (Mixtral: a sliding window of 4) whose experts are random packed GPTQ layers under the checkpoint's
    per-expert names."""
    import safetensors.torch
    import transformers
    common = dict(vocab_size=64, hidden_size=256, num_hidden_layers=2, num_attention_heads=4, num_key_value_heads=2, head_dim=64, max_position_embeddings=64,
                  torch_dtype="float16", num_experts_per_tok=2)
    if family == "mixtral":
        cfg, block, names = transformers.MixtralConfig(intermediate_size=384, num_local_experts=4, sliding_window=4, **common), "block_sparse_moe", ("w1", "w3", "w2")
    else:
        cfg = transformers.Qwen3MoeConfig(intermediate_size=384, moe_intermediate_size=384, num_experts=4, norm_topk_prob=True, **common)
        block, names = "mlp", ("gate_proj", "up_proj", "down_proj")
    torch.manual_seed(0)
    model = transformers.AutoModelForCausalLM.from_config(cfg).half()
    sd = {k: v.contiguous() for k, v in model.state_dict().items() if ".experts." not in k}
    for layer in range(2):
        for ex in range(4):
            for kind, (name, (k, n)) in enumerate(zip(names, ((256, 384), (256, 384), (384, 256)))):
                d = synth("GPTQ", 4, 128, k, n, seed=1000 * layer + 10 * ex + kind)
                for buf in ("qweight", "qzeros", "scales", "g_idx"):
                    sd[f"model.layers.{layer}.{block}.experts.{ex}.{name}.{buf}"] = torch.from_numpy(np.ascontiguousarray(d[buf]))
    cfg.save_pretrained(path)
    safetensors.torch.save_file(sd, os.path.join(path, "model.safetensors"))
    json.dump(dict(bits=4, group_size=128, version="GPTQ", quant_method="gptq"), open(os.path.join(path, "quantize_config.json"), "w"))


@pytest.mark.parametrize("family", ["mixtral", "qwen3_moe"])
def test_a_loaded_checkpoint_round_trips_through_save_quantized(family, tmp_path):
    from qllm_amd.modeling.base import load_quantized, save_quantized
    tiny_checkpoint(str(tmp_path / "a"), family)
    first = load_quantized(str(tmp_path / "a"), device=None)
    save_quantized(first, str(tmp_path / "b"))
    again = load_quantized(str(tmp_path / "b"), device=None)
    a, b = first.state_dict(), again.state_dict()
    assert again.quant_experts == 2 and again.load_report["unexpected_keys"] == [] and sum(k.endswith(".qweight") for k in b) == 24
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
