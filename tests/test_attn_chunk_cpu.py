"""No GPU: qllm_attn_chunk as far as a host reaches -- the plan's refusals, the pure describe / workspace entries, the C entry's checks before
device work, the built kernels' resources -- and the host logic of install_fused_attention(model, prefill="split") on the tiny llama of
tests/decode_loop_cases.py with torch restatements in the ops' place."""
import os
import re
import subprocess
import sys

import pytest
import torch

import attn_prefill_cases as AP
import attn_sliding_cases as S
import decode_loop_cases as D
from kernel_resources import resources
from test_attn_decode_cpu import tiny_model
from test_rope_cpu import fake_op as fake_rope

from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, uninstall_fused_attention
from qllm_amd.modeling.q_layers.fused_rope import _CORE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, UNS, WS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED, _lib.QLLM_ERR_WORKSPACE


def tensors(b=1, hq=8, hk=2, d=64, s=4, L=300, dtype=torch.float16):
    return torch.zeros(b, hq, s, d, dtype=dtype), torch.zeros(b, hk, L, d, dtype=dtype), torch.zeros(b, hk, L, d, dtype=dtype)


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,why", [(dict(s=1), "at least two rows"), (dict(hq=8, hk=1, s=17), "128 query rows"), (dict(hq=9, hk=1), "8 query heads per kv head"),
                                     (dict(d=96), "head_dim 64 or 128"), (dict(b=1100, hq=8, hk=1, d=128, s=16, L=16), "a workspace of at most")])
def test_the_plan_refuses_what_the_kernel_does_not_serve(how, why):
    q, k, v = tensors(**how)
    with pytest.raises(ops.QllmUnsupported, match=why):
        ops.attn_chunk_plan(q, k, v, k.shape[2])


def test_the_plan_is_attn_prefill_plans_tuple_and_refuses_a_short_mask():
    q, k, v = tensors()
    mask = torch.ones(1, 1, 4, 300, dtype=torch.bool)
    assert ops.attn_chunk_plan(q, k, v, 200, mask) == ops.attn_prefill_plan(q, k, v, 200, mask) and len(ops.attn_chunk_plan(q, k, v, 200)) == 16
    with pytest.raises(ops.QllmUnsupported, match="the mask must cover 200 positions"):
        ops.attn_chunk_plan(q, k, v, 200, mask[..., :199])


# ---- describe and workspace bytes: pure and monotone ---------------------------------------------------------------------------------------------------
GEOMETRY_256 = """
import re
from qllm_amd import ops, _lib
lib = _lib.load()
def geo(*a):
    return {k: int(v) for k, v in re.findall(r"(rows|row_tiles|kv_tile|splits|chunk)=(\\d+)", ops.attn_chunk_describe(*a))}
g = geo(1, 32, 8, 128, 16, 4096)
assert g == dict(rows=64, row_tiles=2, kv_tile=64, splits=32, chunk=128), g
assert ops.attn_chunk_describe(1, 32, 8, 128, 16, 4096).endswith("grid=32x8x1")
for b, hq, hk, d, s in ((1, 32, 32, 128, 2), (1, 32, 8, 128, 16), (4, 28, 4, 128, 8), (64, 8, 8, 64, 128), (500, 8, 8, 64, 3)):
    last = 0
    for lmax in (s, 64, 65, 1000, 4096, 4097, 100000):
        if lmax < s:
            continue
        g = geo(b, hq, hk, d, s, lmax)
        tiles = -(-lmax // g["kv_tile"])
        assert g["chunk"] % g["kv_tile"] == 0 and 1 <= g["splits"] <= min(32, tiles) and g["splits"] == -(-lmax // g["chunk"]), (g, lmax)
        assert b * hk * g["splits"] <= 2 * 256 + b * hk                       # about two blocks per compute unit
        need = lib.qllm_attn_chunk_workspace_bytes(b, hq, hk, d, s, lmax)
        assert need >= 16384 + b * hk * g["splits"] * g["rows"] * (d + 4) * 4   # the counter page and every live block's rows
        assert need >= last and need == lib.qllm_attn_chunk_workspace_bytes(b, hq, hk, d, s, lmax)
        assert need <= lib.qllm_attn_chunk_workspace_bytes(b + 1, hq, hk, d, s, lmax)
        last = need
print("ok")
"""


def test_describe_and_workspace_bytes_are_pure_and_monotone_at_256_compute_units():
    env = dict(os.environ, QLLM_NUM_CU="256", PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-c", GEOMETRY_256], env=env, capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and out.stdout.strip().endswith("ok"), out.stderr[-2000:]


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: only where no HIP device is visible")
def test_the_entry_refuses_bad_arguments_before_device_work():
    lib = _lib.load()
    p = torch.zeros(1 << 14, dtype=torch.float16).data_ptr()

    def call(q=p, batch=1, hq=8, hk=2, d=64, s=4, kv_len=100, max_len=300, q_row=64, mask=None, kind=0, mask_len=0, causal=1, ws=None, ws_bytes=0):
        return lib.qllm_attn_chunk(q, p, p, mask, p, batch, hq, hk, d, s, kv_len, None, max_len, 2048, 256, q_row, 0, 19200, 64, kind, mask_len, 0, 300, causal,
                                   0.125, 0, ws, ws_bytes, None)

    assert call(q=None) == INV and call(s=1) == INV and "q_len must lie in 2..max_len" in _lib.last_error()
    assert call(causal=2) == INV and call(q_row=60) == INV and call(q=p + 2) == INV
    assert call(kv_len=3) == INV and call(kv_len=301) == INV
    assert call(mask=p, kind=1, mask_len=99) == INV and "the mask must cover 100 positions" in _lib.last_error()
    assert call(d=96) == UNS and call(hq=9, hk=1) == UNS
    assert call(hq=8, hk=1, s=17) == UNS and "136" in _lib.last_error()                # the kernel's own served checks, behind the shared rules
    assert call(batch=2049, hk=2, hq=2) == UNS and "batch * kv_heads" in _lib.last_error()
    assert call() == WS and call(ws=p, ws_bytes=16384) == WS                            # then the workspace, and nothing was launched


def test_every_instantiation_is_built_without_scratch_or_spills():
    kernels = {name: r for name, r in resources("attn_chunk.hip").items() if "attn_chunk_kernel" in name}
    assert len(kernels) == 12, sorted(kernels)                                       # 2 types x 2 head sizes x 3 mask kinds
    for name, r in kernels.items():
        assert r["private_segment_fixed_size"] == 0 and r["sgpr_spill_count"] == 0 and r["vgpr_spill_count"] == 0, (name, r)


# ---- the modules ------------------------------------------------------------------------------------------------------------------------------------------
PIECES = ((0, 5), (5, 9), (9, 10))               # a prompt, a masked chunk of four behind it, one decode step


def restatements(monkeypatch):
    monkeypatch.setattr(fused_attention, "_on_device", lambda *ts: True)
    fake_rope(monkeypatch)
    calls = S.record(monkeypatch, S.decode_restated, S.prefill_restated)

    def attn_chunk(q, k_cache, v_cache, length, **kw):
        calls.append(("chunk", q.shape[2], int(length), kw.get("mask") is not None))
        return AP.restated(q, k_cache, v_cache, length, **kw)

    monkeypatch.setattr(ops, "attn_chunk", attn_chunk)
    return calls


def names(calls):
    return [(c[0], c[1]) if isinstance(c, tuple) else (c.op, c.q_len) for c in calls]


def run(model, prefill, inp, cache, calls):
    del calls[:]
    assert install_fused_attention(model, prefill=prefill) == D.LAYERS
    try:
        return S.forwards(model, inp, cache, "cpu", PIECES)[0], names(calls)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_split_hands_the_masked_chunk_to_the_op_and_everything_else_where_true_takes_it(cache, batch, monkeypatch):
    model = tiny_model("llama", "sdpa", torch.float16, "cpu")
    inp = D.batch_inputs(batch)
    reference = S.forwards(D.float64_copy(model), inp, "dynamic", "cpu", PIECES)[0]
    unfused = S.forwards(model, inp, cache, "cpu", PIECES)[0]
    calls = restatements(monkeypatch)
    true, true_calls = run(model, True, inp, cache, calls)
    split, split_calls = run(model, "split", inp, cache, calls)
    L = D.LAYERS
    # prefill=True as before: the masked chunk of a dynamic layer on the family's route, that of a static layer through ops.attn_prefill
    assert true_calls == [("prefill", 5)] * L + ([("prefill", 4)] * L if cache == "static" else []) + [("decode", 1)] * L
    assert split_calls == [("prefill", 5)] * L + [("chunk", 4)] * L + [("decode", 1)] * L
    assert all(c[2] == 9 and c[3] for c in calls if isinstance(c, tuple))            # the length behind `update`, and the mask
    assert D.same_bits(split[0], true[0])                                              # the prompt: the same route, the same bits
    e_unfused, e_split = (unfused.double() - reference).abs().max().item(), (split.double() - reference).abs().max().item()
    assert e_unfused > 0 and e_split <= D.M_CPU * e_unfused, (e_split, e_unfused)
    # what keeps a call off the new route leaves it exactly where prefill=True takes it: a refused plan, the row bound, a bound of zero
    def refuse(*a, **kw):
        raise ops.QllmUnsupported(UNS, "refused here")
    for name, value in (("ops.attn_chunk_plan", refuse), ("SPLIT_MAX_ROWS", 3), ("SPLIT_MAX_ROWS", 0)):
        with monkeypatch.context() as m:
            m.setattr(ops if name.startswith("ops.") else fused_attention, name.split(".")[-1], value)
            again, again_calls = run(model, "split", inp, cache, calls)
        assert again_calls == true_calls and D.same_bits(again, true), name


def test_the_option_values_install_the_cores_they_name(monkeypatch):
    model = tiny_model("llama", "sdpa", torch.float16, "cpu")
    core = lambda: {mod.__dict__[_CORE][3] for mod in model.modules() if _CORE in mod.__dict__}
    for prefill, want, counted in ((False, fused_attention._fused_core, 0), (True, fused_attention._fused_core_prefill, D.LAYERS),
                                   ("split", fused_attention._fused_core_split, D.LAYERS)):
        assert install_fused_attention(model, prefill=prefill) == D.LAYERS
        assert core() == {want} and fused_attention.count_fused_attention_prefill(model) == counted
        assert uninstall_fused_attention(model) == D.LAYERS
    monkeypatch.setenv("QLLM_FUSE_ATTENTION_PREFILL", "0")                              # "split" becomes a no-op like True
    assert install_fused_attention(model, prefill="split") == D.LAYERS and core() == {fused_attention._fused_core}
    assert uninstall_fused_attention(model) == D.LAYERS
    with pytest.raises(ValueError):
        install_fused_attention(model, prefill="chunk")
    assert set(fused_attention.PREFILL_ROUTES) == {(k, m) for k in ("dynamic", "static", "dynamic_sliding", "static_sliding") for m in (False, True)}
