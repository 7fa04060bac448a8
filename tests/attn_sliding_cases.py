"""What tests/test_attn_sliding_cpu.py and tests/test_attn_sliding_gpu.py share: the sliding window as a bool band (the form in which the
float64 oracles of attn_decode_cases.py and attn_prefill_cases.py take it), the torch restatements of ops.attn_decode / ops.attn_prefill
with the `window` keyword, the tiny Mistral and Qwen2 models whose layers slide, and the harness that records what the modules hand to the ops.

Semantics (transformers' sliding_window_overlay on a linear cache): a query at absolute position p sees key j only if p - W < j <= p."""
from types import SimpleNamespace

import torch

import attn_decode_cases as AD
import attn_prefill_cases as AP
import decode_loop_cases as D

GROUPS = ((8, 2), (7, 1))
DIMS = (64, 128)
DTYPES = (torch.float16, torch.bfloat16)


# ---- the band ------------------------------------------------------------------------------------------------------------------------------------
def decode_band(n, window, width):
    """[1, width] bool: the positions the query at n - 1 sees of n counted ones, n - W <= j < n (window None: every j < n)."""
    j = torch.arange(width)[None, :]
    return (j < n) & (j >= (0 if window is None else n - window))


def prefill_band(s, n, window, width):
    """[1, s, width] bool: row i at n - s + i sees j > n - s + i - W (window None: every j); causality and the length are the oracle's."""
    j, i = torch.arange(width)[None, None, :], torch.arange(s)[None, :, None]
    return torch.ones(1, s, width, dtype=torch.bool) if window is None else j > n - s + i - window


def with_band(mask, band):
    """`mask` (None, bool, or additive) ANDed with `band` (bool, broadcastable to it): hidden where the band hides."""
    if mask is None:
        return band
    if mask.dtype == torch.bool:
        return mask & band
    return torch.where(band, mask, torch.full((), torch.finfo(mask.dtype).min, dtype=mask.dtype, device=mask.device))


# ---- the ops restated with the window --------------------------------------------------------------------------------------------------------------
def _decode_mask(q, k_cache, length, k_new, mask, window):
    if window is None:
        return mask
    n = int(length) + (1 if k_new is not None else 0)
    band = decode_band(n, window, k_cache.shape[2]).to(q.device)
    if mask is None:
        return band
    m2 = mask.reshape(mask.shape[0], -1)
    return with_band(m2, band[:, :m2.shape[1]])


def decode_restated32(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None, *, window=None):
    return AD.restated32(q, k_cache, v_cache, length, k_new, v_new, _decode_mask(q, k_cache, length, k_new, mask, window), scaling)


def decode_restated(q, k_cache, v_cache, length, k_new=None, v_new=None, mask=None, scaling=None, *, out=None, plan=None, window=None):
    """ops.attn_decode restated in torch with its `window` keyword (any device).  Same signature."""
    return decode_restated32(q, k_cache, v_cache, length, k_new, v_new, mask, scaling, window=window).to(q.dtype)


def _prefill_mask(q, k_cache, length, mask, window):
    if window is None:
        return mask
    band = prefill_band(q.shape[2], int(length), window, k_cache.shape[2]).to(q.device)
    if mask is None:
        return band
    m3 = mask[:, 0] if mask.dim() == 4 else mask
    return with_band(m3, band[:, :, :m3.shape[2]])


def prefill_restated32(q, k_cache, v_cache, length, mask=None, causal=True, scaling=None, *, window=None):
    return AP.restated32(q, k_cache, v_cache, length, _prefill_mask(q, k_cache, length, mask, window), causal, scaling)


def prefill_restated(q, k_cache, v_cache, length, mask=None, causal=True, scaling=None, *, out=None, plan=None, window=None):
    """ops.attn_prefill restated in torch with its `window` keyword (any device).  Same signature."""
    return prefill_restated32(q, k_cache, v_cache, length, mask, causal, scaling, window=window).to(q.dtype)


# ---- the models ------------------------------------------------------------------------------------------------------------------------------------
MODELS = {"mistral-4": ("mistral", 4), "mistral-8": ("mistral", 8), "qwen2-4": ("qwen2", 4)}


def sliding_model(name, attn="sdpa", dtype=torch.float16, device="cpu"):
    """(test_attn_decode_cpu.tiny_model whose layers slide, [whether layer l slides], the window).  mistral-W: both layers slide;
    qwen2-4: layer 0 full, layer 1 sliding.  With the 5-token prompt and 8 steps of decode_loop_cases, W = 4 is crossed in the prompt and
    W = 8 during the decode steps."""
    from test_attn_decode_cpu import tiny_model
    family, window = MODELS[name]
    if family == "mistral":
        return tiny_model("mistral", attn, dtype, device, sliding_window=window), [True, True], window
    model = tiny_model("qwen2", attn, dtype, device, use_sliding_window=True, sliding_window=window, max_window_layers=1)
    assert model.config.layer_types == ["full_attention", "sliding_attention"]
    return model, [False, True], window


def record(monkeypatch, decode_op, prefill_op):
    """`ops.attn_decode` / `ops.attn_prefill` replaced by recorders around the two given ops (the restatements on the CPU, the kernels on the
    device).  -> the list the calls are appended to: op, q_len, the length as an int, whether it came as a device tensor, the positions
    of what `update` returned, whether `window` was passed and its value."""
    from qllm_amd import ops
    calls = []

    def wrap(name, real):
        def op(q, k_cache, v_cache, length, *a, **kw):
            calls.append(SimpleNamespace(op=name, q_len=q.shape[2] if name == "prefill" else 1, length=int(length), on_device=isinstance(length, torch.Tensor),
                                         returned=k_cache.shape[2], has_window="window" in kw, window=kw.get("window")))
            return real(q, k_cache, v_cache, length, *a, **kw)
        return op

    monkeypatch.setattr(ops, "attn_decode", wrap("decode", decode_op))
    monkeypatch.setattr(ops, "attn_prefill", wrap("prefill", prefill_op))
    return calls


def expected_decode_call(cache, slides, window, tokens):
    """(length, on_device, returned) of the decode call of one layer after `update` took the `tokens`-th token (StaticCache:
    decode_loop_cases.MAX_CACHE_LEN positions)."""
    if not slides:
        return (tokens, True, D.MAX_CACHE_LEN) if cache == "static" else (tokens, False, tokens)
    if cache == "dynamic":                                                     # the layer keeps W - 1 positions and returns them with the new one
        return min(tokens, window), False, min(tokens, window)
    held = min(window, D.MAX_CACHE_LEN)
    return (tokens, True, held) if tokens <= held else (held, False, held)     # the device counter until the layer overflows, then all it returns


def open_routes(monkeypatch):
    """Every (cache layer kind, mask or none) routed to ops.attn_prefill, chunks included: the routing tests are about the modules, not about
    where the kernel wins."""
    from qllm_amd.modeling.q_layers import fused_attention
    kinds = ("dynamic", "static", "dynamic_sliding", "static_sliding")
    monkeypatch.setattr(fused_attention, "PREFILL_ROUTES", {(k, m): (2, None, True) for k in kinds for m in (False, True)})


def forwards(model, inp, cache, device, pieces):
    """The token ranges `pieces` ((0, 5), (5, 8), (8, 9), ...) fed one after the other through `cache` ("dynamic" / "static").  -> the
    last-token logits of each forward [pieces, B, V] on the CPU, and the cache."""
    ids, pos = inp.ids.to(device), inp.pos.to(device)
    mask = None if inp.mask is None else inp.mask.to(device)
    cache = D.make_cache(model, cache)
    out = []
    with torch.no_grad():
        for a, b in pieces:
            out.append(model(ids[:, a:b], attention_mask=None if mask is None else mask[:, :b], position_ids=pos[:, a:b], past_key_values=cache,
                             use_cache=True).logits[:, -1].cpu())
    return torch.stack(out), cache


# ---- the 4-bit GPTQ tiny Mistral ---------------------------------------------------------------------------------------------------------------------
def mistral_config(dtype="float16", window=4):
    import transformers
    return transformers.MistralConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=D.LAYERS, num_attention_heads=4, num_key_value_heads=2,
                                      vocab_size=D.VOCAB, max_position_embeddings=64, torch_dtype=dtype, tie_word_embeddings=False, sliding_window=window)


def quantized_mistral(window=4):
    """decode_loop_cases.quantized_llama as a Mistral whose layers slide: every decoder linear a 4-bit, group-128 GPTQ layer."""
    import transformers
    from test_loader_repack_cpu import _quantize_in_place
    torch.manual_seed(0)
    model, _ = _quantize_in_place(transformers.MistralForCausalLM(mistral_config(window=window)).half(), "GPTQ")
    return model.eval()


def dense_mistral_reference(qmodel, window=4):
    """decode_loop_cases.dense_reference for `quantized_mistral`: a dense float64 MistralForCausalLM, scales * (codes - zeros) from the
    integers."""
    import transformers
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    cfg = mistral_config("float64", window)
    cfg._attn_implementation = "sdpa"
    ref = transformers.MistralForCausalLM(cfg).double().eval()
    quantized = {n: m for n, m in qmodel.named_modules() if isinstance(m, QuantLinearGPTQ)}
    state = {}
    for name, layer in quantized.items():
        codes, zeros = layer.unpack_qweight("cpu").double(), layer.unpack_qzeros("cpu").double()
        g = layer.g_idx.long()
        state[name + ".weight"] = (layer.scales.double()[g] * (codes - zeros[g])).T.contiguous()
    for name, t in qmodel.state_dict().items():
        if name.rsplit(".", 1)[0] not in quantized:
            state[name] = t.double()
    ref.load_state_dict(state, strict=True)
    return ref


# ---- exact selection under a window ------------------------------------------------------------------------------------------------------------------
SEL_A, SEL_SCALING = 64.0, 0.125


def snake_code(j):
    """(c, 16 + block) of key j: block = j // 16, c = j % 16 walked back and forth (15 - j % 16 in odd blocks), so that NEIGHBOURING keys
    always share exactly one of their two components.  (With a code whose neighbours differ in both, the two keys that mix their
    components score, together, what the neighbours score together: no q could put one neighbour first and the other second.)"""
    block, c = j // 16, j % 16
    return torch.where(block % 2 == 0, c, 15 - c), 16 + block


def window_selection(b, hq, hk, d, s, q_start, window, dtype):
    """q, k, v, target [S], scaling in the style of attn_prefill_cases.selection: key j carries A (e_c + e_block) of `snake_code`.  Row i at
    p = q_start + i carries the code of the key at p - W (just outside its window) once and the code of its target p - W + 1 (the oldest
    key it sees) half: the hidden key scores 2.5 A^2 / 8, the target 2 A^2 / 8, every other key at most 1.5 A^2 / 8 -- 256 below the target,
    369 in the log2 domain: weight exactly 0.  Where p - W < 0 there is no hidden key and the target is key 0.  So out[b, i, h, :] ==
    V[b, h / G, target[i], :] bit for bit, and a kernel that lets p - W in returns that row instead."""
    n = q_start + s
    assert n <= 16 * (d - 16) and n <= 401
    j = torch.arange(n)
    c, blk = snake_code(j)
    k1 = torch.zeros(n, d, dtype=torch.float64)
    k1[j, c] = SEL_A
    k1[j, blk] = SEL_A
    p = q_start + torch.arange(s)
    hidden, target = p - window, (p - window + 1).clamp(min=0)
    q1 = 0.5 * k1[target]
    q1[hidden >= 0] += k1[hidden[hidden >= 0]]
    k = k1[None, None].expand(b, hk, n, d).to(dtype).contiguous()
    q = q1[None, None].expand(b, hq, s, d).to(dtype).contiguous()
    assert torch.equal(q.double()[0, 0], q1) and torch.equal(k.double()[0, 0], k1)                         # exact in the type
    return q, k, AP.value_rows(b, hk, n, d, dtype), target, SEL_SCALING


def window_selection_expected(v, target, hq):
    """[B, S, Hq, D]: V[b, h / G, target[i], :]"""
    return v[:, :, target].repeat_interleave(hq // v.shape[1], dim=1).transpose(1, 2).contiguous()
