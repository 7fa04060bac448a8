"""-m gpu: ops.attn_prefill_quant (csrc/attn_prefill_quant.hip), the caches quantised on the CPU: every output element within
attn_prefill_cases.bound of the float64 oracle over dequantize_rows of the same codes (the values the kernel consumes), at shapes on the edges of a row tile of 128 packed
rows and of a key tile of 64; the length from the device in one captured launch; and install_fused_attention(model, prefill="codes_all")."""
import functools

import pytest
import torch

import decode_loop_cases as D
from attn_prefill_cases import DIMS, DTYPES, bound, fp32_error, left_padded, oracle
from test_attn_chunk_modules_gpu import tier_a

import qllm_amd
from qllm_amd import ops
from qllm_amd.modeling.q_layers import install_fused_attention, uninstall_fused_attention
from qllm_amd.modeling.quant_cache import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, LMAX = 2, 200
# (Hq, Hkv, S): G = 1 and two row tiles, the second of 2 rows; G = 4, R = 132; G = 7, R = 133 (the tile edge inside a token); G = 8,
# R = 136; the smallest call
CASES = ((1, 1, 130), (8, 2, 33), (7, 1, 19), (8, 1, 17), (8, 2, 2))
PROMPT, CHUNK, CACHE = 20, 18, 48               # both above SPLIT_MAX_ROWS: the prompt and the chunk are the new route's
tag = lambda dtype: str(dtype)[6:]
lengths = lambda s: (s, s + 63, s + 65, LMAX)   # nothing cached, a key-tile edge on either side, the whole cache


@functools.lru_cache(maxsize=None)
def caches(dtype, d, hk, bits):
    """(k_codes, k_params, v_codes, v_params) of random [B, Hkv, LMAX, D] rows and the (K, V) they dequantise to, on the CPU, computed once."""
    gen = torch.Generator().manual_seed(100 * d + 10 * hk + bits)
    codes = sum((quantize_rows(torch.randn(B, hk, LMAX, d, generator=gen, dtype=torch.float64).to(dtype), bits) for _ in range(2)), ())
    return codes, (dequantize_rows(codes[0], codes[1], bits), dequantize_rows(codes[2], codes[3], bits))


@functools.lru_cache(maxsize=None)
def query(dtype, d, hq, s):
    gen = torch.Generator().manual_seed(1000 * s + hq)
    return torch.randn(B, s, hq, d, generator=gen, dtype=torch.float64).to(dtype).transpose(1, 2)   # the view of the projection output


def masks(kind, dtype, s, n):   # None, or the left-padded mask of a batch whose second row hides every key, bool or additive
    return None if kind is None else left_padded(B, s, n - s, LMAX, [min(7, n - s), LMAX], kind, dtype)


@pytest.mark.parametrize("hq,hk,s", CASES)
@pytest.mark.parametrize("kind", (None, "bool", "additive"))
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("bits", (8, 4))
def test_every_element_lies_within_the_bound_of_the_float64_oracle(bits, dtype, d, kind, hq, hk, s):
    codes, (k, v) = caches(dtype, d, hk, bits)
    dev, q = [t.to(DEV) for t in codes], query(dtype, d, hq, s)
    worst = 0.0
    for n in lengths(s):
        mask = masks(kind, dtype, s, n)
        ref, pv = oracle(q, k, v, n, d ** -0.5, True, mask, weights=True)
        tol = bound(ref, pv, fp32_error(q, k, v, n, d ** -0.5, ref, True, mask), dtype)
        got = ops.attn_prefill_quant(q.to(DEV), *dev, bits, n, mask=None if mask is None else mask.to(DEV))
        err = (got.cpu().double() - ref).abs()
        worst = max(worst, (err / tol).max().item())
        assert bool((err <= tol).all()), (n, (err / tol).max().item(), (err > tol).nonzero()[:4].tolist())
    print(f"attn_prefill_quant bits={bits} {tag(dtype)} d={d} mask={kind} ({hq},{hk},{s}): largest err / bound {worst:.3f}")


@pytest.mark.parametrize("hq,hk,s", ((8, 2, 33), (7, 1, 19)))
@pytest.mark.parametrize("bits", (8, 4))
def test_one_captured_launch_serves_every_length_from_the_device(bits, hq, hk, s):
    dtype, d = torch.float16, 128
    q, md = query(dtype, d, hq, s).to(DEV), masks("bool", dtype, s, LMAX).to(DEV)   # (the mask of the longest call: rows see pads[b] <= j)
    dev = [t.to(DEV) for t in caches(dtype, d, hk, bits)[0]]
    eager = {n: ops.attn_prefill_quant(q, *dev, bits, n, mask=md) for n in lengths(s)}
    length = torch.tensor(LMAX, dtype=torch.int64, device=DEV)
    for n in lengths(s):
        length.fill_(n)
        assert D.same_bits(ops.attn_prefill_quant(q, *dev, bits, length, mask=md), eager[n]), n
    out = torch.zeros(B, s, hq, d, dtype=dtype, device=DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_prefill_quant(q, *dev, bits, length, mask=md, out=out)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.attn_prefill_quant(q, *dev, bits, length, mask=md, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for n in (s + 65, s, LMAX):
        length.fill_(n)
        out.fill_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert D.same_bits(out, eager[n]), n


def pieces(model, inp, cache, device):   # the prompt, the chunk, one decode step: the logits of the chunk and of the step
    ids, pos, mask = inp.ids.to(device), inp.pos.to(device), None if inp.mask is None else inp.mask.to(device)
    out = []
    with torch.no_grad():
        for a, b in ((0, PROMPT), (PROMPT, PROMPT + CHUNK), (PROMPT + CHUNK, PROMPT + CHUNK + 1)):
            out.append(model(ids[:, a:b], attention_mask=None if mask is None else mask[:, :b], position_ids=pos[:, a:b], past_key_values=cache,
                             use_cache=True).logits.cpu())
    return torch.cat(out[1:], dim=1)


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("bits", (8, 4))
def test_codes_all_reads_the_codes_in_place_for_prompt_and_chunk_and_a_refusal_ends_where_codes_does(bits, batch, monkeypatch):
    model, ref = tier_a()
    inp = D.batch_inputs(batch, prompt=PROMPT, steps=CHUNK + 1)
    cache = lambda: qllm_amd.quant_static_cache(model.config, CACHE, bits=bits)
    reference = pieces(ref, inp, D.make_cache(ref, "dynamic"), "cpu")
    unfused = pieces(model, inp, cache(), DEV)
    calls = []
    for name in ("attn_prefill_quant", "attn_prefill", "kv_dequantize"):
        def op(*a, _real=getattr(ops, name), _name=name, **kw):
            calls.append(_name)
            return _real(*a, **kw)
        monkeypatch.setattr(ops, name, op)

    def run(prefill):
        del calls[:]
        assert install_fused_attention(model, prefill=prefill) == D.LAYERS
        try:
            return pieces(model, inp, cache(), DEV), list(calls)
        finally:
            assert uninstall_fused_attention(model) == D.LAYERS

    codes, codes_calls = run("codes")
    got, got_calls = run("codes_all")
    assert got_calls == ["attn_prefill_quant"] * 2 * D.LAYERS, got_calls       # the prompt and the chunk of every layer; no row dequantised
    assert codes_calls.count("kv_dequantize") == 4 * D.LAYERS and "attn_prefill_quant" not in codes_calls
    e_unfused, e_got = (unfused.double() - reference).abs().max().item(), (got.double() - reference).abs().max().item()
    print(f"codes_all modules bits={bits} {batch}: E(unfused) {e_unfused:.3e} E(codes_all) {e_got:.3e} ratio {e_got / e_unfused:.3f}")
    assert e_unfused > 0 and e_got <= D.M_DEVICE * e_unfused

    def refuse(*a, **kw):
        raise ops.QllmUnsupported(0, "refused here")
    monkeypatch.setattr(ops, "attn_prefill_quant_plan", refuse)
    again, again_calls = run("codes_all")
    assert again_calls == codes_calls and D.same_bits(again, codes)
