"""-m gpu: ops.attn_chunk_quant (csrc/attn_chunk_quant.hip) on test_attn_chunk_gpu's shapes, the caches quantised on the CPU: bit identity with
ops.attn_chunk over ops.kv_dequantize of the same codes, and attn_prefill_cases.bound against the float64 oracle over dequantize_rows."""
import functools

import pytest
import torch

import decode_loop_cases as D
from attn_prefill_cases import DIMS, DTYPES, GROUPS, bound, fp32_error, left_padded, oracle
from test_attn_chunk_gpu import COUNTER_BYTES, LMAX, Q_LENS, geometry, lengths, same, tag
from test_attn_chunk_modules_gpu import CHUNK, pieces, tier_a

import qllm_amd
from qllm_amd import ops
from qllm_amd.modeling.q_layers import fused_attention, install_fused_attention, uninstall_fused_attention
from qllm_amd.modeling.quant_cache import dequantize_rows, quantize_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B = 3
BITS = (8, 4)


@functools.lru_cache(maxsize=None)
def caches(dtype, d, hk, bits):
    """(k_codes, k_params, v_codes, v_params) of random [B, Hkv, LMAX, D] rows, on the CPU: computed once and left unchanged."""
    gen = torch.Generator().manual_seed(100 * d + 10 * hk + bits)
    return sum((quantize_rows(torch.randn(B, hk, LMAX, d, generator=gen, dtype=torch.float64).to(dtype), bits) for _ in range(2)), ())


@functools.lru_cache(maxsize=None)
def query(dtype, d, hq, s):
    gen = torch.Generator().manual_seed(1000 * s + hq)
    return torch.randn(B, s, hq, d, generator=gen, dtype=torch.float64).to(dtype).transpose(1, 2)   # the view of the projection output


def masks(kind, dtype, s, n):
    """None, or test_attn_chunk_gpu's left-padded mask (batch row 1 hides every key) as bool or additive."""
    if kind is None:
        return None
    m = left_padded(B, s, n - s, LMAX, [min(7, n - s), LMAX, 0], "bool", dtype)
    return m if kind == "bool" else torch.where(m, torch.zeros((), dtype=dtype), torch.full((), torch.finfo(dtype).min, dtype=dtype))


@pytest.mark.parametrize("kind", (None, "bool", "additive"))
@pytest.mark.parametrize("hq,hk", GROUPS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("bits", BITS)
def test_the_bits_are_attn_chunks_over_the_dequantised_cache(bits, dtype, d, hq, hk, kind):
    """Any wrong nibble, group, scale / zero index or row stride changes bits.  Once more with the partials full of NaN; counters zero."""
    kc, kp, vc, vp = (t.to(DEV) for t in caches(dtype, d, hk, bits))
    kd, vd = (ops.kv_dequantize(c, p, bits, LMAX, torch.zeros(B, hk, LMAX, d, dtype=dtype, device=DEV)) for c, p in ((kc, kp), (vc, vp)))
    for s in Q_LENS[(hq, hk)]:
        g = geometry(B, hq, hk, d, s)
        assert ops.attn_chunk_quant_describe(B, hq, hk, d, bits, s, LMAX) == ops.attn_chunk_describe(B, hq, hk, d, s, LMAX).replace("attn_chunk ", f"attn_chunk_quant bits={bits} ")
        q = query(dtype, d, hq, s).to(DEV)
        for n in lengths(g, s):
            mask = masks(kind, dtype, s, n)
            md = None if mask is None else mask.to(DEV)
            want = ops.attn_chunk(q, kd, vd, n, mask=md)
            assert same(ops.attn_chunk_quant(q, kc, kp, vc, vp, bits, n, mask=md), want), (s, n)
            nbytes = ops._lib.load().qllm_attn_chunk_workspace_bytes(B, hq, hk, d, s, LMAX)
            ws = ops.workspace(torch.device(DEV), nbytes)
            ws[COUNTER_BYTES:nbytes].view(torch.float32).fill_(float("nan"))
            assert same(ops.attn_chunk_quant(q, kc, kp, vc, vp, bits, torch.tensor(n, dtype=torch.int64, device=DEV), mask=md), want), (s, n)
            assert not bool(ws[:COUNTER_BYTES].any()), (s, n)


@pytest.mark.parametrize("d,hq,hk", ((128, 8, 2), (64, 7, 1)))
@pytest.mark.parametrize("dtype", DTYPES, ids=tag)
@pytest.mark.parametrize("bits", BITS)
def test_every_element_lies_within_the_bound_of_the_float64_oracle(bits, dtype, d, hq, hk):
    """The kernel consumes exactly the act-rounded values dequantize_rows gives, so attn_prefill_cases.bound applies as it stands."""
    cpu = caches(dtype, d, hk, bits)
    k, v = dequantize_rows(cpu[0], cpu[1], bits), dequantize_rows(cpu[2], cpu[3], bits)
    dev = [t.to(DEV) for t in cpu]
    worst = 0.0
    for s in Q_LENS[(hq, hk)]:
        q = query(dtype, d, hq, s)
        for n in lengths(geometry(B, hq, hk, d, s), s):
            mask = masks("bool", dtype, s, n)
            ref, pv = oracle(q, k, v, n, d ** -0.5, True, mask, weights=True)
            tol = bound(ref, pv, fp32_error(q, k, v, n, d ** -0.5, ref, True, mask), dtype)
            err = (ops.attn_chunk_quant(q.to(DEV), *dev, bits, n, mask=mask.to(DEV)).cpu().double() - ref).abs()
            worst = max(worst, (err / tol).max().item())
            assert bool((err <= tol).all()), (s, n, (err / tol).max().item(), (err > tol).nonzero()[:4].tolist())
    print(f"attn_chunk_quant bits={bits} {tag(dtype)} d={d} ({hq},{hk}): largest err / bound {worst:.3f}")


@pytest.mark.parametrize("bits", BITS)
def test_one_captured_launch_serves_lengths_on_both_sides_of_a_chunk_boundary(bits):
    dtype, d, hq, hk, s = torch.float16, 128, 8, 2, 9
    g = geometry(B, hq, hk, d, s)
    q, md = query(dtype, d, hq, s).to(DEV), masks("bool", dtype, s, LMAX).to(DEV)
    dev = [t.to(DEV) for t in caches(dtype, d, hk, bits)]
    length = torch.tensor(LMAX, dtype=torch.int64, device=DEV)
    out = torch.zeros(B, s, hq, d, dtype=dtype, device=DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_chunk_quant(q, *dev, bits, length, mask=md, out=out)      # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.attn_chunk_quant(q, *dev, bits, length, mask=md, out=out)
    torch.cuda.current_stream().wait_stream(side)
    for at in (g["chunk"], g["chunk"] + 1, s, 3 * g["chunk"] - 1, LMAX, g["chunk"] + 1):
        length.fill_(at)
        out.fill_(1.0)
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, ops.attn_chunk_quant(q, *dev, bits, at, mask=md)), at


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("bits", BITS)
def test_codes_sends_the_masked_chunk_over_the_codes_and_a_refusal_where_split_takes_it(bits, batch, monkeypatch):
    model, ref = tier_a()
    inp = D.batch_inputs(batch, steps=CHUNK + 1)
    cache = lambda: qllm_amd.quant_static_cache(model.config, D.MAX_CACHE_LEN, bits=bits)
    reference = pieces(ref, inp, D.make_cache(ref, "dynamic"), "cpu")
    unfused = pieces(model, inp, cache(), DEV)
    calls = []
    for name in ("attn_chunk_quant", "attn_chunk", "kv_dequantize"):
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

    split, split_calls = run("split")
    codes, codes_calls = run("codes")
    # the prompt dequantises (two launches per layer through `update`) either way; the chunk and the decode step of "codes" do not
    assert codes_calls == ["kv_dequantize"] * 2 * D.LAYERS + ["attn_chunk_quant"] * D.LAYERS, codes_calls
    assert split_calls.count("attn_chunk") == D.LAYERS and split_calls.count("kv_dequantize") == 4 * D.LAYERS
    e_unfused, e_codes = (unfused.double() - reference).abs().max().item(), (codes.double() - reference).abs().max().item()
    print(f"codes modules bits={bits} {batch}: E(unfused) {e_unfused:.3e} E(codes) {e_codes:.3e} ratio {e_codes / e_unfused:.3f}")
    assert e_unfused > 0 and e_codes <= D.M_DEVICE * e_unfused
    assert D.same_bits(codes, split)                                   # the same values reach the same MFMAs

    def refuse(*a, **kw):
        raise ops.QllmUnsupported(0, "refused here")
    monkeypatch.setattr(ops, "attn_chunk_quant_plan", refuse)
    again, again_calls = run("codes")
    assert again_calls == split_calls and D.same_bits(again, split)
