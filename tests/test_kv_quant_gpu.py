"""-m gpu: the quantized KV cache on the device -- ops.kv_quantize / kv_dequantize (csrc/kv_quant.hip), ops.attn_decode_quant
(csrc/attn_decode_quant.hip) and q_layers/fused_attention.py over modeling/quant_cache.py.

1. The format, exact: quantize then dequantize against the formulas written out here; params and values bit for bit; nothing outside the
   positions of the call is touched.  2. The kernel against the float64 oracle over the float64-dequantised cache, within
   attn_decode_cases.bound of the CPU's own fp32 error: lengths at every split edge, host and device length, with and without the append,
   no / bool / additive mask, NaN params and 0x80 codes behind the length; the appended row's bytes, every other byte, the counter page.
3. ONE captured appending launch replayed from length 0.  4. Refusals before any launch.  5. The modules on a tiny llama."""
import re

import pytest
import torch

import attn_decode_cases as AD
import decode_loop_cases as DL

import qllm_amd
from qllm_amd import ops
from qllm_amd.modeling.q_layers import install_fused_attention, uninstall_fused_attention

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BITS = (8, 4)
quant = pytest.mark.parametrize("bits", BITS, ids=["8bit", "4bit"])
types = pytest.mark.parametrize("dtype", AD.DTYPES, ids=["float16", "bfloat16"])
dims = pytest.mark.parametrize("d", AD.DIMS, ids=["D64", "D128"])


def dev_int(n):
    return torch.tensor(n, dtype=torch.int64, device=DEV)


def formulas(x, bits):
    """The issue's formulas: x [..., D] of an act type -> (codes [..., D] float32 integers, s, z [..., D / 32] of x's type; z zeros at 8 bits)."""
    dtype = x.dtype
    g = x.float().unflatten(-1, (-1, 32))
    if bits == 8:
        s = (g.abs().amax(-1) / 127.0).to(dtype)
        z = torch.zeros_like(s)
        c = torch.round(g / s.float()[..., None]).clamp(-127, 127)
    else:
        z = g.amin(-1).to(dtype)
        s = ((g.amax(-1) - g.amin(-1)) / 15.0).to(dtype)
        c = torch.round((g - z.float()[..., None]) / s.float()[..., None]).clamp(0, 15)
    return torch.where(s[..., None] == 0, torch.zeros_like(c), c), s, z


def values64(c, s, z):
    """[..., D] float64: z + code * s, exact."""
    return (z.double()[..., None] + c.double() * s.double()[..., None]).flatten(-2)


def params_of(s, z, bits):
    return s if bits == 8 else torch.cat((s, z), dim=-1)


def empty_cache(b, hk, L, d, bits, dtype, codes=0, params=0.0):
    nbytes, nparams = ops.kv_quant_shapes(d, bits)
    return (torch.full((b, hk, L, nbytes), codes, dtype=torch.uint8, device=DEV), torch.full((b, hk, L, nparams), params, dtype=dtype, device=DEV))


# ---- 1. the format ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("rows", [1, 37])
@dims
@types
@quant
def test_format_is_exact(bits, dtype, d, rows, pos0, on_device):
    b, hk, L = 2, 2, 48
    x = torch.randn((b, rows, hk, d), generator=torch.Generator().manual_seed(rows + d))
    x[:, :, 1] *= 300                      # a large_v-sized range
    x[:, :, 0, :32] = 0                    # a constant group: s == 0
    x[:, :, 1, :32] = 1.5                  # constant and not zero: s == 0 with a zero at 4 bits
    x[:, :, 0, 40] = -9                    # a group whose largest magnitude is negative
    x = x.to(dtype)
    src = x.to(DEV).transpose(1, 2)        # the [B, S, H, D] view of the projections, read in place
    codes, params = empty_cache(b, hk, L, d, bits, dtype, 0xA5, 1.25)
    ops.kv_quantize(src, codes, params, bits, dev_int(pos0) if on_device else pos0)
    c, s, z = formulas(x.transpose(1, 2), bits)
    inside = slice(pos0, pos0 + rows)
    assert torch.equal(params[:, :, inside].cpu().view(torch.int16), params_of(s, z, bits).view(torch.int16))
    outside = torch.ones(L, dtype=torch.bool)
    outside[inside] = False
    assert bool((codes.cpu()[:, :, outside] == 0xA5).all()) and bool((params.cpu()[:, :, outside] == 1.25).all())
    n = pos0 + rows
    out = torch.full((b, hk, L, d), 7.0, dtype=dtype, device=DEV)
    ops.kv_dequantize(codes, params, bits, dev_int(n) if on_device else n, out)
    want = values64(c, s, z).float().to(dtype)
    assert torch.equal(out[:, :, inside].cpu().view(torch.int16), want.view(torch.int16))
    assert bool((out[:, :, n:] == 7.0).all())


# ---- 2. the kernel against float64 -----------------------------------------------------------------------------------------------------------------
def quant_geometry(b, hq, hk, d, bits):
    def parse(n):
        return {k: int(v) for k, v in re.findall(r"(tile|splits|chunk)=(\d+)", ops.attn_decode_quant_describe(b, hq, hk, d, bits, n))}
    g0 = parse(1024)
    lmax = min(g0["splits"] * g0["tile"] + 3, 2051)
    g = parse(lmax)
    assert g["splits"] >= 3 and (g["splits"] - 1) * g["chunk"] < lmax <= g["splits"] * g["chunk"], g
    return lmax, g


def counters_are_zero():
    return int(ops.workspace(torch.device(DEV), 0)[:16384].count_nonzero()) == 0


@pytest.mark.parametrize("family", ["peaked", "large_v"])
@pytest.mark.parametrize("b", AD.BATCHES, ids=["B1", "B3"])
@pytest.mark.parametrize("hq,hk", [(1, 1), (8, 2), (7, 1), (8, 1)])
@dims
@types
@quant
def test_kernel_against_float64(bits, dtype, d, hq, hk, b, family):
    lmax, g = quant_geometry(b, hq, hk, d, bits)
    q, k, v, scaling = AD.FAMILIES[family](b, hq, hk, d, lmax, dtype, torch.Generator().manual_seed(17 * hq + d + bits))
    (kc, ks, kz), (vc, vs, vz) = formulas(k, bits), formulas(v, bits)
    k64, v64 = values64(kc, ks, kz), values64(vc, vs, vz)
    k32, v32 = ((z.float()[..., None] + c * s.float()[..., None]).flatten(-2) for c, s, z in ((kc, ks, kz), (vc, vs, vz)))
    master = empty_cache(b, hk, lmax, d, bits, dtype) + empty_cache(b, hk, lmax, d, bits, dtype)   # k codes, k params, v codes, v params
    ops.kv_quantize(k.to(DEV), master[0], master[1], bits, 0)
    ops.kv_quantize(v.to(DEV), master[2], master[3], bits, 0)
    qd, kd, vd = q.to(DEV)[:, :, None], k.to(DEV), v.to(DEV)
    gen = torch.Generator().manual_seed(5)
    worst = 0.0
    for n in AD.reduced_lengths(lmax, g):
        visible = torch.rand((b, lmax), generator=gen) > 0.25            # holes
        visible[:, n - 1] = True
        if b > 1:
            visible[b - 1] = False                                          # one fully hidden row: zeros
        shown = visible.clone()
        if b > 1:
            shown[b - 1] = True                                             # (the oracle's row for it: all keys, then set to zero)
        extra = torch.where(torch.rand((b, lmax), generator=gen) > 0.5, -1.5, 0.0)
        masks = {"none": (None, None, None), "bool": (visible, shown, None),
                 "additive": (torch.where(visible, extra, torch.finfo(dtype).min).to(dtype), shown, extra.to(dtype).double())}
        for kind, (mask, vis, bias) in masks.items():
            want = AD.oracle(q, k64, v64, n, scaling, vis, bias)
            as_restated = None if mask is None else vis if bias is None else torch.where(vis, bias.float(), float("-inf"))
            e32, _ = AD.fp32_error(q, k32, v32, n, scaling, want, as_restated)
            if mask is not None and b > 1:
                want[b - 1] = 0
            tol = AD.bound(want, e32, dtype)
            for on_device in (False, True):
                for append in (False, True):
                    at = n - 1 if append else n                             # the length handed in; the call sees n positions either way
                    cache = [t.clone() for t in master]
                    for t in cache:
                        t[:, :, at:] = float("nan") if t.dtype == dtype else 0x80
                    before = [t.clone() for t in cache]
                    new = dict(k_new=kd[:, :, n - 1:n], v_new=vd[:, :, n - 1:n]) if append else {}
                    got = ops.attn_decode_quant(qd, *cache, bits, dev_int(at) if on_device else at, mask=None if mask is None else mask.to(DEV),
                                                scaling=scaling, **new)
                    err = (got.cpu().double() - want).abs()
                    worst = max(worst, (err / tol).max().item())
                    assert bool((err <= tol).all()), (n, kind, on_device, append, (err / tol).max().item())
                    if mask is not None and b > 1:
                        assert int(got[b - 1].count_nonzero()) == 0
                    for t, t0, m in zip(cache, before, master):
                        if append:
                            assert torch.equal(t[:, :, at], m[:, :, at])        # the bytes kv_quantize writes for that row
                            t[:, :, at] = t0[:, :, at]
                        assert torch.equal(t.view(torch.uint8), t0.view(torch.uint8))   # (NaN params: compared as bytes)
                    assert counters_are_zero()
    # the length on the device at L_max with an append: nothing is stored, the first L_max positions are attended
    cache = [t.clone() for t in master]
    got = ops.attn_decode_quant(qd, *cache, bits, dev_int(lmax), k_new=kd[:, :, :1], v_new=vd[:, :, :1], scaling=scaling)
    assert torch.equal(got, ops.attn_decode_quant(qd, *master, bits, lmax, scaling=scaling)) and all(torch.equal(t, m) for t, m in zip(cache, master))
    print(f"attn_decode_quant {bits}bit {dtype} D{d} {hq}x{hk} B{b} {family}: worst error / bound {worst:.3f}")


# ---- 3. one captured appending launch ----------------------------------------------------------------------------------------------------------------
@dims
@types
@quant
def test_one_captured_launch_serves_every_length(bits, dtype, d):
    b, hq, hk = 2, 4, 2
    lmax, g = quant_geometry(b, hq, hk, d, bits)
    steps = g["tile"] + 3
    gen = torch.Generator().manual_seed(11)
    qs, ks, vs = (torch.randn((steps, b, h, 1, d), generator=gen).to(dtype).to(DEV) for h in (hq, hk, hk))

    def stepping(call):
        cache = empty_cache(b, hk, lmax, d, bits, dtype) + empty_cache(b, hk, lmax, d, bits, dtype)
        length, q, k, v, out = dev_int(0), qs[0].clone(), ks[0].clone(), vs[0].clone(), torch.empty((b, hq, d), dtype=dtype, device=DEV)
        step = call(cache, length, q, k, v, out)
        outs = []
        for i in range(steps):
            q.copy_(qs[i]), k.copy_(ks[i]), v.copy_(vs[i])
            step()
            outs.append(out.clone())
        assert int(length) == steps
        return torch.stack(outs), cache

    def eager(cache, length, q, k, v, out):
        def step():
            ops.attn_decode_quant(q, *cache, bits, length, k_new=k, v_new=v, out=out)
            length.add_(1)
        return step

    def captured(cache, length, q, k, v, out):
        eager(cache, length, q, k, v, out)()           # the workspace exists before the capture
        length.zero_()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            eager(cache, length, q, k, v, out)()
        length.zero_()
        return graph.replay

    want, want_cache = stepping(eager)
    got, got_cache = stepping(captured)
    assert torch.equal(got, want) and all(torch.equal(a, c) for a, c in zip(got_cache, want_cache)) and counters_are_zero()


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["bits", "head_dim", "group", "params pointer", "mask"])
def test_refusals_leave_the_cache_alone(what):
    bits, d, hq, hk, L, dtype = (3 if what == "bits" else 8), (96 if what == "head_dim" else 64), (9 if what == "group" else 4), (1 if what == "group" else 2), 64, torch.float16
    shape_bits = 8 if what == "bits" else bits
    cache = [torch.full((1, hk, L, n), fill, dtype=t, device=DEV) for n, fill, t in ((d * shape_bits // 8, 0x5A, torch.uint8), (max(d // 32, 1) + 2, 1.0, dtype)) * 2]
    tensors = [t if t.dtype == torch.uint8 else t[..., :max(d // 32, 1)] for t in cache]
    if what == "params pointer":
        tensors[1] = cache[1].flatten()[1:1 + 2 * hk * L].view(1, hk, L, 2)     # two bytes off a 4-byte boundary
        assert tensors[1].data_ptr() % 4 == 2
    q, k = (torch.ones((1, h, 1, d), dtype=dtype, device=DEV) for h in (hq, hk))
    mask = torch.ones((1, 1, 1, 3), dtype=torch.bool, device=DEV) if what == "mask" else None
    before = [t.clone() for t in cache]
    with pytest.raises(ops.QllmUnsupported):
        ops.attn_decode_quant(q, *tensors, bits, 7, k_new=k, v_new=k, mask=mask)
    assert all(torch.equal(t, t0) for t, t0 in zip(cache, before))


# ---- 5. the modules ------------------------------------------------------------------------------------------------------------------------------------
@types
@quant
def test_modules_decode_on_the_quantized_cache(bits, dtype, monkeypatch):
    import transformers
    torch.manual_seed(0)
    model = transformers.LlamaForCausalLM(DL.llama_config(str(dtype)[6:])).to(dtype).eval()
    reference, inp = DL.float64_copy(model), DL.batch_inputs("padded")
    ref = DL.run(reference, inp)
    model = model.to(DEV)

    def fresh():
        return qllm_amd.quant_static_cache(model.config, DL.MAX_CACHE_LEN, bits=bits)

    unfused = DL.run(model, inp, fresh(), DEV)          # `update` alone: what QLLM_FUSE_ATTENTION=0 leaves
    monkeypatch.setenv("QLLM_FUSE_ATTENTION", "0")
    assert install_fused_attention(model) == 0
    monkeypatch.delenv("QLLM_FUSE_ATTENTION")
    calls = {"attn": 0, "dequant": 0}
    for name, op in (("attn", "attn_decode_quant"), ("dequant", "kv_dequantize")):
        monkeypatch.setattr(ops, op, lambda *a, _n=name, _real=getattr(ops, op), **kw: (calls.__setitem__(_n, calls[_n] + 1), _real(*a, **kw))[1])
    assert install_fused_attention(model) == DL.LAYERS
    try:
        fused = DL.run(model, inp, fresh(), DEV, calls)
        assert fused.at_prefill == {"attn": 0, "dequant": 2 * DL.LAYERS}
        assert calls == {"attn": DL.LAYERS * inp.steps, "dequant": 2 * DL.LAYERS}      # one kernel per layer and step, no row dequantised at decode
        e_unfused, e_fused = DL.error(unfused, ref), DL.error(fused, ref)
        print(f"quant cache {bits}bit {dtype}: E(update) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
        assert DL.same_bits(fused.prefill, unfused.prefill)
        assert e_unfused > 0 and e_fused <= DL.M_DEVICE * e_unfused
        # reset, then reuse: the bits of a fresh cache.  crop: the last three steps again
        fused.cache.reset()
        again = DL.run(model, inp, fused.cache, DEV)
        DL.assert_same_logits(again.steps, fused.steps, "reset")
        again.cache.crop(-3)                       # as transformers' assisted generation calls it: the last three tokens go
        ids, pos, mask = inp.ids.to(DEV), inp.pos.to(DEV), inp.mask.to(DEV)
        last = inp.prompt + inp.steps
        with torch.no_grad():
            tail = [model(ids[:, i:i + 1], attention_mask=mask[:, :i + 1], position_ids=pos[:, i:i + 1], past_key_values=again.cache, use_cache=True).logits[:, -1]
                    for i in range(last - 3, last)]
        DL.assert_same_logits(torch.stack(tail).cpu(), fused.steps[-3:], "crop")
    finally:
        uninstall_fused_attention(model)
