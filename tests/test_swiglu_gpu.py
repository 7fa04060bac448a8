"""-m gpu: the fused SwiGLU down-projection (qllm_linear_forward_swiglu, csrc/strip1_swiglu.hip: the SWIGLU forms of the batch-1 kernel)
through the C ABI and the modules -- every form of the kernel's shape table in fp16 and bf16.

The arithmetic contract is bit identity with the plain launch on x = act(gate) * up.  It is pinned independently of any `exp`: for gates
in {0} u {20..40}, silu(g) == g exactly (1 + exp(-g) rounds to 1 in fp32), so `linear_forward_swiglu(w, g, u)` must equal
`linear_forward(w, F.silu(g) * u)` bit for bit whatever the device's expf does.  Random gates are held to the project's tolerances against
the oracle (tests/test_strip1_gpu.py) and the share of outputs that differ from the unfused launch is printed, not asserted.

Measured on an MI355X (the printed shares, random gates of both signs, all 278 cells): 0.00000 everywhere -- DESIGN 3.10."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from gpu_util import Ref, guarded, randx, synth, to_layer
from test_strip1_gpu import B3_FORMS, FORMS, G64_FORMS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float16, torch.bfloat16)
SENTINEL = 0x7E5A   # an fp16 / bf16 NaN nobody computes (tests/test_bitgemv_group_gpu.py)

# (kind, K, N): every K of the three form lists at N = 256 (16 strips: one block per CU at most) and, for K <= 4096, at N = 8192 too (more
# strips than CUs: the wide-launch forms of those K)
KINDS = {"w4": (4, 128), "g64": (4, 64), "b3": (3, 128), "b3g64": (3, 64)}
NW16 = "+nw16"   # a kind with this suffix: the case runs with QLLM_S1_T256_NW16 = 1, which the (16, 16) pair of the shape table needs
KINDS.update({kind + NW16: v for kind, v in list(KINDS.items())})


def _cases():
    out = []
    for kind, forms in (("w4", FORMS), ("g64", G64_FORMS), ("b3", B3_FORMS), ("b3g64", B3_FORMS)):
        for K, _ in forms:
            out.append((kind, K, 256))
            if K <= 4096:
                out.append((kind, K, 8192))
    return out


# (kind, K, N, the plan line's form): one case for every form of csrc/strip1_forms.hpp's table that the three lists do not plan to -- N = 256,
# or 8192 for the pairs taken on wide launches only; K = 32 NW MAXS for an exact form, a K of the lists (or the smallest) for a shifted one.
# With these every SWIGLU and every RESID form is launched here and in tests/test_residual_gpu.py, and its plain twin next to it.
MORE = [("b3", 256, 256, "nw=4 round=8 bits=3 grid"), ("b3g64", 256, 256, "nw=4 round=8 g64 bits=3 grid"), ("b3", 1152, 256, "nw=4 round=16 bits=3 grid"),
        ("g64", 1152, 256, "nw=4 round=16 g64 grid"), ("b3g64", 1152, 256, "nw=4 round=16 g64 bits=3 grid"), ("w4", 3200, 8192, "nw=7 round=16 grid"),
        ("b3", 3200, 8192, "nw=7 round=16 bits=3 grid"), ("g64", 3200, 8192, "nw=7 round=16 g64 grid"), ("b3g64", 3200, 8192, "nw=7 round=16 g64 bits=3 grid"),
        ("b3", 3840, 8192, "nw=8 round=16 bits=3 grid"), ("g64", 3840, 8192, "nw=8 round=16 g64 grid"), ("b3g64", 3840, 8192, "nw=8 round=16 g64 bits=3 grid"),
        ("b3", 6144, 256, "nw=8 round=24 exact bits=3 grid"), ("g64", 6144, 256, "nw=8 round=24 exact g64 grid"), ("b3g64", 6144, 256, "nw=8 round=24 exact g64 bits=3 grid"),
        ("b3", 6656, 256, "nw=8 round=32 bits=3 grid"), ("g64", 6656, 256, "nw=8 round=32 g64 grid"), ("b3g64", 6656, 256, "nw=8 round=32 g64 bits=3 grid"),
        ("w4", 11520, 256, "nw=15 round=24 exact grid"), ("b3", 11520, 256, "nw=15 round=24 exact bits=3 grid"), ("g64", 11520, 256, "nw=15 round=24 exact g64 grid"),
        ("b3g64", 11520, 256, "nw=15 round=24 exact g64 bits=3 grid"), ("w4+nw16", 6656, 256, "nw=16 round=16 grid"), ("b3+nw16", 6656, 256, "nw=16 round=16 bits=3 grid"),
        ("g64+nw16", 6656, 256, "nw=16 round=16 g64 grid"), ("b3g64+nw16", 6656, 256, "nw=16 round=16 g64 bits=3 grid"), ("w4+nw16", 8192, 256, "nw=16 round=16 exact grid"),
        ("b3+nw16", 8192, 256, "nw=16 round=16 exact bits=3 grid"), ("g64+nw16", 8192, 256, "nw=16 round=16 exact g64 grid"), ("b3g64+nw16", 8192, 256, "nw=16 round=16 exact g64 bits=3 grid"),
        ("b3", 11776, 256, "nw=16 round=24 bits=3 grid"), ("g64", 11776, 256, "nw=16 round=24 g64 grid"), ("b3g64", 11776, 256, "nw=16 round=24 g64 bits=3 grid"),
        ("b3", 12288, 256, "nw=16 round=24 exact bits=3 grid"), ("g64", 12288, 256, "nw=16 round=24 exact g64 grid"), ("b3g64", 12288, 256, "nw=16 round=24 exact g64 bits=3 grid"),
        ("g64", 16384, 256, "nw=16 round=32 exact g64 grid"), ("g64", 20480, 256, "nw=16 round=40 exact g64 grid"), ("g64", 22016, 256, "nw=16 round=48 g64 grid"),
        ("w4", 28800, 256, "nw=16 round=64 grid")]
CASES = _cases() + [c[:3] for c in MORE]
FORM_OF = {c[:3]: c[3] for c in MORE}
# zero points / bias / layout rotate over the cases (the staging under test does not depend on them); test_zero_kinds_and_bias crosses them
VARIANTS = (("GPTQ", "asym", False), ("HQQ", "asym", True), ("GPTQ", "sym", True), ("HQQ", "asym", False), ("GPTQ", "asym", True), ("GPTQ", "sym", False))


def _native(layer, d, zk, compat=0):
    from qllm_amd import ops
    if zk == "sym":
        layer._descriptor(None, 0)
        src = ops.make_weight("GPTQ", layer.qweight, layer.scales, None, None, layer.bias, d["K"], d["N"], d["groupsize"], d["bits"], compat)
        return ops.repack_native(*src)[0:2]
    return layer.native_descriptor(compat), None


@functools.lru_cache(maxsize=None)
def _layer(kind, K, N, variant=None, compat=0):
    """(synth dict, q_layer, native descriptor, keepalive): built once per case and shared by the tests below."""
    bits, g = KINDS[kind]
    layout, zk, bias = VARIANTS[(CASES.index((kind, K, N)) if variant is None else variant) % len(VARIANTS)]
    d = synth(layout, bits, g, K, N, zk, False, bias, seed=K + N + g + bits)
    d["scales"] = (d["scales"].astype(np.float32) * (4096 / K) ** 0.5 * 0.5).astype(np.float16)
    d["compat"] = compat
    layer = to_layer(d, DEV)
    w, keep = _native(layer, d, zk, compat)
    return d, layer, w, keep


def _rows(kind, K):
    return (1, 2, 3, 4) if KINDS[kind] == (4, 128) and K <= 16384 else (1,)


@pytest.fixture(autouse=True)
def nw16_cases(request):
    """QLLM_S1_T256_NW16 = 1 for the length of a test whose `kind` carries the suffix."""
    from qllm_amd import ops
    kind = request.node.callspec.params.get("kind", "") if hasattr(request.node, "callspec") else ""
    if not str(kind).endswith(NW16):
        yield
        return
    ops.set_knob("QLLM_S1_T256_NW16", 1)
    try:
        yield
    finally:
        ops.reset_knobs()


def _exact_gates(m, K, dtype, seed):
    """Gates in {0} u {20..40}: silu(g) == g exactly in fp32; every value is an fp16 and a bf16 number."""
    rng = np.random.default_rng(seed)
    vals = np.concatenate([[0.0], np.arange(20.0, 41.0)]).astype(np.float32)
    return torch.from_numpy(vals[rng.integers(0, len(vals), size=(m, K))]).to(dtype)


def _check_plan(w, m):
    from qllm_amd import ops
    plan = ops.plan_describe([w], m)
    assert plan.startswith("strip1 "), plan
    assert ops.swiglu_describe(w, m) == "swiglu " + plan   # the same (nw, round, grid / exact) as the plain call
    return plan


def test_silu_is_the_identity_on_the_exact_gates():
    """The premise of the bit-identity test, checked on the CPU in both activation types."""
    vals = torch.cat([torch.zeros(1), torch.arange(20.0, 41.0)])
    for dtype in DTYPES:
        g = vals.to(dtype)
        assert torch.equal(g.float(), vals)                      # representable
        assert torch.equal(F.silu(g), g)                         # torch's eager silu in that type
        assert torch.equal(g.float() / (1 + torch.exp(-g.float())), vals)   # ... and the fp32 expression itself


@pytest.mark.parametrize("kind,K,N", CASES)
def test_bit_identity_with_the_unfused_launch(kind, K, N):
    """linear_forward_swiglu(w, g, u) == linear_forward(w, silu(g) * u), bit for bit, on gates where silu is exact: pins the staging --
    windows, the shifted last window, xkeep, row strides at M > 1, the odd wave counts, 1..4 chunks per lane."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    for m in _rows(kind, K):
        assert FORM_OF.get((kind, K, N), "").replace(" grid", " rows=4 grid" if m > 1 else " grid") in _check_plan(w, m)
        for dtype in DTYPES:
            g = _exact_gates(m, K, dtype, seed=K + m).to(DEV)
            u = (torch.from_numpy(randx(m, K, seed=K + 7 * m)) / 16).to(dtype).to(DEV)
            x = F.silu(g) * u
            assert x.dtype == dtype
            fused = ops.linear_forward_swiglu(w, g, u)
            plain = ops.linear_forward(w, x)
            assert fused.dtype == dtype and fused.shape == (m, N)
            assert bool(torch.isfinite(plain.float()).all())
            assert torch.equal(fused, plain), (kind, K, N, m, dtype, int((fused != plain).sum()))


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_zero_kinds_and_bias(variant):
    """Packed, fp16 and symmetric zero points, with and without bias, on the K = 11008 form (15 waves x 24, shifted last window) at 1 and 3
    rows, and with the AutoGPTQ offset on the packed case."""
    from qllm_amd import ops
    K, N = 11008, 256
    layout, zk, _ = VARIANTS[variant]
    for compat in ((0, 1) if (layout, zk) == ("GPTQ", "asym") else (0,)):
        d, layer, w, keep = _layer("w4", K, N, variant, compat)
        assert w.add_zero_bias == compat
        for m in (1, 3):
            _check_plan(w, m)
            for dtype in DTYPES:
                g = _exact_gates(m, K, dtype, seed=variant + m).to(DEV)
                u = (torch.from_numpy(randx(m, K, seed=variant + 11 * m)) / 16).to(dtype).to(DEV)
                assert torch.equal(ops.linear_forward_swiglu(w, g, u), ops.linear_forward(w, F.silu(g) * u)), (variant, compat, m, dtype)
    if (layout, zk) == ("GPTQ", "asym"):   # the offset is really applied: against the oracle with compat = 1
        x = randx(1, K, seed=5)
        g = torch.from_numpy(x).to(DEV) * 2
        u = torch.from_numpy(randx(1, K, seed=6)).to(DEV)
        xt = (F.silu(g) * u).cpu().numpy()
        assert O.rel_err(ops.linear_forward_swiglu(w, g, u).cpu().numpy(), Ref(d).y16(xt)) <= 1e-2


@pytest.mark.parametrize("kind,K,N", CASES)
def test_random_gates_vs_oracle(kind, K, N, capsys):
    """Gates of both signs (randx * 2): against the oracle on x_t = silu(g) * u as torch computes it on the device in the activation type,
    with the tolerances of tests/test_strip1_gpu.py.  Prints the share of outputs that are not the unfused launch's bits."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    ref = Ref(d)
    for m in _rows(kind, K)[::3]:   # 1 row, and 4 where the four-row forms serve
        for dtype in DTYPES:
            g = (torch.from_numpy(randx(m, K, seed=3 * m)) * 2).to(dtype).to(DEV)
            u = torch.from_numpy(randx(m, K, seed=3 * m + 1)).to(dtype).to(DEV)
            xt = F.silu(g) * u
            y = ops.linear_forward_swiglu(w, g, u)
            differ = float((y != ops.linear_forward(w, xt)).float().mean())
            with capsys.disabled():
                print(f"\nswiglu differ-share kind={kind} K={K} N={N} M={m} {str(dtype)[6:]}: {differ:.5f}", end="")
            xn = xt.float().cpu().numpy().astype(np.float16)   # (bf16: the kernel stages fp16 -- what test_strip1_gpu.py compares with)
            yn = y.float().cpu().numpy()
            assert np.isfinite(yn).all()
            e16 = O.rel_err(yn, ref.y16(xn))
            e64 = O.rel_err(yn.astype(np.float64), ref.y64(xn))
            assert e16 <= 1e-2, (kind, K, N, m, dtype, e16)
            assert e64 <= (2e-3 if dtype == torch.float16 else 2e-2), (kind, K, N, m, dtype, e64)


GUARD_CASES = [("w4", 256, 256, 1), ("w4", 11008, 256, 1), ("w4", 11008, 256, 3), ("w4", 4096, 8192, 2), ("w4", 14336, 256, 4), ("g64", 5120, 256, 1),
               ("b3", 11008, 256, 1), ("b3g64", 3584, 8192, 1), ("w4", 32768, 256, 1)]


@pytest.mark.parametrize("kind,K,N,m", GUARD_CASES)
def test_reads_and_writes_stay_inside_their_tensors(kind, K, N, m):
    """gate, up and y carved out of larger buffers: NaN bands around the activations, sentinel bands around y.  A read outside [M, K] of
    either input puts a NaN into the result; a store outside [M, N] changes a band."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    for dtype in DTYPES:
        g0 = (torch.from_numpy(randx(m, K, seed=m)) * 2).to(dtype).to(DEV)
        u0 = torch.from_numpy(randx(m, K, seed=m + 1)).to(dtype).to(DEV)
        gbuf, g = guarded(g0)
        ubuf, u = guarded(u0)
        band = 2048
        ybuf = torch.full((band + m * N + band,), SENTINEL, dtype=torch.int16, device=DEV)
        y = ybuf[band:band + m * N].view(dtype).view(m, N)
        out = ops.linear_forward_swiglu(w, g, u, out=y)
        torch.cuda.synchronize()
        assert out.data_ptr() == y.data_ptr()
        assert bool(torch.isfinite(y.float()).all()), (kind, K, m, dtype)
        assert bool((ybuf[:band] == SENTINEL).all()) and bool((ybuf[band + m * N:] == SENTINEL).all()), "a store outside y"
        lead = (gbuf.numel() - m * K) // 2
        for buf in (gbuf, ubuf):
            assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + m * K:]).all())
        assert torch.equal(g, g0) and torch.equal(u, u0)
        assert torch.equal(y, ops.linear_forward_swiglu(w, g0, u0))


@pytest.mark.parametrize("kind,K,N,m", [("w4", 11008, 256, 1), ("w4", 4096, 8192, 4), ("g64", 11008, 256, 1), ("b3", 8192, 256, 1)])
def test_deterministic_and_capturable(kind, K, N, m):
    """Two calls give the same bits; one call captured on one stream (no parallel branches) and replayed equals the eager call."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    g = (torch.from_numpy(randx(m, K, seed=21)) * 2).to(DEV)
    u = torch.from_numpy(randx(m, K, seed=22)).to(DEV)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        eager = ops.linear_forward_swiglu(w, g, u).clone()
        again = ops.linear_forward_swiglu(w, g, u).clone()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    assert torch.equal(eager, again)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.linear_forward_swiglu(w, g, u)
    for _ in range(2):
        y.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)


def test_refusals_on_the_device():
    """What the entry does not serve raises QllmUnsupported and leaves y alone: five rows, 64-wide groups at two rows, the reference layout."""
    from qllm_amd import ops
    d, layer, w, keep = _layer("w4", 4096, 256)
    d64, layer64, w64, keep64 = _layer("g64", 4096, 256)
    for desc, m in ((w, 5), (w64, 2), (layer._descriptor(None, 0), 1)):
        g = torch.zeros((m, 4096), dtype=torch.float16, device=DEV)
        y = torch.full((m, 256), 3.0, dtype=torch.float16, device=DEV)
        assert ops.swiglu_describe(desc, m).startswith("refused: ")
        with pytest.raises(ops.QllmUnsupported):
            ops.linear_forward_swiglu(desc, g, g.clone(), out=y)
        assert bool((y == 3.0).all())


# ---- module level ---------------------------------------------------------------------------------------------------------------------
def _tiny_mlp(layout, g):
    import transformers
    from transformers.models.llama.modeling_llama import LlamaMLP
    from qllm_amd.modeling.q_layers import install_sibling_groups
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, vocab_size=32)
    mlp = LlamaMLP(cfg)
    for i, (name, K, N) in enumerate((("gate_proj", 256, 512), ("up_proj", 256, 512), ("down_proj", 512, 256))):
        setattr(mlp, name, to_layer(synth(layout, 4, g, K, N, "asym", False, False, seed=40 + i + g), DEV))
    assert install_sibling_groups(mlp, [type(mlp.down_proj)]) == 1   # gate / up: one grouped launch
    return mlp.to(DEV).eval()


@pytest.mark.parametrize("layout,g", [("GPTQ", 128), ("HQQ", 64)])
def test_llama_mlp_with_the_fused_forward(layout, g, monkeypatch):
    from qllm_amd import ops
    from qllm_amd.modeling.q_layers import install_fused_mlp, uninstall_fused_mlp
    mlp = _tiny_mlp(layout, g)
    q_type = type(mlp.down_proj)
    x1 = torch.from_numpy(randx(1, 256, seed=1)).to(DEV).view(1, 1, 256)
    x5 = torch.from_numpy(randx(5, 256, seed=2)).to(DEV).view(1, 5, 256)
    with torch.no_grad():
        before1, before5 = mlp(x1.clone()), mlp(x5.clone())
    calls = []
    real = ops.linear_forward_swiglu
    monkeypatch.setattr(ops, "linear_forward_swiglu", lambda *a, **k: (calls.append(a[1].shape[0]), real(*a, **k))[1])
    assert install_fused_mlp(mlp, [q_type]) == 1
    with torch.no_grad():
        after1 = mlp(x1.clone())
        assert calls == [1]                                       # exactly one fused call
        assert after1.shape == before1.shape
        a, b = after1.float().cpu().numpy().reshape(1, -1), before1.float().cpu().numpy().reshape(1, -1)
        assert O.rel_err(a, b) <= 1e-2 and O.rel_err(a.astype(np.float64), b.astype(np.float64)) <= 2e-3
        after5 = mlp(x5.clone())                                  # five rows: above the modules' cutoff, today's path
        assert torch.equal(after5, before5) and calls == [1]
        mlp.down_proj.swiglu_max_m = 8                            # ... and, sent to the entry: refused once, remembered, today's path
        assert torch.equal(mlp(x5.clone()), before5) and calls == [1, 5]
        assert torch.equal(mlp(x5.clone()), before5) and calls == [1, 5]
        assert torch.equal(mlp(x1.clone()), after1) and calls == [1, 5, 1]   # one row is still fused
    assert uninstall_fused_mlp(mlp) == 1
    with torch.no_grad():
        assert torch.equal(mlp(x1.clone()), before1) and calls == [1, 5, 1]


class _Tok:
    """The two things generate_smoke asks of a tokenizer."""
    eos_token_id = 2

    def __call__(self, prompt, return_tensors="pt"):
        import transformers
        ids = torch.tensor([[1] + [3 + (ord(c) % 100) for c in prompt[:6]]])
        return transformers.BatchEncoding({"input_ids": ids, "attention_mask": torch.ones_like(ids)})

    def decode(self, ids):
        return " ".join(str(int(i)) for i in ids)


def test_load_quantized_with_fuse_mlp(tmp_path, monkeypatch):
    """The loader's opt-in patches every MLP of the tiny checkpoint; logits stay within the loader test's bound of the default load and
    generate_smoke runs, with fused calls on its decode steps."""
    from test_loader_repack_cpu import _quantize_in_place, _tiny_llama
    from qllm_amd import ops
    from qllm_amd.modeling import base
    from qllm_amd.plugin.perplexity_utils import generate_smoke
    model, names = _quantize_in_place(_tiny_llama(), "GPTQ")
    d = str(tmp_path / "ckpt")
    base.save_quantized(model, d)
    plain = base.load_quantized(d, device=DEV)
    assert not hasattr(plain, "fused_mlps")                      # off by default
    fused = base.load_quantized(d, device=DEV, fuse_mlp=True)
    assert fused.fused_mlps == 2
    calls = []
    real = ops.linear_forward_swiglu
    monkeypatch.setattr(ops, "linear_forward_swiglu", lambda *a, **k: (calls.append(a[1].shape[0]), real(*a, **k))[1])
    ids = torch.randint(0, 128, (1, 1), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        a, b = fused(ids).logits.float().cpu().numpy()[0], plain(ids).logits.float().cpu().numpy()[0]
    assert calls == [1, 1]
    assert O.rel_err(a, b) <= 2e-2
    text = generate_smoke(fused, _Tok(), max_length=12)
    assert len(text.split()) == 12 and len(calls) > 2
