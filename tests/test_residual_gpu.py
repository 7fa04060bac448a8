"""-m gpu: the fused residual add (qllm_linear_forward_residual; csrc/strip1_resid.hip, csrc/strip1_swiglu_resid.hip: the RESID forms of the
batch-1 kernel) through the C ABI and the modules -- every form of the kernel's shape table, plain and SwiGLU input, in fp16 and bf16.

The arithmetic contract is bit identity with the eager add behind the unfused launch: y = round(residual + round(linear(x))).  The inputs
separate that from a kernel that adds before it rounds: the residual is random at the scale of the launch's own output, where -- asserted
here on the CPU from the oracle's fp64 result -- round(r + y) and round(r + round(y)) differ in more than a tenth of the elements."""
import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from gpu_util import Ref, guarded, randx, synth, to_layer
from test_swiglu_gpu import CASES, FORM_OF, SENTINEL, VARIANTS, _layer, _Tok, nw16_cases  # noqa: F401  (nw16_cases: the autouse fixture)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float16, torch.bfloat16)


def _inputs(K, N, dtype, seed):
    """x, gate (both signs) and up: unit normal data."""
    x = torch.from_numpy(randx(1, K, seed=seed)).to(dtype).to(DEV)
    g = (torch.from_numpy(randx(1, K, seed=seed + 1)) * 2).to(dtype).to(DEV)
    u = torch.from_numpy(randx(1, K, seed=seed + 2)).to(dtype).to(DEV)
    return x, g, u


def _residual(y, seed):
    std = float(y.float().std())
    r = torch.randn(y.shape, generator=torch.Generator().manual_seed(seed)) * std
    return r.to(y.dtype).to(y.device)


def _check_plan(w):
    from qllm_amd import ops
    plan = ops.plan_describe([w], 1)
    assert plan.startswith("strip1 "), plan
    assert ops.residual_describe(w, 1) == "residual " + plan and ops.residual_describe(w, 1, True) == "residual swiglu " + plan
    return plan


def _premise(ref, x, r, dtype):
    """Share of elements in which adding before rounding and rounding before adding differ, from the oracle's fp64 result."""
    xn = x.float().cpu().numpy().astype(np.float16)
    y64 = torch.from_numpy(ref.y64(xn))
    r64 = r.cpu().double()
    once = (r64 + y64).to(dtype)
    twice = (r64 + y64.to(dtype).double()).to(dtype)
    assert bool(torch.isfinite(once.float()).all())
    return float((once != twice).float().mean())


@pytest.mark.parametrize("kind,K,N", CASES)
def test_bit_identity_with_the_eager_add(kind, K, N):
    """linear_forward_residual(w, x, r) == r + linear_forward(w, x) and linear_forward_swiglu_residual(w, g, u, r) == r +
    linear_forward_swiglu(w, g, u), bit for bit, with r at the scale of the launch's output (random gates of both signs: both sides
    stage through the same code)."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    assert FORM_OF.get((kind, K, N), "") in _check_plan(w)
    ref = Ref(d) if N == 256 else None
    for dtype in DTYPES:
        x, g, u = _inputs(K, N, dtype, K + N)
        plain = ops.linear_forward(w, x)
        r = _residual(plain, seed=K)
        if ref is not None:   # (the premise, once per K and type: the wide launches share their K's arithmetic)
            share = _premise(ref, x, r, dtype)
            assert share >= 0.10, (kind, K, dtype, share)
        want = r + plain
        got = ops.linear_forward_residual(w, x, r)
        assert got.dtype == dtype and got.shape == (1, N) and bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, want), (kind, K, N, dtype, int((got != want).sum()))
        mlp = ops.linear_forward_swiglu(w, g, u)
        r2 = _residual(mlp, seed=K + 1)
        want = r2 + mlp
        got = ops.linear_forward_swiglu_residual(w, g, u, r2)
        assert got.dtype == dtype and bool(torch.isfinite(got.float()).all())
        assert torch.equal(got, want), (kind, K, N, dtype, int((got != want).sum()))


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
def test_zero_kinds_and_bias(variant):
    """Packed, fp16 and symmetric zero points, with and without bias, on the K = 11008 form (15 waves x 24, shifted last window), and with
    the AutoGPTQ offset on the packed case."""
    from qllm_amd import ops
    K, N = 11008, 256
    layout, zk, _ = VARIANTS[variant]
    for compat in ((0, 1) if (layout, zk) == ("GPTQ", "asym") else (0,)):
        d, layer, w, keep = _layer("w4", K, N, variant, compat)
        assert w.add_zero_bias == compat
        for dtype in DTYPES:
            x, g, u = _inputs(K, N, dtype, variant + 3 * compat)
            plain, mlp = ops.linear_forward(w, x), ops.linear_forward_swiglu(w, g, u)
            r = _residual(plain, seed=variant)
            assert torch.equal(ops.linear_forward_residual(w, x, r), r + plain), (variant, compat, dtype)
            assert torch.equal(ops.linear_forward_swiglu_residual(w, g, u, r), r + mlp), (variant, compat, dtype)


@pytest.mark.parametrize("kind,K,N", [("w4", 4096, 256), ("w4", 11008, 256), ("g64", 5120, 256), ("b3", 8192, 256), ("w4", 4096, 8192)])
def test_in_place(kind, K, N):
    """The residual row passed as y too: the result of the out-of-place call, and `residual` is the tensor returned."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    for dtype in DTYPES:
        x, g, u = _inputs(K, N, dtype, 5)
        r = _residual(ops.linear_forward(w, x), seed=6)
        for fused, args in ((ops.linear_forward_residual, (x,)), (ops.linear_forward_swiglu_residual, (g, u))):
            want = fused(w, *args, r)
            rr = r.clone()
            out = fused(w, *args, rr, out=rr)
            assert out.data_ptr() == rr.data_ptr() and torch.equal(rr, want), (kind, K, dtype, fused.__name__)


# one case per form family, the forms that load the residual late (SWIGLU with rounds of 24 at 64 registers, of 56 and 64) and K = 32768
GUARD_CASES = [("w4", 256, 256), ("w4", 11008, 256), ("w4", 12288, 256), ("w4", 4096, 8192), ("g64", 5120, 256), ("b3", 11008, 256),
               ("b3g64", 3584, 8192), ("w4", 28672, 256), ("w4", 32768, 256)]


@pytest.mark.parametrize("kind,K,N", GUARD_CASES)
def test_reads_and_writes_stay_inside_their_tensors(kind, K, N):
    """x / gate / up / residual carved out of NaN-banded buffers, y between sentinel bands: a read outside an input puts a NaN into the
    result, a store outside [1, N] changes a band."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    for dtype in DTYPES:
        x0, g0, u0 = _inputs(K, N, dtype, 9)
        r0 = _residual(ops.linear_forward(w, x0), seed=10)
        (xbuf, x), (gbuf, g), (ubuf, u), (rbuf, r) = guarded(x0), guarded(g0), guarded(u0), guarded(r0)
        for fused, args, args0 in ((ops.linear_forward_residual, (x,), (x0,)), (ops.linear_forward_swiglu_residual, (g, u), (g0, u0))):
            band = 2048
            ybuf = torch.full((band + N + band,), SENTINEL, dtype=torch.int16, device=DEV)
            y = ybuf[band:band + N].view(dtype).view(1, N)
            out = fused(w, *args, r, out=y)
            torch.cuda.synchronize()
            assert out.data_ptr() == y.data_ptr()
            assert bool(torch.isfinite(y.float()).all()), (kind, K, dtype)
            assert bool((ybuf[:band] == SENTINEL).all()) and bool((ybuf[band + N:] == SENTINEL).all()), "a store outside y"
            assert torch.equal(y, fused(w, *args0, r0))
        for buf, view, orig in ((xbuf, x, x0), (gbuf, g, g0), (ubuf, u, u0), (rbuf, r, r0)):
            lead = (buf.numel() - orig.numel()) // 2
            assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + orig.numel():]).all())
            assert torch.equal(view, orig)


@pytest.mark.parametrize("kind,K,N", [("w4", 11008, 256), ("w4", 4096, 8192), ("g64", 11008, 256), ("b3", 8192, 256)])
def test_deterministic_and_capturable(kind, K, N):
    """Two calls give the same bits; one call captured on one stream (no parallel branches) and replayed twice equals the eager call."""
    from qllm_amd import ops
    d, layer, w, keep = _layer(kind, K, N)
    x, g, u = _inputs(K, N, torch.float16, 21)
    r = _residual(ops.linear_forward(w, x), seed=22)
    for fused, args in ((ops.linear_forward_residual, (x,)), (ops.linear_forward_swiglu_residual, (g, u))):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            eager = fused(w, *args, r).clone()
            again = fused(w, *args, r).clone()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert torch.equal(eager, again)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = fused(w, *args, r)
        for _ in range(2):
            y.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(y, eager)


def test_refusals_on_the_device():
    """What the entry does not serve raises QllmUnsupported and leaves y alone: two rows, the reference layout, the batch-1 kernel
    switched off; a residual of another shape never reaches the library."""
    from qllm_amd import ops
    d, layer, w, keep = _layer("w4", 4096, 256)

    def refused(desc, m):
        x = torch.zeros((m, 4096), dtype=torch.float16, device=DEV)
        r = torch.ones((m, 256), dtype=torch.float16, device=DEV)
        for sw, call in ((False, lambda y: ops.linear_forward_residual(desc, x, r, out=y)),
                         (True, lambda y: ops.linear_forward_swiglu_residual(desc, x, x.clone(), r, out=y))):
            y = torch.full((m, 256), 3.0, dtype=torch.float16, device=DEV)
            assert ops.residual_describe(desc, m, sw).startswith("refused: ")
            with pytest.raises(ops.QllmUnsupported):
                call(y)
            torch.cuda.synchronize()
            assert bool((y == 3.0).all()) and bool((r == 1.0).all())

    refused(w, 2)
    refused(layer._descriptor(None, 0), 1)
    try:
        ops.set_knob("QLLM_STRIP1", 0)
        refused(w, 1)
    finally:
        ops.reset_knobs()
    x = torch.zeros((1, 4096), dtype=torch.float16, device=DEV)
    for bad in (torch.zeros((1, 128), dtype=torch.float16, device=DEV), torch.zeros((1, 256), dtype=torch.bfloat16, device=DEV),
                torch.zeros((256, 2), dtype=torch.float16, device=DEV).t()[:1]):
        with pytest.raises(RuntimeError, match="residual"):
            ops.linear_forward_residual(w, x, bad)


# ---- module level ---------------------------------------------------------------------------------------------------------------------
def _tiny_layer(layout, g):
    """One LlamaDecoderLayer (hidden 256, intermediate 512) whose seven linears are q_layers, and its rotary embedding."""
    import transformers
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer, LlamaRotaryEmbedding
    from qllm_amd.modeling.q_layers import install_sibling_groups
    cfg = transformers.LlamaConfig(hidden_size=256, intermediate_size=512, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4,
                                   vocab_size=32, max_position_embeddings=64)
    cfg._attn_implementation = "eager"
    torch.manual_seed(0)
    layer = LlamaDecoderLayer(cfg, 0).half()
    for i, (parent, name, K, N) in enumerate((("self_attn", "q_proj", 256, 256), ("self_attn", "k_proj", 256, 256), ("self_attn", "v_proj", 256, 256),
                                              ("self_attn", "o_proj", 256, 256), ("mlp", "gate_proj", 256, 512), ("mlp", "up_proj", 256, 512),
                                              ("mlp", "down_proj", 512, 256))):
        setattr(getattr(layer, parent), name, to_layer(synth(layout, 4, g, K, N, "asym", False, False, seed=60 + i + g), DEV))
    with torch.no_grad():
        layer.input_layernorm.weight.copy_(torch.rand(256) + 0.5)
        layer.post_attention_layernorm.weight.copy_(torch.rand(256) + 0.5)
    assert install_sibling_groups(layer, [type(layer.mlp.down_proj)]) == 2   # q/k/v and gate/up
    return layer.to(DEV).eval(), LlamaRotaryEmbedding(cfg).to(DEV)


def _step(layer, rot, x):
    pos = torch.arange(x.shape[1], device=DEV).unsqueeze(0)
    with torch.no_grad():
        return layer(x.clone(), attention_mask=None, position_ids=pos, position_embeddings=rot(x, pos))


def _count(monkeypatch):
    from qllm_amd import ops
    calls = {"plain": 0, "swiglu": 0}
    real_p, real_s = ops.linear_forward_residual, ops.linear_forward_swiglu_residual

    def plain(*a, **k):
        calls["plain"] += 1
        assert k.get("out") is None and len(a) == 3                  # module calls never write in place
        return real_p(*a, **k)

    def swiglu(*a, **k):
        calls["swiglu"] += 1
        assert k.get("out") is None and len(a) == 4
        return real_s(*a, **k)

    monkeypatch.setattr(ops, "linear_forward_residual", plain)
    monkeypatch.setattr(ops, "linear_forward_swiglu_residual", swiglu)
    return calls


@pytest.mark.parametrize("layout,g", [("GPTQ", 128), ("HQQ", 64)])
def test_llama_decoder_layer_with_the_fused_residuals(layout, g, monkeypatch):
    from qllm_amd.modeling.q_layers import (install_fused_mlp, install_fused_norm, install_fused_residual, uninstall_fused_mlp,
                                            uninstall_fused_norm, uninstall_fused_residual)
    layer, rot = _tiny_layer(layout, g)
    q = [type(layer.mlp.down_proj)]
    x1 = (torch.from_numpy(randx(1, 256, seed=1)) * 0.5).to(DEV).view(1, 1, 256)
    x5 = (torch.from_numpy(randx(5, 256, seed=2)) * 0.5).to(DEV).view(1, 5, 256)
    before1, before5 = _step(layer, rot, x1), _step(layer, rot, x5)
    assert before1.shape == x1.shape and bool(torch.isfinite(before1.float()).all())
    calls = _count(monkeypatch)
    # only the residuals: two plain-residual calls, bit for bit the class's forward
    assert install_fused_residual(layer, q) == 1
    assert torch.equal(_step(layer, rot, x1), before1) and calls == {"plain": 2, "swiglu": 0}
    assert torch.equal(_step(layer, rot, x5), before5) and calls == {"plain": 2, "swiglu": 0}     # five rows: no fused call
    # all three installs, in the loader's order
    assert uninstall_fused_residual(layer) == 1
    assert install_fused_mlp(layer, q) == 1 and install_fused_norm(layer, q) == 2 and install_fused_residual(layer, q) == 1
    calls.update(plain=0, swiglu=0)
    after1 = _step(layer, rot, x1)
    assert calls == {"plain": 1, "swiglu": 1}
    a, b = after1.float().cpu().numpy().reshape(1, -1), before1.float().cpu().numpy().reshape(1, -1)
    assert O.rel_err(a, b) <= 2e-2                                    # (the fused norm and silu round like the eager ones up to rare last bits)
    after5 = _step(layer, rot, x5)
    assert calls == {"plain": 1, "swiglu": 1}                          # five rows: no fused call
    assert O.rel_err(after5.float().cpu().numpy().reshape(1, -1), before5.float().cpu().numpy().reshape(1, -1)) <= 2e-2
    # without the other two, five rows are the uninstalled output bit for bit
    assert uninstall_fused_norm(layer) == 2 and uninstall_fused_mlp(layer) == 1
    assert torch.equal(_step(layer, rot, x5), before5) and calls == {"plain": 1, "swiglu": 1}
    assert torch.equal(_step(layer, rot, x1), before1) and calls == {"plain": 3, "swiglu": 1}
    assert uninstall_fused_residual(layer) == 1
    assert torch.equal(_step(layer, rot, x1), before1) and torch.equal(_step(layer, rot, x5), before5) and calls == {"plain": 3, "swiglu": 1}
    assert not any("forward" in m.__dict__ for m in layer.modules())


def test_load_quantized_with_fuse_residual(tmp_path, monkeypatch):
    """The loader's opt-in patches both decoder layers of the tiny checkpoint; the logits at one token are the default load's bit for bit
    and generate_smoke runs, with fused calls on its decode steps."""
    from test_loader_repack_cpu import _quantize_in_place, _tiny_llama
    from qllm_amd.modeling import base
    from qllm_amd.plugin.perplexity_utils import generate_smoke
    model, names = _quantize_in_place(_tiny_llama(), "GPTQ")
    d = str(tmp_path / "ckpt")
    base.save_quantized(model, d)
    plain = base.load_quantized(d, device=DEV)
    assert not hasattr(plain, "fused_residuals")                     # off by default
    fused = base.load_quantized(d, device=DEV, fuse_residual=True)
    assert fused.fused_residuals == 2
    calls = _count(monkeypatch)
    ids = torch.randint(0, 128, (1, 1), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        a, b = fused(ids).logits, plain(ids).logits
    assert calls == {"plain": 4, "swiglu": 0}
    assert torch.equal(a, b)
    text = generate_smoke(fused, _Tok(), max_length=12)
    assert len(text.split()) == 12 and calls["plain"] > 4
