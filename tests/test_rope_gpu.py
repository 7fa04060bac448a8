"""-m gpu: the rotary embedding of q and k as one kernel (qllm_rope, csrc/rope.hip) through ops.rope and the modules.

The oracle is the eager expression itself -- transformers' apply_rotary_pos_emb, restated in tests/test_rope_cpu.py and held to
transformers' own function there -- evaluated by torch on the CPU; the comparison is torch.equal, no tolerance; every oracle result is
asserted free of NaN on the CPU side.

Shapes: rows 1, 2, 3 and 17 as B x S = 1x1, 2x1, 1x3, 1x17 (17 rows of 40 heads x 16 chunks: more than one block, a ragged last one), batch
2 also with one [1, S, D] table; heads (1, 1), (4, 4), (8, 2), (32, 8); head_dim 16 (one thread per head), 64, 80 (five threads per head:
no power of two), 128, 256 (the largest); both head layouts; q and k contiguous and as slices of one [rows, (Hq + 2 Hk) D] buffer; q
alone; 2048 x (32, 8) x 128 once per type: 2560 blocks' worth of threads on a grid capped at eight blocks per compute unit, the
grid-stride path."""
import pytest
import torch

from gpu_util import guarded
from test_rope_cpu import FAMILIES, eager_rope, module_dicts, prefill_and_decode, tiny_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = (torch.float16, torch.bfloat16)
BS = ((1, 1, 1), (2, 1, 2), (2, 1, 1), (1, 3, 1), (1, 17, 1))          # (B, S, the table's batch)
HEADS = ((1, 1), (4, 4), (8, 2), (32, 8))
DIMS = (16, 64, 80, 128, 256)
VALUES = ("randx", "zeros", "subnormal", "overflow")


def _values(kind, shape, dtype, g):
    """A tensor of `shape` for q / k, and whether cos / sin are +-1 and 0 instead of real angles."""
    if kind == "randx":
        return torch.randn(shape, generator=g).to(dtype)
    sign = torch.randint(0, 2, shape, generator=g) * 2.0 - 1.0
    if kind == "zeros":                                      # +0 and -0, and a few ordinary values among them
        x = torch.where(torch.rand(shape, generator=g) < 0.8, torch.zeros(shape), torch.randn(shape, generator=g))
        return (x.to(dtype).float() + 0.0).to(dtype) * sign.to(dtype)
    if kind == "subnormal":                                  # bit patterns below the smallest normal, both signs
        top = 1 << (10 if dtype == torch.float16 else 7)
        bits = torch.randint(1, top, shape, generator=g).to(torch.int16)
        return bits.view(dtype) * sign.to(dtype)
    assert kind == "overflow"                                # +-max (65504 in fp16): with |cos| = |sin| = 1 the sum is +-inf or 0
    return torch.full(shape, torch.finfo(dtype).max).to(dtype) * sign.to(dtype)


def _case(b, s, cb, hq, hk, d, dtype, kind="randx", ud=1, sliced=False, seed=0, with_k=True):
    """CPU tensors q, k, cos, sin of one case, q / k in the layout the attention forward hands over (ud 1: [B, H, S, D] views of
    [B, S, H, D] memory; ud 2: [B, S, H, D]), contiguous or as slices of one wide buffer whose third part (v) is NaN."""
    g = torch.Generator().manual_seed(seed + 1000 * d + 10 * hq + s)
    q, k = _values(kind, (b, s, hq, d), dtype, g), _values(kind, (b, s, hk, d), dtype, g)
    if sliced:
        buf = torch.full((b, s, (hq + 2 * hk) * d), float("nan"), dtype=dtype)
        buf[..., :hq * d] = q.view(b, s, -1)
        buf[..., hq * d:(hq + hk) * d] = k.view(b, s, -1)
        q, k = buf[..., :hq * d].view(b, s, hq, d), buf[..., hq * d:(hq + hk) * d].view(b, s, hk, d)
    if ud == 1:
        q, k = q.transpose(1, 2), k.transpose(1, 2)
    if kind == "overflow":                                   # |cos| = |sin| = 1
        cos = (torch.randint(0, 2, (cb, s, d), generator=g) * 2.0 - 1.0).to(dtype)
        sin = (torch.randint(0, 2, (cb, s, d), generator=g) * 2.0 - 1.0).to(dtype)
    else:
        ang = torch.rand(cb, s, d // 2, generator=g) * 6.2832
        ang = torch.cat((ang, ang), -1)
        cos, sin = ang.cos().to(dtype), ang.sin().to(dtype)
        if kind == "zeros":                                  # signed zeros in the tables too
            z = torch.rand(cb, s, d, generator=g) < 0.3
            cos, sin = torch.where(z, -torch.zeros((), dtype=dtype), cos), torch.where(z.roll(1, -1), torch.zeros((), dtype=dtype), sin)
    return q, (k if with_k else None), cos, sin


def _to_dev(t):
    """The tensor on the device with the CPU tensor's strides and (for a view into a wider buffer) its surroundings."""
    if t is None:
        return None
    whole = torch.empty(t.untyped_storage().nbytes() // t.element_size(), dtype=t.dtype)
    whole.set_(t.untyped_storage())
    return whole.to(DEV).as_strided(t.shape, t.stride(), t.storage_offset())


def _same(got, want):
    """Bit for bit (NaN-free by the oracle's assertion, so torch.equal is a bit comparison up to the sign of zero, which is checked too),
    and the strides of every dimension longer than one."""
    assert not bool(torch.isnan(want.float()).any())
    got = got.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    assert torch.equal(got, want), int((got != want).sum())
    assert torch.equal(torch.signbit(got), torch.signbit(want)), "the sign of a zero"
    assert [st for n, st in zip(got.shape, got.stride()) if n > 1] == [st for n, st in zip(want.shape, want.stride()) if n > 1]


def _check(case, ud):
    from qllm_amd import ops
    q, k, cos, sin = case
    want = eager_rope(q, k, cos, sin, ud)
    got = ops.rope(_to_dev(q), _to_dev(k), _to_dev(cos), _to_dev(sin), ud)
    _same(got[0], want[0])
    if k is None:
        assert got[1] is None
    else:
        _same(got[1], want[1])


# ---- bit identity with eager ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_bit_identity_with_the_eager_expression(dtype, d):
    for b, s, cb in BS:
        for hq, hk in HEADS:
            for ud in (1, 2):
                for sliced in (False, True):
                    _check(_case(b, s, cb, hq, hk, d, dtype, ud=ud, sliced=sliced), ud)
            _check(_case(b, s, cb, hq, hk, d, dtype, with_k=False, seed=5), 1)      # q alone


@pytest.mark.parametrize("kind", VALUES[1:])
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_signed_zeros_subnormals_and_overflow_come_out_as_eager_does(dtype, kind):
    seen_inf = seen_negzero = False
    for d in DIMS:
        for b, s, cb in ((1, 3, 1), (1, 17, 1), (2, 1, 1)):
            for ud, sliced in ((1, False), (2, True)):
                case = _case(b, s, cb, 8, 2, d, dtype, kind=kind, ud=ud, sliced=sliced, seed=7)
                want = eager_rope(*case, ud)[0]
                seen_inf |= bool(torch.isinf(want).any())
                seen_negzero |= bool(((want == 0) & torch.signbit(want)).any())
                _check(case, ud)
    assert seen_inf == (kind == "overflow")                                            # the premise: the sum overflows to inf in eager too
    assert seen_negzero or kind != "zeros"


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_2048_rows_take_the_grid_stride_path(dtype):
    from qllm_amd import _lib
    cus = _lib.device_info(0)["compute_units"]
    assert 2048 * 40 * 8 > cus * 8 * 256                                               # more threads' worth of work than the capped grid has
    _check(_case(1, 2048, 1, 32, 8, 128, dtype, seed=11), 1)


# ---- memory, determinism, capture ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_in_place(dtype):
    from qllm_amd import ops
    for b, s, hq, hk, d in ((1, 1, 32, 8, 128), (2, 3, 4, 4, 80), (1, 17, 8, 2, 16)):
        q, k, cos, sin = _case(b, s, b, hq, hk, d, dtype, ud=2, seed=13)
        want = eager_rope(q, k, cos, sin, 2)
        qd, kd = q.to(DEV), k.to(DEV)
        out = ops.rope(qd, kd, cos.to(DEV), sin.to(DEV), 2, out=(qd, kd))
        assert out[0] is qd and out[1] is kd
        _same(qd, want[0])
        _same(kd, want[1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["f16", "bf16"])
def test_reads_and_writes_stay_inside_their_tensors(dtype):
    """NaN bands around all six tensors: a read outside an input puts a NaN into a result, a store outside an output changes a band.
    Contiguous inputs; with slices of one buffer the neighbours are NaN already (`_case`)."""
    from qllm_amd import ops
    for b, s, hq, hk, d in ((1, 1, 1, 1, 16), (1, 1, 32, 8, 128), (1, 17, 8, 2, 80), (2, 3, 4, 4, 256)):
        q, k, cos, sin = _case(b, s, b, hq, hk, d, dtype, ud=2, seed=17)
        want = eager_rope(q, k, cos, sin, 2)
        bufs = [guarded(t.to(DEV)) for t in (q, k, cos, sin)]
        outs = [guarded(torch.zeros_like(t).to(DEV)) for t in (q, k)]
        got = ops.rope(*(v for _, v in bufs), 2, out=(outs[0][1], outs[1][1]))
        torch.cuda.synchronize()
        _same(got[0], want[0])
        _same(got[1], want[1])
        for (buf, view), orig in zip(bufs + outs, (q, k, cos, sin, want[0], want[1])):
            lead = (buf.numel() - view.numel()) // 2
            assert bool(torch.isnan(buf[:lead]).all()) and bool(torch.isnan(buf[lead + view.numel():]).all())
            assert torch.equal(view.cpu(), orig)                                       # (the inputs are what they were)


def test_deterministic_and_capturable():
    """Two runs give the same bits, and a captured launch replayed twice gives them again."""
    from qllm_amd import ops
    for dtype, ud, sliced in ((torch.float16, 1, True), (torch.bfloat16, 2, False)):
        q, k, cos, sin = (_to_dev(t) for t in _case(1, 17, 1, 32, 8, 128, dtype, ud=ud, sliced=sliced, seed=19))
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            first = [o.clone() for o in ops.rope(q, k, cos, sin, ud)]
            again = [o.clone() for o in ops.rope(q, k, cos, sin, ud)]
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, again))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            outs = ops.rope(q, k, cos, sin, ud)
        for _ in range(2):
            for o in outs:
                o.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip(outs, first))


def test_refusals_on_the_device():
    """head_dim 24 and 272, a misaligned view and mixed types raise QllmUnsupported and launch nothing: the outputs keep their fill."""
    from qllm_amd import ops

    def refused(q, k, cos, sin):
        outs = (torch.full(q.shape, 3.0, dtype=q.dtype, device=DEV), torch.full(k.shape, 3.0, dtype=k.dtype, device=DEV))
        with pytest.raises(ops.QllmUnsupported):
            ops.rope(q, k, cos, sin, 2, out=outs)
        with pytest.raises(ops.QllmUnsupported):
            ops.rope(q, k, cos, sin, 2)
        torch.cuda.synchronize()
        assert all(bool((o == 3.0).all()) for o in outs)

    for d in (24, 272):
        refused(*(t.to(DEV) for t in _case(1, 3, 1, 4, 2, d, torch.float16, ud=2)))
    q, k, cos, sin = (t.to(DEV) for t in _case(1, 3, 1, 4, 2, 64, torch.float16, ud=2))
    wide = torch.zeros(q.numel() + 8, dtype=q.dtype, device=DEV)
    off = wide[4:-4].view(q.shape)
    assert off.data_ptr() % 16 == 8
    refused(off, k, cos, sin)
    refused(q, k, cos.float(), sin.float())
    refused(q, k.bfloat16(), cos, sin)
    want = eager_rope(*(t.cpu() for t in (q, k, cos, sin)), 2)                         # ... and the same tensors, aligned and of one type, are served
    _same(ops.rope(q, k, cos, sin, 2)[0], want[0])


# ---- module level ---------------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch):
    from qllm_amd import ops
    calls = {"rope": 0}
    real = ops.rope

    def rope(*a, **kw):
        calls["rope"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "rope", rope)
    return calls


@pytest.mark.parametrize("attn", ["eager", "sdpa"])
@pytest.mark.parametrize("heads,kv_heads", [(4, 4), (4, 2)])
@pytest.mark.parametrize("family", FAMILIES)
def test_tiny_models_compute_the_same_logits_with_the_kernel(family, heads, kv_heads, attn, monkeypatch):
    """tests/test_rope_cpu.py's tiny-model test in fp16 on the device with the real op: a 5-token prefill and 4 decode steps, bit for bit
    the unpatched model's logits, one kernel per layer and forward."""
    from qllm_amd.modeling.q_layers import install_fused_rope, uninstall_fused_rope
    model = tiny_model(family, heads, kv_heads, attn, device=DEV)
    before = module_dicts(model)
    want = prefill_and_decode(model, DEV)
    assert all(bool(torch.isfinite(w.float()).all()) for w in want)
    calls = _count(monkeypatch)
    assert install_fused_rope(model) == 2
    got = prefill_and_decode(model, DEV)
    assert calls["rope"] == 2 * 5
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    assert uninstall_fused_rope(model) == 2 and module_dicts(model) == before
    assert all(torch.equal(g, w) for g, w in zip(prefill_and_decode(model, DEV), want)) and calls["rope"] == 2 * 5


@pytest.mark.parametrize("order", ["rope_last", "rope_first"])
def test_llama_decoder_layer_with_all_four_fusions(order, monkeypatch):
    """The quantized decoder layer of tests/test_residual_gpu.py with fuse_mlp, fuse_norm, fuse_residual and fuse_rope installed in two
    orders: bit for bit the layer with the other three only, at one row and at five."""
    from gpu_util import randx
    from test_residual_gpu import _step, _tiny_layer
    from qllm_amd.modeling.q_layers import (install_fused_mlp, install_fused_norm, install_fused_residual, install_fused_rope, uninstall_fused_mlp,
                                            uninstall_fused_norm, uninstall_fused_residual, uninstall_fused_rope)
    layer, rot = _tiny_layer("GPTQ", 128)
    q = [type(layer.mlp.down_proj)]
    xs = [(torch.from_numpy(randx(m, 256, seed=m)) * 0.5).to(DEV).view(1, m, 256) for m in (1, 5)]
    others = lambda: install_fused_mlp(layer, q) == 1 and install_fused_norm(layer, q) == 2 and install_fused_residual(layer, q) == 1  # noqa: E731
    assert others()
    want = [_step(layer, rot, x) for x in xs]
    assert all(bool(torch.isfinite(w.float()).all()) for w in want)
    calls = _count(monkeypatch)
    if order == "rope_last":
        assert install_fused_rope(layer) == 1
    else:
        assert uninstall_fused_residual(layer) == 1 and uninstall_fused_norm(layer) == 2 and uninstall_fused_mlp(layer) == 1
        assert install_fused_rope(layer) == 1 and install_fused_residual(layer, q) == 1 and install_fused_norm(layer, q) == 2 and install_fused_mlp(layer, q) == 1
    for x, w in zip(xs, want):
        assert torch.equal(_step(layer, rot, x), w)
    assert calls["rope"] == 2
    assert uninstall_fused_rope(layer) == 1
    for x, w in zip(xs, want):
        assert torch.equal(_step(layer, rot, x), w)
    assert calls["rope"] == 2
    assert uninstall_fused_residual(layer) == 1 and uninstall_fused_norm(layer) == 2 and uninstall_fused_mlp(layer) == 1
    assert not any("forward" in m.__dict__ for m in layer.modules())


def test_load_quantized_with_fuse_rope_generates_the_same_tokens(tmp_path, monkeypatch):
    """load_quantized(fuse_rope=True) against the default load of a saved tiny checkpoint: 8 greedy steps through a KV cache, the same
    logits bit for bit and so the same tokens; one kernel per layer and step."""
    from test_loader_repack_cpu import _quantize_in_place, _tiny_llama
    from qllm_amd.modeling import base
    model, _ = _quantize_in_place(_tiny_llama(), "GPTQ")
    d = str(tmp_path / "ckpt")
    base.save_quantized(model, d)
    plain = base.load_quantized(d, device=DEV)
    assert not hasattr(plain, "fused_ropes")                                           # off by default
    fused = base.load_quantized(d, device=DEV, fuse_rope=True)
    assert fused.fused_ropes == 2
    calls = _count(monkeypatch)
    tok_p = tok_f = torch.tensor([[5, 9, 2]], device=DEV)
    pkv_p = pkv_f = None
    with torch.no_grad():
        for step in range(8):
            op = plain(tok_p, past_key_values=pkv_p, use_cache=True)
            of = fused(tok_f, past_key_values=pkv_f, use_cache=True)
            pkv_p, pkv_f = op.past_key_values, of.past_key_values
            assert torch.equal(op.logits, of.logits), step
            tok_p, tok_f = op.logits[:, -1:].argmax(-1), of.logits[:, -1:].argmax(-1)
            assert torch.equal(tok_p, tok_f)
    assert calls["rope"] == 2 * 8
