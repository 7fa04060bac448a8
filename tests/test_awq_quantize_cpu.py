"""The AWQ quantizer's entry points (qllm_awq_clip_search, qllm_awq_clip_search_workspace_bytes, qllm_awq_quantize) on a GPU-less host:
symbols, argument validation (it runs before any device work), and the torch plumbing of qllm_amd/quantization/awq.py that needs no
device: folding the scales into the previous op, the token sample, the refusal of CPU weights."""
import ctypes
import os

import pytest

from qllm_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16, F32 = 0, 1, 3
SHRINK = ctypes.c_float(0.5)


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def _clip(lib, w=16, dtype=F16, gram=16, N=64, K=256, bits=4, g=128, n_grid=20, shrink=0.5, bm=16, bi=16, err=16, ws=None, ws_bytes=0):
    """Fake aligned pointers: every call below is refused before anything is dereferenced or launched."""
    return lib.qllm_awq_clip_search(w, dtype, gram, N, K, bits, g, n_grid, ctypes.c_float(shrink), bm, bi, err, ws, ws_bytes, None)


def _quant(lib, w=16, dtype=F16, s=16, clip=16, N=64, K=256, bits=4, g=128, codes=16, sc=16, z=16, wq=16):
    return lib.qllm_awq_quantize(w, dtype, s, clip, N, K, bits, g, codes, sc, z, wq, None)


def test_symbols_exist_and_the_abi_version_is_unchanged(lib):
    text = open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read()
    assert "#define QLLM_ABI_VERSION 7" in text and lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    for name in ("qllm_awq_clip_search", "qllm_awq_clip_search_workspace_bytes", "qllm_awq_quantize"):
        assert name in _lib.EXPORTS and name in text
        assert ctypes.cast(getattr(lib, name), ctypes.c_void_p).value


def test_workspace_bytes_is_pure(lib):
    f = lib.qllm_awq_clip_search_workspace_bytes
    shapes = [(64, 256, 128), (1000, 512, 64), (4096, 11008, 128), (0, 0, 0), (-1, 256, 32)]
    first = [f(*s) for s in shapes]
    assert [f(*s) for s in shapes] == first == [f(*s) for s in reversed(shapes)][::-1]
    assert all(v % 16 == 0 for v in first)          # the search keeps its state in registers and LDS: currently 0 everywhere
    assert first == [0] * len(shapes)


def test_validation_runs_before_any_device_work(lib):
    for null in ("w", "gram", "bm", "bi", "err"):
        assert _clip(lib, **{null: None}) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error(), null
    assert _quant(lib, w=None) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error()
    assert _quant(lib, codes=None, sc=None, z=None, wq=None) == _lib.QLLM_ERR_INVALID and "every output is NULL" in _lib.last_error()
    for call in (_clip, _quant):
        assert call(lib, dtype=2) == _lib.QLLM_ERR_INVALID and "w_dtype" in _lib.last_error()
        assert call(lib, N=0) == _lib.QLLM_ERR_INVALID and call(lib, K=-4) == _lib.QLLM_ERR_INVALID
        # widths other than 2..8, groups other than 32 / 64 / 128
        for kw in (dict(bits=9), dict(bits=1), dict(g=48, K=240), dict(g=16), dict(g=256, K=512)):
            assert call(lib, **kw) == _lib.QLLM_ERR_UNSUPPORTED, kw
            assert "bits 2..8" in _lib.last_error() and "32 / 64 / 128" in _lib.last_error()
        # an allowed group that does not divide K
        assert call(lib, K=224, g=64) == _lib.QLLM_ERR_INVALID and "multiple of group_size" in _lib.last_error()
        assert call(lib, K=320, g=128) == _lib.QLLM_ERR_INVALID
        assert call(lib, w=18, dtype=F32) == _lib.QLLM_ERR_INVALID and "aligned" in _lib.last_error()
    with pytest.raises(_lib.QllmUnsupported):
        _lib.check(_clip(lib, bits=9))
    # the Gram tiles are read four floats at a time; the search serves 1..10 candidates
    assert _clip(lib, gram=24) == _lib.QLLM_ERR_INVALID and "16-byte aligned" in _lib.last_error()
    assert _clip(lib, bm=18) == _lib.QLLM_ERR_INVALID
    for kw in (dict(n_grid=0), dict(shrink=0.0), dict(shrink=1.5), dict(n_grid=40), dict(n_grid=1, shrink=0.5)):
        assert _clip(lib, **kw) == _lib.QLLM_ERR_UNSUPPORTED and "candidates" in _lib.last_error(), kw
    # an unaligned workspace is refused even though none is needed
    assert _clip(lib, ws=24, ws_bytes=64) == _lib.QLLM_ERR_WORKSPACE and "16-byte aligned" in _lib.last_error()
    assert _quant(lib, s=18) == _lib.QLLM_ERR_INVALID and _quant(lib, clip=18) == _lib.QLLM_ERR_INVALID
    assert _quant(lib, wq=18, dtype=F32) == _lib.QLLM_ERR_INVALID and _quant(lib, codes=18) == _lib.QLLM_ERR_INVALID


def _block_and_input():
    """Block 0 of a small fp32 Llama with what the model hands it."""
    import torch
    import transformers
    from qllm_amd.quantization._common import Catcher, Stop
    cfg = transformers.LlamaConfig(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=4, num_key_value_heads=4,
                                   vocab_size=64, max_position_embeddings=32, tie_word_embeddings=False)
    torch.manual_seed(0)
    model = transformers.LlamaForCausalLM(cfg).float().eval()
    block, catcher = model.model.layers[0], Catcher()
    model.model.layers[0] = catcher
    try:
        model(torch.randint(0, 64, (2, 12), generator=torch.Generator().manual_seed(1)), use_cache=False)
    except Stop:
        pass
    return block, catcher.inputs[0], catcher.args, catcher.kwargs


@pytest.mark.parametrize("group", ["norm->qkv", "v->o", "norm->gate/up", "up->down"])
def test_fold_scales_leaves_the_block_output_unchanged(group):
    import torch
    from qllm_amd.quantization import fold_scales
    block, x, args, kwargs = _block_and_input()
    att, mlp = block.self_attn, block.mlp
    prev_op, layers = {"norm->qkv": (block.input_layernorm, [att.q_proj, att.k_proj, att.v_proj]), "v->o": (att.v_proj, [att.o_proj]),
                       "norm->gate/up": (block.post_attention_layernorm, [mlp.gate_proj, mlp.up_proj]),
                       "up->down": (mlp.up_proj, [mlp.down_proj])}[group]
    s = torch.exp(0.7 * torch.randn(layers[0].in_features, generator=torch.Generator().manual_seed(2)))
    with torch.no_grad():
        before = block(x, *args, **kwargs)
        before = before[0] if isinstance(before, tuple) else before
        w0 = [l.weight.data.clone() for l in layers]
        fold_scales(block, prev_op, layers, s)
        after = block(x, *args, **kwargs)
        after = after[0] if isinstance(after, tuple) else after
    assert all(torch.allclose(l.weight.data, w * s.view(1, -1), rtol=1e-6) for l, w in zip(layers, w0))
    assert float((after - before).norm() / before.norm()) <= 1e-5


def test_fold_scales_raises_on_an_unsupported_previous_op():
    import torch
    from qllm_amd.quantization import fold_scales
    fc = torch.nn.Linear(8, 8)
    with pytest.raises(NotImplementedError, match="not supported"):
        fold_scales(None, torch.nn.GELU(), [fc], torch.ones(8))
    with pytest.raises(NotImplementedError, match="not supported"):
        fold_scales(None, torch.nn.Embedding(4, 8), [fc], torch.ones(8))


@pytest.mark.parametrize("tokens", [100, 512, 1000])
def test_token_sampling_rule(tokens):
    import torch
    from qllm_amd.quantization.awq import gram_matrices, sample_tokens
    x = torch.arange(tokens * 64, dtype=torch.float32).reshape(tokens, 64) / 1000
    step = max(1, tokens // 512)                     # the reference's x[0::T // 512]; every token below 512 of them
    got = sample_tokens(x)
    assert torch.equal(got, x[0::step]) and got.shape[0] == {100: 100, 512: 512, 1000: 1000}[tokens]
    assert torch.equal(sample_tokens(x, 64), x[0::max(1, tokens // 64)])
    gm = gram_matrices(x, 32)
    xs = x[0::step].double().reshape(-1, 2, 32)
    assert gm.shape == (2, 32, 32) and gm.dtype == torch.float32
    assert torch.allclose(gm.double(), torch.einsum("tjg,tjh->jgh", xs, xs) / xs.shape[0], rtol=1e-5)


def test_python_entry_points_refuse_cpu_weights(lib):
    import torch
    from qllm_amd.quantization import awq_quantize_model, clip_linear, search_scales
    from test_loader_repack_cpu import _tiny_llama
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X: qllm_amd ships no CPU quantizer"):
        awq_quantize_model(_tiny_llama(), torch.zeros((1, 8), dtype=torch.long))
    fc = torch.nn.Linear(128, 16, bias=False)
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X"):
        clip_linear(fc, torch.zeros(4, 128), 4, 128)
    with pytest.raises(RuntimeError, match="needs the weight on an MI355X"):
        search_scales(fc, [fc], torch.zeros(4, 128), {}, 4, 128)
