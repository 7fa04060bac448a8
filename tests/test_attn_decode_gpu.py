"""-m gpu: single-token attention over the KV cache as one kernel (qllm_attn_decode, csrc/attn_decode.hip) through ops.attn_decode and
the modules of q_layers/fused_attention.py.

Shapes.  The tile T, the split count S and the positions per split come from qllm_attn_decode_describe; L_max = S * T + 3 of the answer
for 1024 positions (at most 2051), so the last split is ragged.  Lengths: 1, 2, T - 1, T, T + 1, the last position of a middle split and
the first of the next, L_max - 1, L_max.  Heads (1, 1), (4, 4), (8, 2), (28, 4), (32, 8); head_dim 64 and 128; batch 1 and 3; fp16 and bf16.

Exact tests (bit for bit): one key wins (integer q and K put one score at least 40 above every other: the other weights are below 2^-57
and vanish in fp32), uniform weights (q = 0, integer V whose mean is representable).  Accuracy on N(0, 1) values: the float64 oracle
(tests/attn_decode_cases.py) from the same rounded inputs; the kernel's maximum absolute error must not exceed that of transformers' eager
arithmetic in the activation type on the CPU, per case, with no margin.  Both figures are printed per case (pytest -s)."""
import pytest
import torch

from attn_decode_cases import BATCHES, DIMS, DTYPES, HEADS, eager, oracle, parse_describe

from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = [(hq, hk, d, b, dt) for (hq, hk) in HEADS for d in DIMS for b in BATCHES for dt in DTYPES]
IDS = [f"{hq}x{hk}-d{d}-b{b}-{str(dt)[6:]}" for hq, hk, d, b, dt in CASES]


def geometry(b, hq, hk, d):
    g0 = parse_describe(ops.attn_decode_describe(b, hq, hk, d, 1024))
    lmax = min(g0["splits"] * g0["tile"] + 3, 2051)
    g = parse_describe(ops.attn_decode_describe(b, hq, hk, d, lmax))
    assert g["splits"] >= 3 and g["chunk"] % g["tile"] == 0 and (g["splits"] - 1) * g["chunk"] < lmax <= g["splits"] * g["chunk"], g
    return lmax, g


def lengths(lmax, g):
    t, c, mid = g["tile"], g["chunk"], max(1, g["splits"] // 2)
    return sorted({n for n in (1, 2, t - 1, t, t + 1, mid * c, mid * c + 1, lmax - 1, lmax) if 1 <= n <= lmax})


def randn(shape, dtype, gen):
    return torch.randn(shape, generator=gen).to(dtype)


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_one_key_wins_bit_for_bit(hq, hk, d, b, dtype):
    """q = 16 e_g (g: the head's place in its group) plus +-1 noise in columns 8..23; K +-1 noise in the same columns and 16 in column g
    of the position where head g of the group wins; scaling 0.25: the winner scores at least 60, every other at most 4.  The output must
    be the winner's V row of the head's kv head.  Two sweeps, one launch each step:
    - kv_len = L_max, and query head h of batch entry i wins at the (h + i + r)-th position of the length list, for every rotation r:
      every query head wins once at every chosen position, with all splits live;
    - kv_len = each length n of the list, and every head wins at position n - 1, the last one that counts: the live splits are fewer than
      the grid's, the last live one is ragged, and the positions behind it hold a key (16 in every column of the group, V of 64) that
      would win if it were read."""
    lmax, geo = geometry(b, hq, hk, d)
    ls, grp = lengths(lmax, geo), hq // hk
    gen = torch.Generator().manual_seed(hq * 131 + d + b)
    v = torch.randint(1, 9, (b, hk, lmax, d), generator=gen).float() * (torch.randint(0, 2, (b, hk, lmax, d), generator=gen) * 2 - 1)
    k = torch.zeros(b, hk, lmax, d)
    k[..., 8:24] = torch.randint(-1, 2, (b, hk, lmax, 16), generator=gen).float()
    q = torch.zeros(b, hq, d)
    q[..., 8:24] = torch.randint(-1, 2, (b, hq, 16), generator=gen).float()
    noise = torch.einsum("bkgd,bknd->bkgn", q.view(b, hk, grp, d), k) * 0.25        # every score but for the winners' 16 * 16 * 0.25 = 64
    assert 64 - 2 * noise.abs().max().item() >= 40
    bi, hi = torch.meshgrid(torch.arange(b), torch.arange(hq), indexing="ij")
    q[bi, hi, hi % grp] = 16.0
    qd, kd, vd = q.to(dtype)[:, :, None].to(DEV), k.to(dtype).to(DEV), v.to(dtype).to(DEV)
    v, at = v.to(dtype), torch.tensor(ls)
    bi_d, hi_d = bi.to(DEV), hi.to(DEV)
    for r in range(len(ls)):
        pos = at[(hi + bi + r) % len(ls)] - 1                                       # [B, Hq]
        k1 = kd.clone()
        k1[bi_d, hi_d // grp, pos.to(DEV), hi_d % grp] = 16.0
        got = ops.attn_decode(qd, k1, vd, lmax, scaling=0.25).cpu()
        assert torch.equal(got.view(torch.int16), v[bi, hi // grp, pos].view(torch.int16)), r
    for n in ls:
        k1, v1 = kd.clone(), vd.clone()
        k1[:, :, n - 1:, :grp] = 16.0
        v1[:, :, n:] = 64.0
        got = ops.attn_decode(qd, k1, v1, n, scaling=0.25).cpu()
        assert torch.equal(got.view(torch.int16), v[bi, hi // grp, n - 1].view(torch.int16)), n


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_uniform_weights_exact_mean(hq, hk, d, b, dtype):
    """q = 0: every weight is 1 / kv_len.  V: integers of magnitude <= 8; from position 16 on they come in pairs (x, -x), so the sum over a
    power-of-two length is the sum of at most 16 values (magnitude <= 128) and the mean is representable in both types."""
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(hq + d + b)
    v = torch.randint(-8, 9, (b, hk, lmax, d), generator=gen).float()
    v[:, :, 17:lmax:2] = -v[:, :, 16:lmax - 1:2]
    k = randn((b, hk, lmax, d), dtype, gen)
    q = torch.zeros(b, hq, d, dtype=dtype)
    kd, vd, qd = k.to(DEV), v.to(dtype).to(DEV), q[:, :, None].to(DEV)
    n = 1
    while n <= lmax:
        mean = v[:, :, :n].double().mean(dim=2)
        want = mean.to(dtype)
        assert torch.equal(want.double(), mean)
        got = ops.attn_decode(qd, kd, vd, n).cpu()
        assert torch.equal(got, want.repeat_interleave(hq // hk, dim=1)), n
        n *= 2


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_accuracy_against_the_eager_arithmetic(hq, hk, d, b, dtype):
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(7 * hq + d + b)
    q, k, v = randn((b, hq, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen)
    kd, vd, qd = k.to(DEV), v.to(DEV), q[:, :, None].to(DEV)
    bad = []
    for n in lengths(lmax, geo):
        ref = oracle(q, k, v, n, d ** -0.5)
        got = ops.attn_decode(qd, kd, vd, n).cpu()
        e_kernel = (got.double() - ref).abs().max().item()
        e_eager = (eager(q, k, v, n, d ** -0.5).double() - ref).abs().max().item()
        print(f"accuracy {hq}x{hk} d={d} b={b} {str(dtype)[6:]} kv_len={n}: kernel {e_kernel:.3e} eager {e_eager:.3e}")
        assert torch.isfinite(got).all()
        if e_kernel > e_eager:
            bad.append((n, e_kernel, e_eager))
    assert not bad, bad


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_nothing_beyond_the_length_is_read(hq, hk, d, b, dtype):
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(3)
    q, k, v = randn((b, hq, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen)
    qd = q[:, :, None].to(DEV)
    for n in lengths(lmax, geo):
        kz, vz, kn, vn = k.clone(), v.clone(), k.clone(), v.clone()
        kz[:, :, n:], vz[:, :, n:], kn[:, :, n:], vn[:, :, n:] = 0, 0, float("nan"), float("nan")
        a = ops.attn_decode(qd, kz.to(DEV), vz.to(DEV), n)
        c = ops.attn_decode(qd, kn.to(DEV), vn.to(DEV), n)
        assert torch.isfinite(c).all() and torch.equal(a.view(torch.int16), c.view(torch.int16)), n


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_masks_bool_and_additive(hq, hk, d, b, dtype):
    """Batch entry i hides a left-padded prefix of its own: none, half and all of the keys at batch 3; half, then all, in two calls at
    batch 1.  The entry that hides everything must store zeros."""
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(5)
    q, k, v = randn((b, hq, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen)
    kd, vd, qd = k.to(DEV), v.to(DEV), q[:, :, None].to(DEV)
    for n in lengths(lmax, geo):
        for hidden in ([[0, n // 2, n]] if b == 3 else [[n // 2], [n]]):
            visible = torch.ones(b, lmax, dtype=torch.bool)
            for i, hcount in enumerate(hidden):
                visible[i, :hcount] = False
            additive = torch.zeros(b, lmax, dtype=dtype).masked_fill(~visible, torch.finfo(dtype).min)
            got_b = ops.attn_decode(qd, kd, vd, n, mask=visible.to(DEV)[:, None, None, :]).cpu()
            got_a = ops.attn_decode(qd, kd, vd, n, mask=additive.to(DEV)[:, None, None, :]).cpu()
            assert torch.equal(got_b.view(torch.int16), got_a.view(torch.int16)), n
            live = [i for i, hcount in enumerate(hidden) if hcount < n]
            dead = [i for i, hcount in enumerate(hidden) if hcount >= n]
            assert torch.equal(got_b[dead], torch.zeros_like(got_b[dead]))
            if live:
                ref = oracle(q[live], k[live], v[live], n, d ** -0.5, visible[live])
                e_kernel = (got_b[live].double() - ref).abs().max().item()
                e_eager = (eager(q[live], k[live], v[live], n, d ** -0.5, additive[live]).double() - ref).abs().max().item()
                print(f"masked {hq}x{hk} d={d} b={b} {str(dtype)[6:]} kv_len={n}: kernel {e_kernel:.3e} eager {e_eager:.3e}")
                assert e_kernel <= e_eager, (n, e_kernel, e_eager)


@pytest.mark.parametrize("device_length", (False, True), ids=("host", "device"))
@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_append_stores_the_row_and_nothing_else(hq, hk, d, b, dtype, device_length):
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(9)
    q, k, v = randn((b, hq, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen)
    k_new, v_new = randn((b, hk, d), dtype, gen), randn((b, hk, d), dtype, gen)
    qd, knd, vnd = q[:, :, None].to(DEV), k_new[:, :, None].to(DEV), v_new[:, :, None].to(DEV)
    for n in [x - 1 for x in lengths(lmax, geo)]:
        kd, vd = k.to(DEV), v.to(DEV)
        kd[:, :, n], vd[:, :, n] = float("nan"), float("nan")      # the row the append overwrites is never read
        length = torch.tensor(n, dtype=torch.int64, device=DEV) if device_length else n
        got = ops.attn_decode(qd, kd, vd, length, knd, vnd)
        k2, v2 = k.clone(), v.clone()
        k2[:, :, n], v2[:, :, n] = k_new, v_new
        assert torch.equal(kd.cpu().view(torch.int16), k2.view(torch.int16)) and torch.equal(vd.cpu().view(torch.int16), v2.view(torch.int16)), n
        plain = ops.attn_decode(qd, k2.to(DEV), v2.to(DEV), n + 1)
        assert torch.equal(got.view(torch.int16), plain.view(torch.int16)), n
    if device_length:   # the cache is full: nothing is stored, the first L_max positions are attended
        kd, vd = k.to(DEV), v.to(DEV)
        got = ops.attn_decode(qd, kd, vd, torch.tensor(lmax, dtype=torch.int64, device=DEV), knd, vnd)
        assert torch.equal(kd.cpu().view(torch.int16), k.view(torch.int16)) and torch.equal(vd.cpu().view(torch.int16), v.view(torch.int16))
        assert torch.equal(got, ops.attn_decode(qd, kd, vd, lmax))


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_strided_views_give_the_same_bits(hq, hk, d, b, dtype):
    """q, k_new and v_new as slices of one [B, (Hq + 2 Hkv) D] buffer (what a fused q/k/v projection returns) and contiguous."""
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(11)
    k, v = randn((b, hk, lmax, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen)
    buf = randn((b, 1, (hq + 2 * hk) * d), dtype, gen).to(DEV)
    qs = buf[..., :hq * d].view(b, 1, hq, d).transpose(1, 2)
    ks = buf[..., hq * d:(hq + hk) * d].view(b, 1, hk, d).transpose(1, 2)
    vs = buf[..., (hq + hk) * d:].view(b, 1, hk, d).transpose(1, 2)
    n = lengths(lmax, geo)[-3] - 1
    k1, v1, k2, v2 = k.to(DEV), v.to(DEV), k.to(DEV), v.to(DEV)
    a = ops.attn_decode(qs, k1, v1, n, ks, vs)
    c = ops.attn_decode(qs.contiguous(), k2, v2, n, ks.contiguous(), vs.contiguous())
    e = ops.attn_decode(qs.transpose(1, 2), k2, v2, n + 1)        # [B, 1, Hq, D], no append: the row is there already
    assert torch.equal(a.view(torch.int16), c.view(torch.int16)) and torch.equal(a.view(torch.int16), e.view(torch.int16))
    assert torch.equal(k1, k2) and torch.equal(v1, v2)


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_same_bits_every_call_and_a_clean_counter_page(hq, hk, d, b, dtype):
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(13)
    q, k, v = randn((b, hq, 1, d), dtype, gen).to(DEV), randn((b, hk, lmax, d), dtype, gen).to(DEV), randn((b, hk, lmax, d), dtype, gen).to(DEV)
    for n in (lengths(lmax, geo)[5], lmax):
        first = ops.attn_decode(q, k, v, n)
        for _ in range(3):
            again = ops.attn_decode(q, k, v, n)
            assert torch.equal(first.view(torch.int16), again.view(torch.int16))
            assert int(ops.workspace(torch.device(DEV), 0)[:16384].count_nonzero()) == 0


@pytest.mark.parametrize("hq,hk,d,b,dtype", CASES, ids=IDS)
def test_one_captured_launch_serves_every_length(hq, hk, d, b, dtype):
    """One captured launch with the length on the device plus the add_, replayed while the length walks across a split boundary."""
    lmax, geo = geometry(b, hq, hk, d)
    gen = torch.Generator().manual_seed(17)
    q = randn((b, hq, 1, d), dtype, gen).to(DEV)
    k, v = randn((b, hk, lmax, d), dtype, gen), randn((b, hk, lmax, d), dtype, gen)
    k_new, v_new = randn((b, hk, 1, d), dtype, gen).to(DEV), randn((b, hk, 1, d), dtype, gen).to(DEV)
    start, steps = geo["chunk"] - 3, 6
    kd, vd, out = k.to(DEV), v.to(DEV), torch.empty(b, hq, d, dtype=dtype, device=DEV)
    length = torch.tensor(1, dtype=torch.int64, device=DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_decode(q, kd.clone(), vd.clone(), length, k_new, v_new, out=out)      # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.attn_decode(q, kd, vd, length, k_new, v_new, out=out)
            length.add_(1)
    torch.cuda.current_stream().wait_stream(side)
    kd.copy_(k), vd.copy_(v)
    for n in [1, 2] + list(range(start, start + steps)):
        length.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        assert int(length) == n + 1
        k2, v2 = kd.clone(), vd.clone()
        plain = ops.attn_decode(q, k2, v2, n + 1)
        assert torch.equal(out.view(torch.int16), plain.view(torch.int16)), n
        assert torch.equal(kd[:, :, n], k_new[:, :, 0]) and torch.equal(vd[:, :, n], v_new[:, :, 0])


# ---- the modules -----------------------------------------------------------------------------------------------------------------------------
def _count(monkeypatch):
    calls = {"attn": 0}
    real = ops.attn_decode

    def attn_decode(*a, **kw):
        calls["attn"] += 1
        return real(*a, **kw)

    monkeypatch.setattr(ops, "attn_decode", attn_decode)
    return calls


@pytest.mark.parametrize("kind", ["dynamic", "static"])
@pytest.mark.parametrize("attn", ["sdpa", "eager"])
@pytest.mark.parametrize("family", ["llama", "mistral", "qwen2"])
def test_tiny_models_decode_with_the_kernel(family, attn, kind, monkeypatch):
    """tests/test_attn_decode_cpu.py's tiny models in fp16 on the device with the real op: a 5-token prefill of a batch of two and 4 decode
    steps.  The prefill is the family's own (the same bits); the decode logits are held to the CPU file's bound (2e-2 on logits below 2:
    the kernel rounds once where the replaced route rounds scores, weights and output)."""
    from test_attn_decode_cpu import close, module_dicts, prefill_and_decode, tiny_model
    from qllm_amd.modeling.q_layers import install_fused_attention, uninstall_fused_attention
    model = tiny_model(family, attn, device=DEV)
    before = module_dicts(model)
    want, want_cache = prefill_and_decode(model, kind, DEV, batch=2)
    calls = _count(monkeypatch)
    assert install_fused_attention(model) == 2
    got, got_cache = prefill_and_decode(model, kind, DEV, batch=2)
    assert calls["attn"] == 2 * 4
    assert torch.equal(got[0], want[0]) and close(got, want)
    if kind == "static":
        for a, b in zip(got_cache.layers, want_cache.layers):
            assert int(a.cumulative_length) == int(b.cumulative_length) == 9
            assert torch.equal(a.keys[:, :, 9:], b.keys[:, :, 9:]) and torch.equal(a.values[:, :, 9:], b.values[:, :, 9:])
    assert uninstall_fused_attention(model) == 2 and module_dicts(model) == before
    again, _ = prefill_and_decode(model, kind, DEV, batch=2)
    assert all(torch.equal(a, w) for a, w in zip(again, want)) and calls["attn"] == 2 * 4


@pytest.mark.parametrize("order", ["attention_last", "attention_first"])
def test_llama_decoder_layer_with_all_five_fusions(order, monkeypatch):
    """The quantized decoder layer of tests/test_residual_gpu.py with fuse_mlp, fuse_norm, fuse_residual, fuse_rope and fuse_attention
    installed in two orders: a 5-row prefill and three decode rows through a DynamicCache against the layer with the other four only."""
    from transformers import DynamicCache
    from gpu_util import randx
    from test_residual_gpu import _tiny_layer
    from qllm_amd.modeling.q_layers import (install_fused_attention, install_fused_mlp, install_fused_norm, install_fused_residual, install_fused_rope,
                                            uninstall_fused_attention, uninstall_fused_mlp, uninstall_fused_norm, uninstall_fused_residual,
                                            uninstall_fused_rope)
    layer, rot = _tiny_layer("GPTQ", 128)
    layer.self_attn.config._attn_implementation = "sdpa"
    q = [type(layer.mlp.down_proj)]
    xs = [(torch.from_numpy(randx(m, 256, seed=m + i)) * 0.5).to(DEV).view(1, m, 256) for i, m in enumerate((5, 1, 1, 1))]

    def steps():
        cache, outs, at = DynamicCache(config=layer.self_attn.config), [], 0
        with torch.no_grad():
            for x in xs:
                pos = torch.arange(at, at + x.shape[1], device=DEV).unsqueeze(0)
                outs.append(layer(x.clone(), attention_mask=None, position_ids=pos, past_key_values=cache, position_embeddings=rot(x, pos)))
                at += x.shape[1]
        return outs

    four = lambda: (install_fused_mlp(layer, q) == 1 and install_fused_norm(layer, q) == 2 and install_fused_residual(layer, q) == 1  # noqa: E731
                    and install_fused_rope(layer) == 1)
    assert four()
    want = steps()
    assert all(bool(torch.isfinite(w.float()).all()) for w in want)
    calls = _count(monkeypatch)
    if order == "attention_last":
        assert install_fused_attention(layer) == 1
    else:
        assert uninstall_fused_rope(layer) == 1 and uninstall_fused_residual(layer) == 1 and uninstall_fused_norm(layer) == 2 and uninstall_fused_mlp(layer) == 1
        assert install_fused_attention(layer) == 1 and four()
    got = steps()
    assert calls["attn"] == 3 and torch.equal(got[0], want[0])
    scale = max(w.float().abs().max().item() for w in want)
    for g, w in zip(got, want):
        assert bool(torch.isfinite(g.float()).all()) and (g.float() - w.float()).abs().max().item() <= 2e-2 * max(1.0, scale)
    assert uninstall_fused_attention(layer) == 1
    assert all(torch.equal(g, w) for g, w in zip(steps(), want)) and calls["attn"] == 3
    assert uninstall_fused_rope(layer) == 1 and uninstall_fused_residual(layer) == 1 and uninstall_fused_norm(layer) == 2 and uninstall_fused_mlp(layer) == 1
    assert not any("forward" in m.__dict__ for m in layer.modules())


def test_load_quantized_with_fuse_attention_generates_the_same_tokens(tmp_path, monkeypatch):
    """load_quantized(fuse_attention=True) against the default load of a saved tiny checkpoint: 8 greedy steps through a KV cache, the same
    tokens; one kernel per layer and decode step, none at the prefill."""
    from test_loader_repack_cpu import _quantize_in_place, _tiny_llama
    from qllm_amd.modeling import base
    model, _ = _quantize_in_place(_tiny_llama(), "GPTQ")
    d = str(tmp_path / "ckpt")
    base.save_quantized(model, d)
    plain = base.load_quantized(d, device=DEV)
    assert not hasattr(plain, "fused_attentions")                                      # off by default
    fused = base.load_quantized(d, device=DEV, fuse_attention=True)
    assert fused.fused_attentions == 2
    calls = _count(monkeypatch)
    tok_p = tok_f = torch.tensor([[5, 9, 2]], device=DEV)
    pkv_p = pkv_f = None
    with torch.no_grad():
        for step in range(8):
            op = plain(tok_p, past_key_values=pkv_p, use_cache=True)
            of = fused(tok_f, past_key_values=pkv_f, use_cache=True)
            pkv_p, pkv_f = op.past_key_values, of.past_key_values
            tok_p, tok_f = op.logits[:, -1:].argmax(-1), of.logits[:, -1:].argmax(-1)
            assert torch.equal(tok_p, tok_f), step
    assert calls["attn"] == 2 * 7
