"""-m gpu: the sliding window of ops.attn_decode and ops.attn_prefill (qllm_attn_decode_window / qllm_attn_prefill_window) on the device, and
q_layers/fused_attention.py on tiny Mistral and Qwen2 models whose layers slide (tests/attn_sliding_cases.py).

1. Decode: windows around the tile and the split edges, at lengths that put the window's lower end inside a split's first tile, on a split
   boundary, above two and more whole splits and inside the last split; host and device length, with and without the append, no mask, bool
   and additive masks with a row whose keys inside the window are all hidden; NaN below the window and behind the length; the float64
   oracle with the band as a mask, per element within attn_decode_cases.bound; the workspace's counter page; the same bits twice; one
   captured launch replayed at lengths on both sides of the window.
2. Prefill: prompt and chunk sizes around the query tile, windows around the key tile, with and without left padding, NaN below the first
   key tile the first block reads; per element within attn_prefill_cases.bound; exact selection of the oldest visible key with a better
   match just outside the window; window with causal=False refused.
3. The modules through the real kernels: E(fused) <= M_DEVICE x E(unfused), both against float64 (printed: pytest -s; recorded in
   profiles/attn_sliding.md), the calls, a 4-bit GPTQ Mistral with every fusion, NaN behind the length of a static sliding layer."""
import functools

import pytest
import torch

import attn_decode_cases as AD
import attn_prefill_cases as AP
import attn_sliding_cases as S
import decode_loop_cases as D

from qllm_amd import ops
from qllm_amd.modeling.q_layers import install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")


def tag(dtype):
    return str(dtype)[6:]


def bits(t):
    return t.contiguous().view(torch.int16)


def dev_len(n):
    return torch.tensor(n, dtype=torch.int64, device=DEV)


def dev(t):
    return None if t is None else t.to(DEV)


CONFIGS = [(hq, hk, d, dtype) for hq, hk in S.GROUPS for d in S.DIMS for dtype in S.DTYPES]
CONFIG_IDS = [f"{hq}x{hk}-{d}-{tag(dtype)}" for hq, hk, d, dtype in CONFIGS]
configs = pytest.mark.parametrize("hq,hk,d,dtype", CONFIGS, ids=CONFIG_IDS)


# ---- 1. decode -------------------------------------------------------------------------------------------------------------------------------------
B, LMAX = 2, 2051


@functools.lru_cache(maxsize=None)
def decode_inputs(hq, hk, d, dtype):
    gen = torch.Generator().manual_seed(7 * hq + d)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    q, k, v = r(B, hq, 1, d), r(B, hk, LMAX, d), r(B, hk, LMAX, d)
    geo = AD.parse_describe(ops.attn_decode_describe(B, hq, hk, d, LMAX))
    assert geo["splits"] >= 5 and geo["chunk"] % geo["tile"] == 0
    return q, k, v, geo


def decode_windows(n, chunk):
    return sorted({w for w in (1, 2, 63, 64, 65, chunk - 1, chunk, chunk + 1, n - 1, n, n + 7) if w >= 1})


def decode_mask(kind, n, window, dtype):
    """[B, 1, 1, LMAX]: row 0 hides every third key but the newest; row 1 shows ONLY keys below the window (none at all where the window
    reaches position 0), so every key it sees inside the window is hidden: zeros."""
    if kind is None:
        return None, None
    j = torch.arange(LMAX)
    lo = max(0, n - window)
    vis = torch.stack(((j % 3 != 0) | (j == n - 1), j < lo))
    return AP.as_mask(vis[:, None, None, :], kind, dtype), vis


@pytest.mark.parametrize("where", ["boundary", "last split"])
@configs
def test_decode_windows_against_the_oracle(hq, hk, d, dtype, where):
    """n counted positions (the append included).  boundary: n = 4 chunks, so W = chunk puts the window's lower end exactly on a split
    boundary, chunk - 1 one position into a split's first tile, chunk + 1 on the last position of the split below, all three with two
    and more splits wholly below; W = 63 .. 65 put it around a tile edge inside the last live split.  last split: n = L_max, whose last split
    is ragged: the small windows lie inside it."""
    q, k, v, geo = decode_inputs(hq, hk, d, dtype)
    chunk = geo["chunk"]
    n = 4 * chunk if where == "boundary" else LMAX
    assert n <= LMAX and (LMAX - 1) // chunk == geo["splits"] - 1 and n // chunk >= 4          # four splits and more hold positions below n
    if where == "last split":
        assert (n - 2) // chunk == geo["splits"] - 1                                              # W = 1 and 2 at least start inside the ragged last split
    qd = q.to(DEV)
    scaling = d ** -0.5
    worst = 0.0
    for window in decode_windows(n, chunk):
        lo = max(0, n - window)
        for kind in (None, "bool", "additive"):
            mask, vis = decode_mask(kind, n, window, dtype)
            band = S.decode_band(n, window, LMAX).expand(B, LMAX)
            visible = band if vis is None else band & vis
            dead = ~visible.any(dim=-1)
            assert kind is None or bool(dead[1]) and not bool(dead[0])
            ref = AD.oracle(q[:, :, 0], k, v, n, scaling, visible=visible | dead[:, None])          # (a dead row: any finite numbers; zeros are asked below)
            e32 = (S.decode_restated32(q, k, v, n, mask=visible | dead[:, None], scaling=scaling).double() - ref)[~dead].abs().max().item()
            tol = AD.bound(ref, e32, dtype)
            outs = []
            for append in (False, True):
                kp, vp = k.clone(), v.clone()
                kp[:, :, :lo], vp[:, :, :lo], kp[:, :, n:], vp[:, :, n:] = NAN, NAN, NAN, NAN
                k_new = v_new = None
                if append:                                                                          # the newest token arrives through k_new / v_new
                    k_new, v_new = k[:, :, n - 1:n].to(DEV), v[:, :, n - 1:n].to(DEV)
                    kp[:, :, n - 1], vp[:, :, n - 1] = NAN, NAN
                for length in (n - append, dev_len(n - append)):
                    kd, vd = kp.to(DEV), vp.to(DEV)
                    got = ops.attn_decode(qd, kd, vd, length, k_new, v_new, mask=dev(mask), scaling=scaling, window=window)
                    again = ops.attn_decode(qd, kd, vd, length, k_new, v_new, mask=dev(mask), scaling=scaling, window=window)
                    assert int(ops.workspace(torch.device(DEV), 0)[:16384].count_nonzero()) == 0
                    got, again = got.cpu(), again.cpu()
                    assert bool(torch.isfinite(got.float()).all()), (window, kind, append)
                    assert torch.equal(bits(got), bits(again)), (window, kind, append)
                    if append:
                        assert torch.equal(bits(kd[:, :, n - 1].cpu()), bits(k[:, :, n - 1])) and torch.equal(bits(vd[:, :, n - 1].cpu()), bits(v[:, :, n - 1]))
                    assert bool((got[dead] == 0).all()), (window, kind, append)
                    err = (got.double() - ref).abs()[~dead]
                    worst = max(worst, (err / tol[~dead]).max().item())
                    assert bool((err <= tol[~dead]).all()), (window, kind, append, (err / tol[~dead]).max().item())
                    outs.append(got)
            assert all(torch.equal(bits(outs[0]), bits(o)) for o in outs[1:]), (window, kind)         # host / device length, append or not: the same bits
    print(f"sliding decode {hq}x{hk} D{d} {tag(dtype)} {where}: n {n} chunk {chunk} splits {geo['splits']} worst error / bound {worst:.3f}")


@configs
def test_decode_without_a_window_is_the_call_without_the_keyword(hq, hk, d, dtype):
    q, k, v, geo = decode_inputs(hq, hk, d, dtype)
    qd, kd, vd = q.to(DEV), k.to(DEV), v.to(DEV)
    for n in (1, geo["chunk"] + 1, LMAX):
        plain = ops.attn_decode(qd, kd, vd, n)
        assert torch.equal(bits(plain), bits(ops.attn_decode(qd, kd, vd, n, window=None)))
        assert torch.equal(bits(plain), bits(ops.attn_decode(qd, kd, vd, n, window=n)))               # a window that hides nothing: the same walk


@pytest.mark.parametrize("hq,hk,d,dtype", CONFIGS[:2] + CONFIGS[-2:], ids=CONFIG_IDS[:2] + CONFIG_IDS[-2:])
def test_one_captured_decode_launch_serves_lengths_on_both_sides_of_the_window(hq, hk, d, dtype):
    q, k, v, geo = decode_inputs(hq, hk, d, dtype)
    window = geo["chunk"] + 1
    qd, kd, vd, out = q.to(DEV), k.to(DEV), v.to(DEV), torch.empty(B, hq, d, dtype=dtype, device=DEV)
    length = dev_len(1)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attn_decode(qd, kd, vd, length, out=out, window=window)                                  # this stream's workspace exists before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            ops.attn_decode(qd, kd, vd, length, out=out, window=window)
    torch.cuda.current_stream().wait_stream(side)
    for n in (1, window - 1, window, window + 1, 3 * geo["chunk"], 3 * geo["chunk"] + 1, LMAX):
        length.fill_(n)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(bits(out), bits(ops.attn_decode(qd, kd, vd, n, window=window))), n
        assert int(ops.workspace(torch.device(DEV), 0)[:16384].count_nonzero()) == 0


# ---- 2. prefill ------------------------------------------------------------------------------------------------------------------------------------
ROWS, STARTS = (2, 127, 128, 129, 200, 300), (0, 5, 64, 100)


def prefill_windows(n):
    return (1, 2, 63, 64, 65, 127, 128, 129, 192, n, n + 5)


@functools.lru_cache(maxsize=None)
def prefill_inputs(hq, hk, d, dtype):
    gen = torch.Generator().manual_seed(11 * hq + d)
    r = lambda *shape: torch.randn(shape, generator=gen, dtype=torch.float64).to(dtype)
    return r(B, hq, max(ROWS), d), r(B, hk, max(ROWS) + max(STARTS), d), r(B, hk, max(ROWS) + max(STARTS), d)


@pytest.mark.parametrize("s", ROWS)
@configs
def test_prefill_windows_against_the_oracle(hq, hk, d, dtype, s):
    qa, ka, va = prefill_inputs(hq, hk, d, dtype)
    scaling = d ** -0.5
    qt, kt = AP.tiles(B, hq, hk, d, s, s)
    assert (qt, kt) == (128, 64)
    q = qa[:, :, :s].contiguous()
    qd = q.to(DEV)
    worst = 0.0
    for q_start in STARTS:
        n = q_start + s
        k, v = ka[:, :, :n].contiguous(), va[:, :, :n].contiguous()
        pads = (min(3, n - 1), min(70, n - 1))                                              # row 1: its first key tile wholly hidden
        for window in prefill_windows(n):
            below = kt * ((q_start - window + 1) // kt)                                       # the first key tile the first block reads starts here
            kp, vp = k.clone(), v.clone()
            if below > 0:
                kp[:, :, :below], vp[:, :, :below] = NAN, NAN
            kd, vd = kp.to(DEV), vp.to(DEV)
            band = S.prefill_band(s, n, window, n)
            for kind in (None, "bool", "additive"):
                mask = None if kind is None else AP.left_padded(B, s, q_start, n, pads, kind, dtype)
                both = band[:, None].expand(B, 1, s, n) if mask is None else S.with_band(mask, band[:, None])
                ref, pv = AP.oracle(q, k, v, n, scaling, True, both, weights=True)
                e32 = AP.fp32_error(q, k, v, n, scaling, ref, True, both)
                got = ops.attn_prefill(qd, kd, vd, n, mask=dev(mask), scaling=scaling, window=window).cpu()
                assert bool(torch.isfinite(got.float()).all()), (q_start, window, kind)
                tol = AP.bound(ref, pv, e32, dtype)
                err = (got.double() - ref).abs()
                worst = max(worst, (err / tol).max().item())
                assert bool((err <= tol).all()), (q_start, window, kind, (err / tol).max().item())
                if kind == "bool" and window == 65:
                    assert torch.equal(bits(got), bits(ops.attn_prefill(qd, kd, vd, dev_len(n), mask=dev(mask), scaling=scaling, window=window).cpu()))
    print(f"sliding prefill {hq}x{hk} D{d} {tag(dtype)} S{s}: worst error / bound {worst:.3f}")


@pytest.mark.parametrize("s", ROWS)
@configs
def test_prefill_selects_the_oldest_visible_key_bit_for_bit(hq, hk, d, dtype, s):
    for q_start in STARTS:
        n = q_start + s
        for window in prefill_windows(n):
            q, k, v, target, scaling = S.window_selection(B, hq, hk, d, s, q_start, window, dtype)
            got = ops.attn_prefill(q.to(DEV), k.to(DEV), v.to(DEV), n, scaling=scaling, window=window).cpu()
            want = S.window_selection_expected(v, target, hq)
            wrong = (bits(got) != bits(want)).any(dim=-1)
            assert not bool(wrong.any()), (q_start, window, "first wrong (b, i, h)", wrong.nonzero()[:4].tolist())


def test_prefill_without_a_window_and_without_causality():
    qa, ka, va = prefill_inputs(8, 2, 64, torch.float16)
    q, k, v = qa[:, :, :129].to(DEV), ka[:, :, :200].to(DEV), va[:, :, :200].to(DEV)
    plain = ops.attn_prefill(q, k, v, 200)
    assert torch.equal(bits(plain), bits(ops.attn_prefill(q, k, v, 200, window=None)))
    with pytest.raises(ops.QllmUnsupported, match="causal"):
        ops.attn_prefill(q, k, v, 200, causal=False, window=64)
    ops.attn_prefill(q, k, v, 200, causal=False)


# ---- 3. the modules ----------------------------------------------------------------------------------------------------------------------------------
_models = {}


def tier_a(name):
    if name not in _models:
        model, slides, window = S.sliding_model(name, device=DEV)
        _models[name] = (model, D.float64_copy(model), slides, window)
    return _models[name]


def recorded(monkeypatch):
    return S.record(monkeypatch, ops.attn_decode, ops.attn_prefill)


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_sliding_layers_decode_within_the_bound(name, cache, batch, monkeypatch):
    from test_attn_sliding_cpu import check_decode_calls
    model, ref, slides, window = tier_a(name)
    inp = D.batch_inputs(batch)
    reference, unfused = D.run(ref, inp), D.run(model, inp, cache, DEV)
    calls = recorded(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model) == D.LAYERS
    try:
        fused = D.run(model, inp, cache, DEV)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    check_decode_calls(calls, cache, slides, window, inp)
    D.assert_case(fused, unfused, reference, D.M_DEVICE, label=f"sliding {name} {cache} {batch}")


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
@pytest.mark.parametrize("name", list(S.MODELS))
def test_prompts_and_chunks_on_sliding_layers_within_the_bound(name, cache, batch, monkeypatch):
    from test_attn_sliding_cpu import PIECES
    model, ref, slides, window = tier_a(name)
    inp = D.batch_inputs(batch)
    reference, _ = S.forwards(ref, inp, "dynamic", "cpu", PIECES)
    unfused, _ = S.forwards(model, inp, cache, DEV, PIECES)
    calls = recorded(monkeypatch)
    S.open_routes(monkeypatch)
    assert install_fused_rope(model) == D.LAYERS and install_fused_attention(model, prefill=True) == D.LAYERS
    try:
        fused, _ = S.forwards(model, inp, cache, DEV, PIECES)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS and uninstall_fused_rope(model) == D.LAYERS
    assert [(c.op, c.q_len) for c in calls] == [("prefill", 5)] * D.LAYERS + [("prefill", 3)] * D.LAYERS + [("decode", 1)] * (2 * D.LAYERS)
    assert [c.window for c in calls] == [window if s else None for s in slides] * 4
    assert bool(torch.isfinite(fused.float()).all())
    e_unfused, e_fused = (unfused.double() - reference).abs().max().item(), (fused.double() - reference).abs().max().item()
    print(f"sliding prefill modules {name} {cache} {batch}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    assert e_unfused > 0 and e_fused <= D.M_DEVICE * e_unfused


def test_a_static_sliding_layer_before_it_fills_over_a_tail_of_nan(monkeypatch):
    """mistral-8: the 5-token prompt and the first three steps leave the layers of 8 positions unfilled; the slots behind the length hold
    NaN from the prompt on, the family's own prompt having run before."""
    model, ref, slides, window = tier_a("mistral-8")
    inp = D.batch_inputs("padded")
    reference, unfused = D.run(ref, inp, steps=3), D.run(model, inp, "static", DEV, steps=3)
    calls = recorded(monkeypatch)
    assert install_fused_attention(model) == D.LAYERS
    try:
        fused = D.run(model, inp, "static", DEV, poison=True, steps=3)
    finally:
        assert uninstall_fused_attention(model) == D.LAYERS
    assert [(c.length, c.on_device) for c in calls] == [(n, True) for n in (6, 6, 7, 7, 8, 8)]
    D.assert_case(fused, unfused, reference, D.M_DEVICE, label="sliding mistral-8 static padded, poisoned tail")


@pytest.fixture(scope="module")
def tier_b(tmp_path_factory):
    from qllm_amd.modeling import base
    qmodel = S.quantized_mistral()
    d = str(tmp_path_factory.mktemp("attn_sliding") / "ckpt")
    base.save_quantized(qmodel, d)
    plain = base.load_quantized(d, device=DEV)
    fused = base.load_quantized(d, device=DEV, fuse_mlp=True, fuse_norm=True, fuse_residual=True, fuse_rope=True, fuse_attention=True, fuse_attention_prefill=True)
    assert (fused.fused_attentions, fused.fused_attention_prefills, fused.fused_ropes) == (2, 2, 2) and plain.config.sliding_window == 4
    return plain, fused, S.dense_mistral_reference(qmodel)


@pytest.mark.parametrize("batch", ["padded", "unpadded"])
@pytest.mark.parametrize("cache", ["dynamic", "static"])
def test_a_quantized_mistral_with_every_fusion_against_the_plain_load(cache, batch, tier_b, monkeypatch):
    from qllm_amd.modeling.q_layers import fused_attention
    plain, fused, ref = tier_b
    inp = D.batch_inputs(batch, prompt=8)                                                   # two windows: the prompt PREFILL_ROUTES routes
    reference, unfused = D.run(ref, inp), D.run(plain, inp, cache, DEV)
    calls = recorded(monkeypatch)
    got = D.run(fused, inp, cache, DEV)
    kind = ("static" if cache == "static" else "dynamic") + "_sliding"
    assert fused_attention._prefill_routed(kind, True, inp.prompt, False, 4)                # (both batches reach the layers with a mask: 8 > 4)
    assert [(c.op, c.q_len) for c in calls] == [("prefill", 8)] * D.LAYERS + [("decode", 1)] * (D.LAYERS * inp.steps) and all(c.window == 4 for c in calls)
    assert bool(torch.isfinite(got.steps.float()).all())
    e_unfused, e_fused = D.error(unfused, reference), D.error(got, reference)
    print(f"sliding quantized mistral {cache} {batch}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e} ratio {e_fused / e_unfused:.3f}")
    assert e_unfused > 0 and e_fused <= D.M_DEVICE * e_unfused
