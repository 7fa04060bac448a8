"""-m gpu: the AWQ quantizer (qllm_awq_quantize, qllm_awq_clip_search, csrc/awq_quant.hip; qllm_amd/quantization/awq.py) against fixtures
minted from the reference's own pseudo_quantize_tensor, auto_clip_layer and _search_module_scale
(tests/golden/make_goldens_awq_quant.py -> tests/golden/awq_quant/).

Bounds.  The pseudo-quantizer is specified operation by operation in fp32: bit-equal.  The clip search sums the reference's output error in
another order (a quadratic form over an fp32 Gram matrix): the chosen candidate may differ where two candidates' errors are within
rounding of each other.  The fixtures are chosen so that the reference agrees with an fp64 evaluation in every group; the kernel may
differ from it in <= 0.5 % of the (row, group) pairs, and where it does its choice is within 1e-4 relative of the fp64 minimum; its two
errors are within 1e-4 relative of fp64 (the form in fp32 agrees with fp64 to about 1e-6).  The scale search must find the fixture's
ratio, which the maker accepted only where the best fp64 loss is >= 1 % below the runner-up.

Measured on an MI355X: profiles/awq_quantize.md."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "awq_quant")
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "awqq_*.npz")))
VARIANTS = {"plain": (False, False), "scale": (True, False), "clip": (False, True), "scale_clip": (True, True)}
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
N_GRID, N_CAND = 20, 10
_fix, _clip = {}, {}


def fixture(name):
    if name not in _fix:
        d = dict(np.load(os.path.join(GOLD, name + ".npz"), allow_pickle=False))
        for k in ("bits", "groupsize", "N", "K", "seed"):
            d[k] = int(d[k])
        d["w_dtype"] = DTYPES[str(d["w_dtype"])]
        _fix[name] = d
    return _fix[name]


def weight(d, dtype):
    W = torch.from_numpy(d["W"]).to(dtype).to(DEV).contiguous()
    assert torch.equal(W.float().cpu(), torch.from_numpy(d["W"]))     # exactly representable
    return W


def operands(d, variant):
    use_s, use_c = VARIANTS[variant]
    return (torch.from_numpy(d["col_scale"]).to(DEV) if use_s else None), (torch.from_numpy(d["best_max"]).to(DEV) if use_c else None)


def emulate(W32, dtype, s, clip, bits, g):
    """The arithmetic of qllm_awq_quantize on the host, in fp32 (IEEE division, round half to even), for W stored as `dtype`."""
    N, K = W32.shape
    maxq = float(2 ** bits - 1)
    v = W32.clone()
    if s is not None:
        v = (v * s.view(1, -1)).to(dtype).float()
    v = v.view(N, K // g, g)
    if clip is not None:
        v = torch.minimum(torch.maximum(v, -clip.unsqueeze(-1)), clip.unsqueeze(-1))
    vmax, vmin = v.amax(-1, keepdim=True), v.amin(-1, keepdim=True)
    sc = (vmax - vmin).clamp(min=1e-5) / maxq
    z = (-torch.round(vmin / sc)).clamp(0, maxq)
    code = (torch.round(v / sc) + z).clamp(0, maxq)
    wq = ((code - z) * sc).view(N, K)
    if s is not None:
        wq = wq / s.view(1, -1)
    return code.view(N, K).to(torch.int32), sc.squeeze(-1), z.squeeze(-1), wq.to(dtype)


# ---- the pseudo-quantizer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", NAMES)
def test_quantize_fp32_equals_the_reference_bit_for_bit(name, variant):
    d = fixture(name)
    s, clip = operands(d, variant)
    codes, scales, zeros, wq = ops.awq_quantize(weight(d, torch.float32), d["bits"], d["groupsize"], col_scale=s, clip=clip)
    assert np.array_equal(codes.cpu().numpy().T, d[f"codes_{variant}"].astype(np.int32))
    assert np.array_equal(scales.cpu().numpy(), d[f"scales_{variant}"]) and np.array_equal(zeros.cpu().numpy(), d[f"zeros_{variant}"])
    assert np.array_equal(wq.cpu().numpy(), d[f"wq_{variant}"])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name", NAMES)
def test_quantize_16_bit_storage_equals_the_emulation_bit_for_bit(name, variant):
    d = fixture(name)
    g, dtype = d["groupsize"], d["w_dtype"]
    s, clip = operands(d, variant)
    W = weight(d, dtype)
    codes, scales, zeros, wq = ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip)
    e_codes, e_sc, e_z, e_wq = emulate(torch.from_numpy(d["W"]), dtype, None if s is None else s.cpu(), None if clip is None else clip.cpu(),
                                       d["bits"], g)
    assert torch.equal(codes.cpu().t(), e_codes) and torch.equal(scales.cpu(), e_sc) and torch.equal(zeros.cpu(), e_z)
    assert torch.equal(wq.cpu().view(torch.int16), e_wq.view(torch.int16))
    # wq is the grid point of its own code, divided by the column scale, in W's dtype
    own = (codes.t().float() - zeros.repeat_interleave(g, 1)) * scales.repeat_interleave(g, 1)
    if s is not None:
        own = own / s.view(1, -1)
    assert torch.equal(wq, own.to(dtype))
    assert 0 <= int(codes.min()) and int(codes.max()) <= 2 ** d["bits"] - 1
    # NULL outputs are skipped: the others do not change
    only = ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip, want=("wq",))
    assert only[:3] == (None, None, None) and torch.equal(only[3], wq)
    some = ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip, want=("codes", "zeros"))
    assert some[1] is None and some[3] is None and torch.equal(some[0], codes) and torch.equal(some[2], zeros)


# ---- the clip search --------------------------------------------------------------------------------------------------------------------
def gram_of(d):
    from qllm_amd.quantization.awq import gram_matrices
    return gram_matrices(torch.from_numpy(d["X"]).to(DEV), d["groupsize"], n_sample_token=64)


def clip_run(name):
    if name not in _clip:
        d = fixture(name)
        W, gm = weight(d, d["w_dtype"]), gram_of(d)
        out = ops.awq_clip_search(W, gm, d["bits"], d["groupsize"])
        torch.cuda.synchronize()
        _clip[name] = (W, gm, out)
    return _clip[name]


@pytest.mark.parametrize("name", NAMES)
def test_clip_search_chooses_the_reference_candidates(name):
    d = fixture(name)
    N, K, g = d["N"], d["K"], d["groupsize"]
    W, gm, (best_max, best_idx, err) = clip_run(name)
    idx, err, err64 = best_idx.cpu().numpy(), err.cpu().numpy().astype(np.float64), d["err64"]
    assert idx.min() >= 0 and idx.max() < N_CAND
    differ = idx != d["best_idx"]
    at = np.take_along_axis(err64, idx[..., None].astype(np.int64), -1)[..., 0]
    excess = float((at / err64.min(-1))[differ].max()) - 1 if differ.any() else 0.0
    rel0, rel1 = np.abs(err[..., 0] / err64[..., 0] - 1).max(), np.abs(err[..., 1] / at - 1).max()
    print(f"clip {name}: {int(differ.sum())} of {differ.size} (row, group) pairs differ ({differ.mean():.4%}), worst excess over the fp64 "
          f"minimum {excess:.2e}; |err / err64 - 1| unclipped {rel0:.2e} chosen {rel1:.2e}; clipped {float((idx > 0).mean()):.1%}")
    assert differ.mean() <= 0.005
    assert excess <= 1e-4
    org = np.abs(d["W"].reshape(N, K // g, g)).max(-1)
    factor = np.array([1 - i / N_GRID for i in range(N_CAND)]).astype(np.float32)
    assert np.array_equal(best_max.cpu().numpy(), org * factor[idx])
    assert (err[..., 1] <= err[..., 0]).all()
    assert rel0 <= 1e-4 and rel1 <= 1e-4


# ---- memory and launch behaviour --------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", ["awqq_w4_g128_k384", "awqq_w3_g64", "awqq_w4_g32"])
def test_repeatable_and_independent_of_the_storage_dtype(name):
    d = fixture(name)
    W, gm, first = clip_run(name)
    assert _same(first, ops.awq_clip_search(W, gm, d["bits"], d["groupsize"]))
    assert _same(first, ops.awq_clip_search(W.float(), gm, d["bits"], d["groupsize"]))
    s, clip = operands(d, "scale_clip")
    q = ops.awq_quantize(W, d["bits"], d["groupsize"], clip=clip)
    assert _same(q, ops.awq_quantize(W, d["bits"], d["groupsize"], clip=clip))
    wide = ops.awq_quantize(W.float(), d["bits"], d["groupsize"], clip=clip)       # (a column scale rounds in the storage dtype)
    assert _same(q[:3], wide[:3]) and torch.equal(wide[3].to(W.dtype), q[3])


def _alloc(specs, guard=0):
    """Outputs, each inside its own buffer with `guard` elements of a canary before and after."""
    bufs, views = [], []
    for shape, dt in specs:
        canary = -77 if dt == torch.int32 else float("nan")
        n = int(np.prod(shape))
        buf = torch.full((guard + n + guard,), canary, dtype=dt, device=DEV)
        bufs.append((buf, canary))
        views.append(buf[guard:guard + n].view(shape))
    return bufs, tuple(views)


def _specs(N, K, G, dtype):
    clip = (((N, G), torch.float32), ((N, G), torch.int32), ((N, G, 2), torch.float32))
    quant = (((K, N), torch.int32), ((N, G), torch.float32), ((N, G), torch.float32), ((N, K), dtype))
    return clip, quant


def _bands_intact(bufs, guard):
    for buf, canary in bufs:
        for band in (buf[:guard], buf[-guard:]):
            assert bool(torch.isnan(band).all()) if canary != canary else bool((band == canary).all())


@pytest.mark.parametrize("name", ["awqq_w4_g128_k384", "awqq_w3_g64", "awqq_w4_g32", "awqq_w4_g128_bf16"])
def test_guard_bands_and_a_poisoned_workspace(name):
    d = fixture(name)
    N, K, g, guard = d["N"], d["K"], d["groupsize"], 1024
    W, gm, first = clip_run(name)
    cs, qs = _specs(N, K, K // g, d["w_dtype"])
    bufs, views = _alloc(cs, guard)
    need = ops._lib.load().qllm_awq_clip_search_workspace_bytes(N, K, g)
    ws_buf = torch.full((guard + max(need, 256) + guard,), 0xFF, dtype=torch.uint8, device=DEV)      # all-ones bytes: NaN as fp32
    ops.awq_clip_search(W, gm, d["bits"], g, out=views, workspace=ws_buf[guard:guard + max(need, 256)])
    torch.cuda.synchronize()
    assert _same(first, views)
    _bands_intact(bufs, guard)
    assert bool((ws_buf[:guard] == 0xFF).all()) and bool((ws_buf[-guard:] == 0xFF).all())
    s, clip = operands(d, "scale_clip")
    want = ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip)
    bufs, views = _alloc(qs, guard)
    ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip, out=views)
    torch.cuda.synchronize()
    assert _same(want, views)
    _bands_intact(bufs, guard)


def test_capturable_in_a_graph():
    name = "awqq_w4_g128_k384"
    d = fixture(name)
    N, K, g = d["N"], d["K"], d["groupsize"]
    W, gm, first = clip_run(name)
    s, clip = operands(d, "scale_clip")
    want = ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip)
    cs, qs = _specs(N, K, K // g, d["w_dtype"])
    cviews, qviews = _alloc(cs)[1], _alloc(qs)[1]

    def both():
        ops.awq_clip_search(W, gm, d["bits"], g, out=cviews)
        ops.awq_quantize(W, d["bits"], g, col_scale=s, clip=clip, out=qviews)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        both()                                                                            # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    for v in cviews + qviews:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same(first, cviews) and _same(want, qviews)


@pytest.mark.parametrize("g", [128, 32])
def test_more_row_tiles_than_one_wave_of_blocks_and_a_ragged_row_tile(g):
    """N = 1000 (63 row tiles, the last one with 8 rows) x K = 512: every row must equal the same row run alone, whatever tile it sits
    in and whichever block walks its groups."""
    gen = torch.Generator().manual_seed(5)
    N, K = 1000, 512
    W = (0.02 * torch.randn((N, K), generator=gen)).half().to(DEV)
    X = (torch.randn((256, K), generator=gen) * torch.exp(0.5 * torch.randn(K, generator=gen))).half().to(DEV)
    from qllm_amd.quantization.awq import gram_matrices
    gm = gram_matrices(X, g)
    s = torch.exp(0.5 * torch.randn(K, generator=gen)).to(DEV)
    rows = torch.tensor([0, 15, 16, 511, 992, 999]).to(DEV)
    full = ops.awq_clip_search(W, gm, 4, g)
    part = ops.awq_clip_search(W[rows].contiguous(), gm, 4, g)
    assert all(torch.equal(a[rows], b) for a, b in zip(full, part))
    assert torch.isfinite(full[0]).all() and torch.isfinite(full[2]).all() and bool((full[2][..., 1] <= full[2][..., 0]).all())
    qf = ops.awq_quantize(W, 4, g, col_scale=s, clip=full[0])
    qp = ops.awq_quantize(W[rows].contiguous(), 4, g, col_scale=s, clip=part[0])
    assert torch.equal(qf[0][:, rows], qp[0]) and all(torch.equal(qf[i][rows], qp[i]) for i in (1, 2, 3))


# ---- the scale search -------------------------------------------------------------------------------------------------------------------
class _MLP(torch.nn.Module):
    def __init__(self, d):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = (torch.nn.Linear(w.shape[1], w.shape[0], bias=False) for w in (d["gate"], d["up"], d["down"]))
        for lin, w in ((self.gate_proj, d["gate"]), (self.up_proj, d["up"]), (self.down_proj, d["down"])):
            lin.weight.data = torch.from_numpy(w.astype(np.float32))
        self.act = torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act(self.gate_proj(x)) * self.up_proj(x))


def test_scale_search_finds_the_reference_ratios():
    from qllm_amd.quantization import search_scales
    d = dict(np.load(os.path.join(GOLD, "awqs_mlp.npz"), allow_pickle=False))
    bits, g = int(d["bits"]), int(d["groupsize"])
    mlp = _MLP(d).to(DEV)
    x = torch.from_numpy(d["x"].astype(np.float32)).to(DEV)
    with torch.no_grad():
        x_down = mlp.act(mlp.gate_proj(x)) * mlp.up_proj(x)
    before = [p.data.clone() for p in mlp.parameters()]
    for key, inspect, fcs, inp in (("mlp", mlp, [mlp.gate_proj, mlp.up_proj], x), ("down", mlp.down_proj, [mlp.down_proj], x_down)):
        s, ratio, history = search_scales(inspect, fcs, inp, {}, bits, g)
        rel = float(((s.cpu() - torch.from_numpy(d[f"s_{key}"])).abs() / torch.from_numpy(d[f"s_{key}"])).max())
        print(f"scale search {key}: ratio {ratio} (reference {float(d[f'ratio_{key}'])}), max rel diff of s {rel:.2e}, "
              f"loss {min(history):.4e} (fp64 {d[f'loss64_{key}'].min():.4e})")
        assert ratio == float(d[f"ratio_{key}"])
        assert rel <= 1e-3
        assert len(history) == N_GRID and np.isfinite(history).all() and int(np.argmin(history)) == round(ratio * N_GRID)
    assert all(torch.equal(p.data, b) for p, b in zip(mlp.parameters(), before))       # the weights are the originals again


# ---- model tier -------------------------------------------------------------------------------------------------------------------------
_models = {}
KINDS = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")


def _fp16_model():
    from test_loader_repack_cpu import _tiny_llama
    import transformers
    tiny = _tiny_llama()
    torch.set_default_dtype(torch.float16)       # built the way the loader builds one (test_hqq_quantize_gpu.py)
    try:
        model = transformers.AutoModelForCausalLM.from_config(tiny.config)
    finally:
        torch.set_default_dtype(torch.float32)
    model.load_state_dict(tiny.state_dict())
    return model.to(DEV).eval()


def quantized(auto_scale, auto_clip):
    key = (auto_scale, auto_clip)
    if key not in _models:
        from qllm_amd.quantization.awq import quantize_model
        model = _fp16_model()
        ids = torch.randint(0, 128, (2, 6), generator=torch.Generator().manual_seed(0)).to(DEV)
        with torch.no_grad():
            ref = model(ids).logits.float()
        calib = torch.randint(0, 128, (4, 32), generator=torch.Generator().manual_seed(3))
        model = quantize_model(model, calib, 4, 128, auto_scale=auto_scale, auto_clip=auto_clip, device=DEV).eval()
        with torch.no_grad():
            logits = model(ids).logits
        _models[key] = (model, ids, logits, float((logits.float() - ref).pow(2).mean()))
    return _models[key]


def test_quantize_model_tiny_llama_round_trip(tmp_path):
    from qllm_amd.modeling import base
    from qllm_amd.modeling.q_layers import WQLinear_GEMM
    from qllm_amd.utils import modelutils
    orig = _fp16_model()
    model, ids, before, mse = quantized(True, True)
    layers = modelutils.find_layers(model, [WQLinear_GEMM])
    assert len(layers) == 14 and "lm_head" not in layers
    assert not any(isinstance(m, torch.nn.Linear) for n, m in model.named_modules() if ".layers." in n)
    assert isinstance(model.lm_head, torch.nn.Linear)
    assert torch.equal(model.lm_head.weight.data, orig.lm_head.weight.data)
    assert torch.equal(model.model.embed_tokens.weight.data, orig.model.embed_tokens.weight.data)
    assert set(model.awq_report) == {"model.layers.%d.%s" % (i, n) for i in range(2) for n in KINDS} == set(layers)
    for n, r in model.awq_report.items():
        assert 0 <= r["ratio"] < 1 and len(r["history"]) == 20 and np.isfinite(r["history"]).all()
        assert int(np.argmin(r["history"])) == round(r["ratio"] * 20)
    rtn_mse = quantized(False, False)[3]
    print(f"tiny llama, logit MSE against the fp16 model: AWQ {mse:.4e}, round-to-nearest {rtn_mse:.4e}")
    assert torch.isfinite(before).all()
    d = str(tmp_path / "awq")
    base.save_quantized(model, d)
    saved = json.load(open(os.path.join(d, "quantize_config.json")))
    assert saved["version"] == "GEMM" and saved["quant_method"] == "awq"
    loaded = base.load_quantized(d, device=DEV)
    assert set(modelutils.find_layers(loaded, [WQLinear_GEMM])) == set(layers)
    with torch.no_grad():
        after = loaded(ids).logits
    assert torch.equal(before, after)


def test_without_the_searches_every_layer_is_round_to_nearest_packed():
    from qllm_amd.modeling.q_layers import WQLinear_GEMM
    from qllm_amd.utils import modelutils
    orig = _fp16_model()
    model = quantized(False, False)[0]
    layers = modelutils.find_layers(model, [WQLinear_GEMM])
    assert len(layers) == 14
    for name, layer in layers.items():
        w = modelutils.get_op_by_name(orig, name).weight.data.contiguous()
        codes, scales, zeros, _ = ops.awq_quantize(w, 4, 128, want=("codes", "scales", "zeros"))
        want = WQLinear_GEMM(4, 128, w.shape[1], w.shape[0], False, dtype=torch.float16)
        want.pack_on_device(codes, zeros.t().contiguous().to(torch.int32))
        assert torch.equal(layer.qweight.cpu(), want.qweight.cpu()) and torch.equal(layer.qzeros.cpu(), want.qzeros.cpu()), name
        assert torch.equal(layer.scales.cpu(), scales.t().contiguous().half().cpu()), name
        assert model.awq_report[name] == {"ratio": None, "history": None, "clip_err": None}


def test_clip_only_never_raises_the_output_error_and_skips_q_and_k():
    model = quantized(False, True)[0]
    for name, r in model.awq_report.items():
        assert r["ratio"] is None
        if name.endswith(("q_proj", "k_proj")):
            assert r["clip_err"] is None
        else:
            unclipped, chosen = r["clip_err"]
            print(f"clip only {name}: output error {unclipped:.4e} -> {chosen:.4e}")
            assert np.isfinite(unclipped) and 0 <= chosen <= unclipped
