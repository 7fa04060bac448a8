"""-m gpu: the GPTQ quantizer (qllm_gptq_quantize, csrc/gptq_quant.hip; qllm_amd/quantization/gptq.py) against fixtures minted from the
reference's own GPTQ.fasterquant (tests/golden/make_goldens_gptq_quant.py -> tests/golden/gptq_quant/gptqq_*.npz).

Bounds.  The trailing update of the reference is a BLAS matmul whose summation order is its own, so codes cannot be bit-equal everywhere:
the fixtures are chosen so that the reference against itself (calibration batches fed in reverse order: rounding noise through H) changes
<= 0.2 % of the codes; a wrong update order, group window or a contracted FMA moves tens of percent.  Hence: <= 1 % of the codes differ,
loss and output error <= 1.01 x the reference's (its self-variation is <= 3e-4), and the output error below the midpoint between the
reference's and round-to-nearest's.  Group 0's parameters depend on the original W only (one subtraction, one division, one rint): exact.

Measured on an MI355X (kernel tier / pipeline tier, share of differing codes): see profiles/gptq_quantize.md.  Inside the first 128
processed columns the kernel tier differs in no code, which is asserted; the pipeline tier factorises H on the device, its U differs from
the fixture's by 2e-6 of the largest entry, and w4_g128_actorder then changes 0.134 % of the first block's codes.
The summation order itself is pinned bit for bit by tests/test_gptq_walk_gpu.py."""
import glob
import json
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from qllm_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "golden", "gptq_quant", "gptqq_*.npz")))
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
_fix, _kernel, _pipe = {}, {}, {}


def fixture(name):
    if name not in _fix:
        d = dict(np.load(os.path.join(HERE, "golden", "gptq_quant", name + ".npz"), allow_pickle=False))
        for k in ("bits", "groupsize", "N", "K", "sym", "act_order", "seed"):
            d[k] = int(d[k])
        d["w_dtype"] = DTYPES[str(d["w_dtype"])]
        X = d["X"].reshape(-1, d["K"]).astype(np.float64)
        d["H64"] = 2.0 / d["X"].shape[0] * (X.T @ X)
        Wz = d["W"].astype(np.float64).copy()
        Wz[:, np.diag(d["H64"]) == 0] = 0            # dead columns: the reference zeroes them before anything else
        d["Wz"] = Wz
        _fix[name] = d
    return _fix[name]


def processing_order(d):
    """(W in processing order with dead columns zeroed, on the device in the fixture's dtype; the reference's codes / scale / zero in
    that same order)."""
    perm = d["perm"]
    W = torch.from_numpy(d["Wz"][:, perm].astype(np.float32)).to(d["w_dtype"]).to(DEV).contiguous()
    assert torch.equal(W.float().cpu(), torch.from_numpy(d["Wz"][:, perm].astype(np.float32)))     # exactly representable
    return W, d["codes"][:, perm]


def kernel_run(name):
    if name not in _kernel:
        d = fixture(name)
        W, _ = processing_order(d)
        U = torch.from_numpy(np.ascontiguousarray(d["U"])).to(DEV)
        out = ops.gptq_quantize(W, U, d["bits"], d["groupsize"], bool(d["sym"]))
        torch.cuda.synchronize()
        _kernel[name] = (W, U, out)
    return _kernel[name]


def pipeline_run(name):
    if name not in _pipe:
        from qllm_amd.quantization import accumulate_hessian, gptq_quantize_weight
        d = fixture(name)
        H, n = None, 0
        for b in range(d["X"].shape[0]):
            H, n = accumulate_hessian(H, n, torch.from_numpy(d["X"][b]).to(DEV))
        W = torch.from_numpy(d["W"]).to(d["w_dtype"]).to(DEV)
        _pipe[name] = gptq_quantize_weight(W, H, d["bits"], d["groupsize"], act_order=bool(d["act_order"]), sym=bool(d["sym"]), debug=True,
                                           pack=d["N"] % 32 == 0)
    return _pipe[name]


def out_err(d, wq_orig_order):
    D = d["Wz"] - wq_orig_order.astype(np.float64)
    return float(np.einsum("nk,kj,nj->", D, d["H64"], D))


def check_quality(d, name, tier, codes_nk, loss, wq_orig_order):
    """codes_nk / wq in the ORIGINAL column order."""
    diff = codes_nk != d["codes"]
    first = diff[:, d["perm"][:128]]
    e = out_err(d, wq_orig_order)
    print(f"{tier} {name}: codes differ {diff.mean():.4%} (first 128 columns {first.mean():.4%}); loss {loss:.6e} vs {d['error']:.6e} "
          f"(x{loss / d['error']:.5f}); out err {e:.6e} vs gptq {d['gptq_out_err']:.6e} (x{e / d['gptq_out_err']:.5f}) rtn {d['rtn_out_err']:.6e}")
    assert diff.mean() <= 0.01
    if tier == "kernel":      # the reference's own U: the first block has no summation order of a matmul behind it
        assert not first.any()
    assert loss <= 1.01 * d["error"]
    assert e <= 1.01 * d["gptq_out_err"]
    assert e < 0.5 * (d["gptq_out_err"] + d["rtn_out_err"])


# ---- kernel tier ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_reference_walk(name):
    d = fixture(name)
    g, K, N, perm = d["groupsize"], d["K"], d["N"], d["perm"]
    W, U, (codes, scale, zero, wq, loss) = kernel_run(name)
    scale_c, zero_c = scale.cpu().numpy(), zero.cpu().numpy()
    # group 0 of the walk: from the original W alone
    assert np.array_equal(scale_c[:, 0], d["scale"][:, 0]) and np.array_equal(zero_c[:, 0], d["zero"][:, 0])
    assert np.isfinite(scale_c).all() and np.array_equal(zero_c, np.rint(zero_c))
    codes_p = codes.cpu().numpy().T                                   # [N, K], processing order
    assert codes_p.min() >= 0 and codes_p.max() <= 2 ** d["bits"] - 1
    # wq == scale * (code - zero), exactly, in W's dtype
    want = (scale.repeat_interleave(g, 1) * (codes.t().float() - zero.repeat_interleave(g, 1))).to(d["w_dtype"])
    assert torch.equal(wq, want)
    inv = np.argsort(perm)
    check_quality(d, name, "kernel", codes_p[:, inv], float(loss.sum().item()), wq.float().cpu().numpy()[:, inv])


@pytest.mark.parametrize("name", NAMES)
def test_identity_factor_is_round_to_nearest(name):
    d = fixture(name)
    g, K, N, maxq = d["groupsize"], d["K"], d["N"], 2 ** d["bits"] - 1
    W, _ = processing_order(d)
    codes, scale, zero, wq, loss = ops.gptq_quantize(W, None, d["bits"], g, bool(d["sym"]))
    Wn = W.float().cpu().numpy().reshape(N, K // g, g)
    mn, mx = np.minimum(Wn.min(2), 0), np.maximum(Wn.max(2), 0)
    if d["sym"]:
        mx = np.maximum(np.abs(mn), mx)
        mn = np.where(mn < 0, -mx, mn)
    flat = (mn == 0) & (mx == 0)
    mn, mx = np.where(flat, np.float32(-1), mn), np.where(flat, np.float32(1), mx)
    s = ((mx - mn) / np.float32(maxq)).astype(np.float32)
    z = np.full_like(s, (maxq + 1) / 2) if d["sym"] else np.rint(-mn / s).astype(np.float32)
    q = np.clip(np.rint(Wn / s[:, :, None]) + z[:, :, None], 0, maxq)
    assert np.array_equal(scale.cpu().numpy(), s) and np.array_equal(zero.cpu().numpy(), z)
    assert np.array_equal(codes.cpu().numpy().T, q.reshape(N, K).astype(np.int32))
    dq = s[:, :, None] * (q - z[:, :, None])
    assert np.array_equal(wq.float().cpu().numpy(), torch.from_numpy(dq.reshape(N, K)).to(d["w_dtype"]).float().numpy())
    np.testing.assert_allclose(loss.cpu().numpy(), ((Wn - dq).astype(np.float64) ** 2).sum((1, 2)) / 2, rtol=1e-5)


@pytest.mark.parametrize("name", ["gptqq_w4_g128_actorder", "gptqq_w4_g64_k320_dead", "gptqq_w4_g32_actorder"])
def test_repeatable_and_independent_of_the_storage_dtype(name):
    d = fixture(name)
    W, U, first = kernel_run(name)
    again = ops.gptq_quantize(W, U, d["bits"], d["groupsize"], bool(d["sym"]))
    wide = ops.gptq_quantize(W.float(), U, d["bits"], d["groupsize"], bool(d["sym"]))
    for i, (a, b, c) in enumerate(zip(first, again, wide)):
        assert torch.equal(a, b), i
        if i != 3:
            assert torch.equal(a, c), i
    assert torch.equal(wide[3].to(d["w_dtype"]), first[3])    # wq: the fp32 run's values are the 16-bit run's before their rounding


def _alloc(N, K, G, dtype, guard=0, fill=None):
    """The five outputs, each inside its own buffer with `guard` elements of a canary before and after."""
    bufs, views = [], []
    for shape, dt, canary in (((K, N), torch.int32, -77), ((N, G), torch.float32, float("nan")), ((N, G), torch.float32, float("nan")),
                              ((N, K), dtype, float("nan")), ((N,), torch.float32, float("nan"))):
        n = int(np.prod(shape))
        buf = torch.full((guard + n + guard,), canary, dtype=dt, device=DEV)
        bufs.append((buf, canary))
        views.append(buf[guard:guard + n].view(shape))
    return bufs, tuple(views)


@pytest.mark.parametrize("name", ["gptqq_w4_g128_actorder", "gptqq_w4_g64_k320_dead", "gptqq_w4_g32_actorder", "gptqq_w4_gK"])
def test_guard_bands_and_a_poisoned_workspace(name):
    d = fixture(name)
    N, K, g = d["N"], d["K"], d["groupsize"]
    W, U, first = kernel_run(name)
    guard = 1024
    bufs, views = _alloc(N, K, K // g, d["w_dtype"], guard)
    need = ops._lib.load().qllm_gptq_quantize_workspace_bytes(N, K)
    ws_buf = torch.full((guard + need + guard,), 0xFF, dtype=torch.uint8, device=DEV)      # all-ones bytes: NaN as fp32
    ops.gptq_quantize(W, U, d["bits"], g, bool(d["sym"]), out=views, workspace=ws_buf[guard:guard + need])
    torch.cuda.synchronize()
    for a, b in zip(first, views):
        assert torch.equal(a, b)
    for buf, canary in bufs:
        for band in (buf[:guard], buf[-guard:]):
            assert bool(torch.isnan(band).all()) if canary != canary else bool((band == canary).all())
    assert bool((ws_buf[:guard] == 0xFF).all()) and bool((ws_buf[-guard:] == 0xFF).all())


def test_capturable_in_a_graph():
    name = "gptqq_w4_g128_actorder"
    d = fixture(name)
    N, K, g = d["N"], d["K"], d["groupsize"]
    W, U, first = kernel_run(name)
    _, views = _alloc(N, K, K // g, d["w_dtype"])
    need = ops._lib.load().qllm_gptq_quantize_workspace_bytes(N, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gptq_quantize(W, U, d["bits"], g, False, out=views, workspace=ws)             # warm-up
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for v in views:
        v.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.gptq_quantize(W, U, d["bits"], g, False, out=views, workspace=ws)
    for v in views:
        v.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, views):
        assert torch.equal(a, b)


def test_more_rows_than_one_wave_of_blocks_and_a_ragged_row_tile():
    """N = 1000 (63 row tiles, the last one with 8 rows) x K = 512 (four column blocks): every row must equal the same row quantized
    alone, whatever tile it sits in (rows are independent), with a genuine dense upper factor."""
    gen = torch.Generator().manual_seed(5)
    N, K = 1000, 512
    W = (0.02 * torch.randn((N, K), generator=gen)).half().to(DEV)
    X = torch.randn((2048, K), generator=gen) * torch.exp(0.5 * torch.randn(K, generator=gen))
    H = (2.0 / 2048 * X.T @ X).double()
    H += 0.01 * H.diag().mean() * torch.eye(K, dtype=torch.float64)
    U = torch.linalg.cholesky(torch.cholesky_inverse(torch.linalg.cholesky(H)), upper=True).float().to(DEV).contiguous()
    full = ops.gptq_quantize(W, U, 4, 64, False)
    rows = torch.tensor([0, 15, 16, 511, 992, 999])
    part = ops.gptq_quantize(W[rows.to(DEV)].contiguous(), U, 4, 64, False)
    assert torch.equal(full[0][:, rows.to(DEV)], part[0])
    for i in (1, 2, 3, 4):
        assert torch.equal(full[i][rows.to(DEV)], part[i])
    assert torch.isfinite(full[4]).all() and torch.isfinite(full[3]).all()


# ---- pipeline tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pipeline_from_activations_to_packed_layer(name):
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    d = fixture(name)
    N, K, g, bits = d["N"], d["K"], d["groupsize"], d["bits"]
    qweight, qzeros, scales, g_idx, loss, ex = pipeline_run(name)
    assert ex["factorization"] == "device"        # no host fallback on the project's own target
    assert np.array_equal(ex["perm"].cpu().numpy(), d["perm"])
    du = float((ex["U"].cpu() - torch.from_numpy(d["U"])).abs().max()) / float(np.abs(d["U"]).max())
    print(f"pipeline {name}: max |U - U_ref| / max |U_ref| = {du:.3e}")
    assert du <= 1e-3
    assert np.array_equal(g_idx.cpu().numpy(), d["g_idx"])
    codes = ex["codes"].cpu().numpy()
    check_quality(d, name, "pipeline", codes, float(loss.item()), ex["wq"].float().cpu().numpy())
    if N % 32:
        # QuantLinearGPTQ packs its zero points in whole 32-column words: this layer has no packed form, and the packer says so
        from qllm_amd.quantization.gptq import _pack
        assert qweight is None
        with pytest.raises(ValueError, match="32"):
            _pack(ex["codes"].t().contiguous().int(), ex["zero"].t().contiguous(), bits, g)
        return
    # the packed layer, in the original column order
    act = bool(d["act_order"])
    w = ops.make_weight("GPTQ", qweight, scales.half(), qzeros, g_idx if act else None, None, K, N, g, bits)[0]
    deq = ops.dequant(w, torch.device(DEV), torch.float16, transposed=True).float().cpu().numpy()      # [N, K]
    gi = d["g_idx"].astype(np.int64)
    s16 = scales.half().float().cpu().numpy().T[:, gi]
    z = ex["zero"].cpu().numpy()[:, gi]
    exact = s16.astype(np.float64) * (codes.astype(np.float64) - z)
    # fp16 q*s - z*s: two roundings of magnitudes <= maxq * s (half an ulp = 2^-11 relative each), one of the difference
    bound = 3 * 2.0 ** -11 * (2 ** bits - 1) * s16
    assert (np.abs(deq - exact) <= bound).all()
    assert np.array_equal(deq, O.dequant("GPTQ", qweight.cpu().numpy(), scales.half().cpu().numpy(), qzeros.cpu().numpy(),
                                         d["g_idx"] if act else None, bits, g, K, 0).T.astype(np.float32))
    layer = QuantLinearGPTQ(bits, g, K, N, False, dtype=torch.float16)
    layer.qweight, layer.qzeros, layer.scales, layer.g_idx = qweight, qzeros, scales.half(), g_idx
    layer = layer.to(DEV)
    x = (torch.randn((3, K), generator=torch.Generator().manual_seed(1))).half()
    y = layer(x.to(DEV)).float().cpu().numpy()
    y16 = O.matmul_f16(x.numpy(), deq.T.astype(np.float16), None).numpy()
    y64 = x.double().numpy() @ deq.T.astype(np.float64)
    assert O.rel_err(y, y16) <= 1e-2 and O.rel_err(y, y64) <= 2e-3


# ---- model tier -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act_order", [False, True])
def test_quantize_model_tiny_llama(tmp_path, act_order):
    from test_loader_repack_cpu import _tiny_llama
    from qllm_amd.modeling import base
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    from qllm_amd.quantization.gptq import quantize_model
    from qllm_amd.utils import modelutils
    import transformers
    tiny = _tiny_llama()
    torch.set_default_dtype(torch.float16)       # built the way the loader builds one (test_hqq_quantize_gpu.py)
    try:
        model = transformers.AutoModelForCausalLM.from_config(tiny.config)
    finally:
        torch.set_default_dtype(torch.float32)
    model.load_state_dict(tiny.state_dict())
    head, embed = model.lm_head.weight.data.clone(), model.model.embed_tokens.weight.data.clone()
    calib = torch.randint(0, 128, (4, 32), generator=torch.Generator().manual_seed(3))
    model = quantize_model(model, calib, 4, 128, act_order=act_order, device=DEV, debug=True).eval()
    layers = modelutils.find_layers(model, [QuantLinearGPTQ])
    assert len(layers) == 14 and "lm_head" not in layers
    assert not any(isinstance(m, torch.nn.Linear) for n, m in model.named_modules() if ".layers." in n)
    assert isinstance(model.lm_head, torch.nn.Linear)
    assert torch.equal(model.lm_head.weight.data.cpu(), head) and torch.equal(model.model.embed_tokens.weight.data.cpu(), embed)
    assert set(model.gptq_losses) == {"model.layers.%d.%s" % (i, n) for i in range(2) for n in
                                      ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj",
                                       "mlp.up_proj", "mlp.down_proj")}
    for n, loss in model.gptq_losses.items():
        print(f"act_order={act_order} {n}: loss {loss:.5e}  1/2 tr(D Hd D^T) {model.gptq_losses_hd[n]:.5e}  round-to-nearest "
              f"{model.gptq_rtn_losses[n]:.5e}")
        assert np.isfinite(loss) and loss < model.gptq_rtn_losses[n]
        assert model.gptq_losses_hd[n] < model.gptq_rtn_losses[n]
    assert all(bool(l._resolve_act_order()) == act_order for l in layers.values())
    ids = torch.randint(0, 128, (2, 6), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        before = model(ids).logits
    assert torch.isfinite(before).all()
    d = str(tmp_path / "gptq")
    base.save_quantized(model, d)
    saved = json.load(open(os.path.join(d, "quantize_config.json")))
    assert saved["version"] == "GPTQ" and bool(saved.get("desc_act", False)) == act_order
    loaded = base.load_quantized(d, device=DEV)
    assert loaded.quant_config.desc_act == act_order
    assert set(modelutils.find_layers(loaded, [QuantLinearGPTQ])) == set(layers)
    with torch.no_grad():
        after = loaded(ids).logits
    assert torch.equal(before, after)


def test_quantize_model_mixed_widths_by_kind_and_by_name(tmp_path):
    """bits_by_layer: a module kind ("down_proj": both blocks) and one full module name; the widths reach the layers, quant_config.by_layer
    and, through save_quantized -> load_quantized, the reloaded model, whose logits are the same bits.  Without debug: no layer carries
    the round-to-nearest comparison."""
    from test_loader_repack_cpu import _tiny_llama
    from qllm_amd.modeling import base
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    from qllm_amd.quantization.gptq import quantize_model
    from qllm_amd.utils import modelutils
    import transformers
    tiny = _tiny_llama()
    torch.set_default_dtype(torch.float16)
    try:
        model = transformers.AutoModelForCausalLM.from_config(tiny.config)
    finally:
        torch.set_default_dtype(torch.float32)
    model.load_state_dict(tiny.state_dict())
    calib = torch.randint(0, 128, (4, 32), generator=torch.Generator().manual_seed(3))
    mixed = {"down_proj": 8, "model.layers.1.self_attn.q_proj": 3}
    model = quantize_model(model, calib, 4, 128, bits_by_layer=mixed, device=DEV).eval()
    layers = modelutils.find_layers(model, [QuantLinearGPTQ])
    want = {n: 8 if n.endswith("down_proj") else 3 if n == "model.layers.1.self_attn.q_proj" else 4 for n in layers}
    assert len(layers) == 14 and sorted(want.values()).count(8) == 2 and sorted(want.values()).count(3) == 1
    for n, l in layers.items():
        assert l.bits == want[n] and l.qweight.shape[0] == l.infeatures // 32 * want[n], n
        assert model.quant_config.by_layer[n]["wbits"] == want[n]
        assert np.isfinite(model.gptq_losses[n]) and not hasattr(l, "gptq_rtn_loss")
    assert not hasattr(model, "gptq_rtn_losses")
    ids = torch.randint(0, 128, (2, 6), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        before = model(ids).logits
    assert torch.isfinite(before).all()
    d = str(tmp_path / "gptq_mixed")
    base.save_quantized(model, d)
    loaded = base.load_quantized(d, device=DEV)
    got = modelutils.find_layers(loaded, [QuantLinearGPTQ])
    assert {n: l.bits for n, l in got.items()} == want
    with torch.no_grad():
        after = loaded(ids).logits
    assert torch.equal(before, after)
