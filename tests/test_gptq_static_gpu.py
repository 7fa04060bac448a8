"""-m gpu: the GPTQ quantizer with static groups (qllm_gptq_quantize_static, csrc/gptq_static.hip; gptq_quantize_weight / quantize_linear /
quantize_model with static_groups=True) against fixtures minted from the reference's own GPTQ.fasterquant(static_groups=True)
(tests/golden/make_goldens_gptq_static.py -> tests/golden/gptq_static/gptqs_*.npz).

Bounds.  Every group's scale / zero depends on the original W alone (a minimum, a maximum, one subtraction, one division, one rint):
bit-equal to the reference for every group.  The walk's bounds are the dynamic tests' (test_gptq_quantize_gpu.py) for the same reason:
the reference's trailing update is a BLAS matmul with a summation order of its own, and the fixtures are chosen so that the reference
against itself (batches fed in reverse) changes <= 0.2 % of the codes, while a wrong order, a wrong group or a contracted FMA moves tens
of percent (the reference's own dynamic-groups run differs in 17-78 %).  Hence <= 1 % of the codes differ, loss and output error <= 1.01 x
the reference's, and the output error below the midpoint between the reference's and round-to-nearest's.  The cross-checks against
qllm_gptq_quantize (u = None, group_size == K) need no tolerance: the same arithmetic gives the same bits.

Measured shares: profiles/gptq_quantize.md."""
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
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "golden", "gptq_static", "gptqs_*.npz")))
DTYPES = {"float16": torch.float16, "bfloat16": torch.bfloat16}
_fix, _kernel, _pipe = {}, {}, {}


def test_all_six_fixtures_are_present():
    assert NAMES == sorted(["gptqs_w4_g128_actorder", "gptqs_w4_g128", "gptqs_w4_g32_actorder_n48", "gptqs_w3_g64_actorder_sym",
                            "gptqs_w4_g64_k320_dead_actorder", "gptqs_w4_g128_actorder_bf16"])


def fixture(name, sub="gptq_static"):
    if name not in _fix:
        d = dict(np.load(os.path.join(HERE, "golden", sub, name + ".npz"), allow_pickle=False))
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


def device_inputs(d):
    """(W in the ORIGINAL column order with dead columns zeroed, in the fixture's dtype; U in processing order; perm or None)."""
    W = torch.from_numpy(d["Wz"].astype(np.float32)).to(d["w_dtype"]).to(DEV).contiguous()
    assert torch.equal(W.float().cpu(), torch.from_numpy(d["Wz"].astype(np.float32)))     # exactly representable
    U = torch.from_numpy(np.ascontiguousarray(d["U"])).to(DEV)
    perm = torch.from_numpy(d["perm"]).to(DEV) if d["act_order"] else None
    return W, U, perm


def kernel_run(name):
    if name not in _kernel:
        d = fixture(name)
        W, U, perm = device_inputs(d)
        out = ops.gptq_quantize_static(W, U, perm, d["bits"], d["groupsize"], bool(d["sym"]))
        torch.cuda.synchronize()
        _kernel[name] = (W, U, perm, out)
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
                                           pack=d["N"] % 32 == 0, static_groups=True)
    return _pipe[name]


def check_quality(d, name, tier, codes_nk, loss, wq):
    """codes_nk / wq in the original column order."""
    diff = codes_nk != d["codes"]
    first = diff[:, d["perm"][:128]]                  # the first 128 processed columns
    D = d["Wz"] - wq.astype(np.float64)
    e = float(np.einsum("nk,kj,nj->", D, d["H64"], D))
    print(f"{tier} {name}: codes differ {diff.mean():.4%} (first 128 columns {first.mean():.4%}); loss {loss:.6e} vs {d['error']:.6e} "
          f"(x{loss / d['error']:.5f}); out err {e:.6e} vs gptq {d['gptq_out_err']:.6e} (x{e / d['gptq_out_err']:.5f}) rtn {d['rtn_out_err']:.6e}")
    assert diff.mean() <= 0.01
    if tier == "kernel":      # the reference's own U: the first block has no summation order of a matmul behind it
        assert not first.any()
    assert loss <= 1.01 * d["error"]
    assert e <= 1.01 * d["gptq_out_err"]
    assert e < 0.5 * (d["gptq_out_err"] + d["rtn_out_err"])


def same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


# ---- kernel tier ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_kernel_matches_the_reference_walk(name):
    d = fixture(name)
    g, K, N = d["groupsize"], d["K"], d["N"]
    assert np.array_equal(d["g_idx"], np.arange(K) // g) and int(d["static_groups"]) == 1
    W, U, perm, (codes, scale, zero, wq, loss) = kernel_run(name)
    # every group's parameters: from the original W alone
    assert np.array_equal(scale.cpu().numpy(), d["scale"]) and np.array_equal(zero.cpu().numpy(), d["zero"])
    codes_nk = codes.cpu().numpy().T                                   # [N, K], already in the original order
    assert codes_nk.min() >= 0 and codes_nk.max() <= 2 ** d["bits"] - 1
    # wq == scale * (code - zero), exactly, in W's dtype, with the trivial group of every original column
    want = (scale.repeat_interleave(g, 1) * (codes.t().float() - zero.repeat_interleave(g, 1))).to(d["w_dtype"])
    assert torch.equal(wq, want)
    check_quality(d, name, "kernel", codes_nk, float(loss.sum().item()), wq.float().cpu().numpy())


@pytest.mark.parametrize("name", NAMES)
def test_identity_factor_equals_the_dynamic_entry_point_with_and_without_perm(name):
    d = fixture(name)
    W, _, _ = device_inputs(d)
    perm = torch.from_numpy(d["perm"]).to(DEV)
    dyn = ops.gptq_quantize(W, None, d["bits"], d["groupsize"], bool(d["sym"]))
    assert same(dyn, ops.gptq_quantize_static(W, None, None, d["bits"], d["groupsize"], bool(d["sym"])))
    assert same(dyn, ops.gptq_quantize_static(W, None, perm, d["bits"], d["groupsize"], bool(d["sym"])))
    assert same(dyn, ops.gptq_quantize_static(W, None, perm.int(), d["bits"], d["groupsize"], bool(d["sym"])))


def test_one_group_per_row_equals_the_dynamic_entry_point():
    """group_size == K: the parameters come from the original row either way.  Without a permutation both entry points see the same
    problem; with one, the dynamic entry point gets the permuted W and its outputs are un-permuted here."""
    d = fixture("gptqq_w4_gK", "gptq_quant")
    K = d["K"]
    assert d["groupsize"] == K and not d["act_order"]
    W, U, _ = device_inputs(d)
    dyn = ops.gptq_quantize(W, U, d["bits"], K, False)
    assert same(dyn, ops.gptq_quantize_static(W, U, None, d["bits"], K, False))
    assert same(dyn, ops.gptq_quantize_static(W, U, torch.arange(K, device=DEV), d["bits"], K, False))
    assert same(dyn, ops.gptq_quantize_static(W, U, None, d["bits"], -1, False))
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(7)).to(DEV)     # (any upper factor serves any order of the walk)
    codes, scale, zero, wq, loss = ops.gptq_quantize(W[:, perm].contiguous(), U, d["bits"], K, False)
    inv = torch.argsort(perm)
    got = ops.gptq_quantize_static(W, U, perm, d["bits"], K, False)
    assert same((codes[inv].contiguous(), scale, zero, wq[:, inv].contiguous(), loss), got)
    assert not torch.equal(got[0], dyn[0])                                           # the order of the walk matters


@pytest.mark.parametrize("name", ["gptqs_w4_g128_actorder", "gptqs_w4_g64_k320_dead_actorder", "gptqs_w4_g32_actorder_n48"])
def test_repeatable_and_independent_of_the_storage_dtype(name):
    d = fixture(name)
    W, U, perm, first = kernel_run(name)
    again = ops.gptq_quantize_static(W, U, perm, d["bits"], d["groupsize"], bool(d["sym"]))
    wide = ops.gptq_quantize_static(W.float(), U, perm, d["bits"], d["groupsize"], bool(d["sym"]))
    for i, (a, b, c) in enumerate(zip(first, again, wide)):
        assert torch.equal(a, b), i
        if i != 3:
            assert torch.equal(a, c), i
    assert torch.equal(wide[3].to(d["w_dtype"]), first[3])    # wq: the fp32 run's values are the 16-bit run's before their rounding


@pytest.mark.parametrize("name", ["gptqs_w4_g64_k320_dead_actorder", "gptqs_w4_g32_actorder_n48"])
def test_guard_bands_and_a_poisoned_workspace(name):
    """The stores are scattered by perm: every output sits between canaries, the workspace starts as NaNs."""
    d = fixture(name)
    N, K, g = d["N"], d["K"], d["groupsize"]
    W, U, perm, first = kernel_run(name)
    guard, bufs, views = 1024, [], []
    for shape, dt, canary in (((K, N), torch.int32, -77), ((N, K // g), torch.float32, float("nan")), ((N, K // g), torch.float32, float("nan")),
                              ((N, K), d["w_dtype"], float("nan")), ((N,), torch.float32, float("nan"))):
        n = int(np.prod(shape))
        buf = torch.full((guard + n + guard,), canary, dtype=dt, device=DEV)
        bufs.append((buf, canary))
        views.append(buf[guard:guard + n].view(shape))
    need = ops._lib.load().qllm_gptq_quantize_workspace_bytes(N, K)
    ws_buf = torch.full((guard + need + guard,), 0xFF, dtype=torch.uint8, device=DEV)      # all-ones bytes: NaN as fp32
    ops.gptq_quantize_static(W, U, perm, d["bits"], g, bool(d["sym"]), out=tuple(views), workspace=ws_buf[guard:guard + need])
    torch.cuda.synchronize()
    assert same(first, views)
    for buf, canary in bufs:
        for band in (buf[:guard], buf[-guard:]):
            assert bool(torch.isnan(band).all()) if canary != canary else bool((band == canary).all())
    assert bool((ws_buf[:guard] == 0xFF).all()) and bool((ws_buf[-guard:] == 0xFF).all())


def test_perm_must_be_a_permutation():
    d = fixture("gptqs_w4_g128")
    W, U, _ = device_inputs(d)
    K = d["K"]
    twice = torch.arange(K, device=DEV)
    twice[5] = 6
    outside = torch.arange(K, device=DEV)
    outside[0] = K
    negative = torch.arange(K, device=DEV)
    negative[3] = -1
    for bad in (twice, outside, negative):
        with pytest.raises(ValueError, match="permutation"):
            ops.gptq_quantize_static(W, U, bad, d["bits"], d["groupsize"], False)
    with pytest.raises(RuntimeError, match="perm must be"):
        ops.gptq_quantize_static(W, U, torch.arange(K - 1, device=DEV), d["bits"], d["groupsize"], False)


# ---- pipeline tier ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_pipeline_from_activations_to_packed_layer(name):
    d = fixture(name)
    N, K, g, bits = d["N"], d["K"], d["groupsize"], d["bits"]
    qweight, qzeros, scales, g_idx, loss, ex = pipeline_run(name)
    assert ex["factorization"] == "device"        # no host fallback on the project's own target
    assert np.array_equal(ex["perm"].cpu().numpy(), d["perm"])
    assert np.array_equal(g_idx.cpu().numpy(), np.arange(K) // g) and g_idx.dtype == torch.int32
    assert np.array_equal(ex["scale"].cpu().numpy(), d["scale"]) and np.array_equal(ex["zero"].cpu().numpy(), d["zero"])
    codes = ex["codes"].cpu().numpy()
    check_quality(d, name, "pipeline", codes, float(loss.item()), ex["wq"].float().cpu().numpy())
    assert float(ex["loss_hd"]) < float(ex["rtn_loss"])
    if N % 32:
        assert qweight is None      # QuantLinearGPTQ packs its zero points in whole 32-column words (test_gptq_quantize_gpu.py)
        return
    assert np.array_equal(O.unpack_along_rows(qweight.cpu().numpy(), bits, K), codes.T.astype(np.int32))
    assert np.array_equal(O.unpack_along_cols(qzeros.cpu().numpy(), bits, N), ex["zero"].cpu().numpy().T.astype(np.int32))
    assert np.array_equal(scales.float().cpu().numpy(), ex["scale"].t().to(scales.dtype).float().cpu().numpy())


# ---- layer tier -------------------------------------------------------------------------------------------------------------------------
def test_an_act_order_layer_with_static_groups_decodes_on_the_plain_route():
    from qllm_amd.quantization import accumulate_hessian
    from qllm_amd.quantization.gptq import quantize_linear
    d = fixture("gptqs_w4_g128_actorder")
    N, K, g, bits = d["N"], d["K"], d["groupsize"], d["bits"]
    H, n = None, 0
    for b in range(d["X"].shape[0]):
        H, n = accumulate_hessian(H, n, torch.from_numpy(d["X"][b]).to(DEV))

    def quantized(**kw):
        lin = torch.nn.Linear(K, N, bias=False).half()
        lin.weight.data = torch.from_numpy(d["W"]).half()
        return quantize_linear(lin, H, bits, g, device=DEV, **kw)

    layer, plain, scrambled = quantized(act_order=True, static_groups=True), quantized(act_order=False), quantized(act_order=True)
    assert layer._resolve_act_order() is False and plain._resolve_act_order() is False and scrambled._resolve_act_order() is True
    assert torch.equal(layer.g_idx.cpu(), (torch.arange(K) // g).int())
    assert not torch.equal(layer.qweight, plain.qweight)             # another walk, other codes ...
    for m in (1, 16):                                                # ... the same plan
        got, want = ops.plan_describe([layer.decode_descriptor()], m), ops.plan_describe([plain.decode_descriptor()], m)
        print(f"M={m}: static + act-order: {got} | plain: {want}")
        assert got == want
    assert ops.plan_describe([layer.decode_descriptor()], 1).startswith("strip1 ")
    w = ops.make_weight("GPTQ", layer.qweight, layer.scales, layer.qzeros, None, None, K, N, g, bits)[0]
    own = ops.dequant(w, torch.device(DEV), torch.float16, transposed=True).double().cpu().numpy()      # the layer's own W, [N, K]
    for m in (1, 16):
        x = torch.randn((m, K), generator=torch.Generator().manual_seed(m)).half()
        y = layer(x.to(DEV)).float().cpu().numpy()
        err = O.rel_err(y, x.double().numpy() @ own.T)
        print(f"M={m}: rel err {err:.3e}")
        assert err <= 2e-3


# ---- model tier -------------------------------------------------------------------------------------------------------------------------
def test_quantize_model_tiny_llama_act_order_with_static_groups(tmp_path):
    from test_loader_repack_cpu import _tiny_llama
    from qllm_amd.modeling import base
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ
    from qllm_amd.quantization.gptq import quantize_model
    from qllm_amd.utils import modelutils
    import transformers
    tiny = _tiny_llama()
    torch.set_default_dtype(torch.float16)       # built the way the loader builds one (test_gptq_quantize_gpu.py)
    try:
        model = transformers.AutoModelForCausalLM.from_config(tiny.config)
    finally:
        torch.set_default_dtype(torch.float32)
    model.load_state_dict(tiny.state_dict())
    calib = torch.randint(0, 128, (4, 32), generator=torch.Generator().manual_seed(3))
    model = quantize_model(model, calib, 4, 128, act_order=True, static_groups=True, device=DEV, debug=True).eval()
    layers = modelutils.find_layers(model, [QuantLinearGPTQ])
    assert len(layers) == 14 and set(model.gptq_losses) == {"model.layers.%d.%s" % (i, n) for i in range(2) for n in
                                                            ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj",
                                                             "mlp.gate_proj", "mlp.up_proj", "mlp.down_proj")}
    for n, l in layers.items():
        assert torch.equal(l.g_idx.cpu(), (torch.arange(l.infeatures) // l.groupsize).int()), n
        assert l._resolve_act_order() is False, n
    for n, loss in model.gptq_losses.items():
        print(f"{n}: loss {loss:.5e}  1/2 tr(D Hd D^T) {model.gptq_losses_hd[n]:.5e}  round-to-nearest {model.gptq_rtn_losses[n]:.5e}")
        assert np.isfinite(loss) and loss < model.gptq_rtn_losses[n]
        assert model.gptq_losses_hd[n] < model.gptq_rtn_losses[n]
    ids = torch.randint(0, 128, (2, 6), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        before = model(ids).logits
    assert torch.isfinite(before).all()
    d = str(tmp_path / "gptq_static")
    base.save_quantized(model, d)
    saved = json.load(open(os.path.join(d, "quantize_config.json")))
    assert saved["version"] == "GPTQ" and saved["static_groups"] is True and saved["desc_act"] is True
    loaded = base.load_quantized(d, device=DEV)
    assert loaded.quant_config.static_groups and loaded.quant_config.desc_act
    got = modelutils.find_layers(loaded, [QuantLinearGPTQ])
    assert set(got) == set(layers) and not any(l._resolve_act_order() for l in got.values())
    with torch.no_grad():
        after = loaded(ids).logits
    assert torch.equal(before, after)
