"""-m gpu: the HQQ quantizer (qllm_hqq_quantize, csrc/hqq_quant.hip; qllm_amd/quantization/hqq.py) against the reference's own runs
(tests/golden/hqq_quant/hqqq_*.npz, minted by tests/golden/make_goldens_hqq_quant.py from the fp32 CPU path of the reference's solver).

Each fixture is quantized ONCE (module cache) with the debug output on -- the solver's own fp32 s and z -- and every property below reads
that one result.  Bounds: scales and the number of rounds exact; zero points within 1e-3 of the reference's in >= 98 % of the groups
(the reference against itself on reversed groups: <= 3.1e-5, see the fixtures' zero_rev); inside agreeing groups <= 0.5 % of the codes
differ, by one; mean |W - dequant| <= 1.002 x the reference's and closer to it than to round-to-nearest's."""
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
NAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(HERE, "golden", "hqq_quant", "hqqq_*.npz")))
_CACHE = {}


def test_fixtures_are_present():
    assert len(NAMES) == 7 and {"hqqq_w2_g64", "hqqq_w3_g64", "hqqq_w4_g64", "hqqq_w8_g64"} <= set(NAMES)


def _w_tensor(g, dtype=None):
    return torch.from_numpy(g["W"]).to(dtype or getattr(torch, str(g["w_dtype"]))).to(DEV)


def case(name):
    """(fixture, result) -- result: numpy arrays of one debug run, [N, G] / [N, K] like the fixture."""
    if name not in _CACHE:
        g = dict(np.load(os.path.join(HERE, "golden", "hqq_quant", name + ".npz"), allow_pickle=False))
        for k in ("bits", "groupsize", "N", "K", "rounds_run"):
            g[k] = int(g[k])
        qweight, scales, zeros, rounds, s, z, errs = ops.hqq_quantize(_w_tensor(g), g["bits"], g["groupsize"], debug=True)
        codes = ops.unpack_qweight(qweight, "HQQ", g["bits"], g["K"], g["N"])
        r = dict(qweight=qweight, scales=scales.cpu().numpy().T, zeros=zeros.cpu().numpy().T, rounds=int(rounds.item()),
                 s=s.cpu().numpy().T.copy(), z=z.cpu().numpy().T.copy(), errs=errs.cpu().numpy(), codes=codes.cpu().numpy().T.copy())
        # the codes the kernel's own fp32 s and z imply: clamp(rint(W s + z)), one rounding per operation
        gs = g["groupsize"]
        se, ze = np.repeat(r["s"], gs, 1), np.repeat(r["z"], gs, 1)
        r["host_codes"] = np.clip(np.rint(g["W"] * se + ze), 0, 2 ** g["bits"] - 1).astype(np.int32)
        r["wdq"] = (r["codes"].astype(np.float32) - ze) / se
        r["agree"] = np.abs(r["z"] - g["zero"]) <= 1e-3
        _CACHE[name] = (g, r)
    return _CACHE[name]


@pytest.mark.parametrize("name", NAMES)
def test_scales_are_bit_exact(name):
    g, r = case(name)
    assert np.array_equal(r["s"].view(np.uint32), g["s_inv"].view(np.uint32))                       # one IEEE division
    want = (np.float32(1.0) / g["s_inv"]).astype(np.float16)
    assert np.array_equal(r["scales"].view(np.uint16), want.view(np.uint16))
    assert np.array_equal(r["zeros"].view(np.uint16), r["z"].astype(np.float16).view(np.uint16))    # stored zero = fp16(final fp32 z)


@pytest.mark.parametrize("name", NAMES)
def test_rounds_run_matches_the_reference(name):
    g, r = case(name)
    print(name, "rounds", r["rounds"], "reference", g["rounds_run"], "per-round mean error (gpu / reference - 1):",
          (r["errs"][:g["rounds_run"]] / g["round_err"] - 1))
    assert r["rounds"] == g["rounds_run"]


@pytest.mark.parametrize("name", NAMES)
def test_zero_points_match_the_reference(name):
    g, r = case(name)
    dz = np.abs(r["z"] - g["zero"])
    print(name, "max |dz|", dz.max(), "agreeing groups", r["agree"].mean())
    assert np.isfinite(r["z"]).all() and np.isfinite(r["zeros"].astype(np.float32)).all()
    assert r["agree"].mean() >= 0.98


@pytest.mark.parametrize("name", NAMES)
def test_codes_match_the_reference_inside_agreeing_groups(name):
    g, r = case(name)
    mask = np.repeat(r["agree"], g["groupsize"], 1)
    diff = r["codes"].astype(np.int32) - g["Wq"].astype(np.int32)
    print(name, "codes that differ inside agreeing groups:", (diff[mask] != 0).mean())
    assert np.abs(diff[mask]).max() <= 1
    assert (diff[mask] != 0).mean() <= 0.005


@pytest.mark.parametrize("name", NAMES)
def test_codes_are_what_the_kernels_own_s_and_z_imply(name):
    g, r = case(name)
    assert np.array_equal(r["codes"], r["host_codes"])


@pytest.mark.parametrize("name", NAMES)
def test_quality_against_the_reference_and_round_to_nearest(name):
    g, r = case(name)
    err = float(np.abs(g["W"] - r["wdq"]).astype(np.float32).mean(dtype=np.float32))
    err_opt, err_rtn = float(g["err_opt"]), float(g["err_rtn"])
    # for information: the error of the STORED layer, fp16 scales and zero points (what QuantLinearHQQ dequantises)
    gs = g["groupsize"]
    stored = (r["codes"].astype(np.float32) - np.repeat(r["zeros"].astype(np.float32), gs, 1)) * np.repeat(r["scales"].astype(np.float32), gs, 1)
    print(name, "err/err_opt", err / err_opt, "err_rtn/err_opt", err_rtn / err_opt, "stored fp16 err/err_opt", float(np.abs(g["W"] - stored).mean()) / err_opt)
    assert err <= err_opt * 1.002
    assert err < err_rtn - 0.5 * (err_rtn - err_opt)


@pytest.mark.parametrize("name", NAMES)
def test_packed_layout_is_the_row_stream_of_the_codes(name):
    g, r = case(name)
    q_kn = torch.from_numpy(np.ascontiguousarray(r["host_codes"].T)).to(DEV)
    assert torch.equal(r["qweight"], ops.pack_qweight(q_kn, "HQQ", g["bits"]))
    assert np.array_equal(r["qweight"].cpu().numpy(), O.pack_along_rows(r["host_codes"].T, g["bits"]).view(np.int32))


@pytest.mark.parametrize("name", ["hqqq_w3_g64", "hqqq_w4_g128_n48"])
def test_two_calls_and_every_input_dtype_give_the_same_bytes(name):
    g, r = case(name)
    a = ops.hqq_quantize(_w_tensor(g), g["bits"], g["groupsize"])
    b = ops.hqq_quantize(_w_tensor(g), g["bits"], g["groupsize"])
    c = ops.hqq_quantize(_w_tensor(g, torch.float32), g["bits"], g["groupsize"])   # the same values read as fp32
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    assert torch.equal(a[0], r["qweight"]) and int(a[3].item()) == r["rounds"]


def test_a_captured_call_replays_to_the_same_bytes():
    g, r = case("hqqq_w4_g64")
    w = _w_tensor(g)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.hqq_quantize(w, g["bits"], g["groupsize"])      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.hqq_quantize(w, g["bits"], g["groupsize"])
    for t in out:
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out[0], r["qweight"]) and int(out[3].item()) == r["rounds"]
    assert np.array_equal(out[1].cpu().numpy().T, r["scales"]) and np.array_equal(out[2].cpu().numpy().T, r["zeros"])


def _torch_solver(W, bits, g, rounds):
    """The solver's loop as torch elementwise ops in fp32 on the device, run for a GIVEN number of rounds: (s, z) [N, G]."""
    N, K = W.shape
    Wg = W.float().reshape(-1, g)
    max_v = 2 ** bits - 1
    mn, mx = Wg.min(1, keepdim=True)[0], Wg.max(1, keepdim=True)[0]
    s = (max_v / (mx - mn)).clamp(max=2e4)
    z = torch.round(-mn * s)
    beta = 10.0
    for _ in range(rounds):
        wq = torch.round(Wg * s + z).clamp(0, max_v)
        x = Wg - (wq - z) / s
        we = torch.sign(x) * torch.relu(x.abs() - (1.0 / beta) * x.abs().pow(0.7 - 1))
        z = (wq - (Wg - we) * s).mean(1, keepdim=True)
        beta *= 1.01
    return s.reshape(N, K // g), z.reshape(N, K // g)


@pytest.mark.parametrize("N,K,g,bits", [
    (1024, 2048, 32, 4),     # 4096 tiles on 2048 blocks: every block walks two tiles; 2 elements per lane
    (64, 768, 96, 3),        # 6 elements per lane in the 8-wide instantiation (masked tail)
    (32, 2048, 1024, 8),     # the widest group: 64 elements per lane
    (48, 1024, 256, 2),      # 16 per lane
    (16, 1536, 512, 4),      # 32 per lane, a single row tile
])
def test_every_kernel_form_agrees_with_the_elementwise_loop(N, K, g, bits):
    W = (0.02 * torch.randn((N, K), generator=torch.Generator().manual_seed(N + K + g))).half().to(DEV)
    W[3, :g] = W[3, 0]                                           # a flat group
    qweight, scales, zeros, rounds, s, z, _ = ops.hqq_quantize(W, bits, g, debug=True)
    run = int(rounds.item())
    assert 1 <= run <= 20
    s_ref, z_ref = _torch_solver(W, bits, g, run)
    assert torch.equal(s.T, s_ref)
    assert torch.isfinite(z).all()
    assert ((z.T - z_ref).abs() <= 1e-3).float().mean().item() >= 0.98
    codes = ops.unpack_qweight(qweight, "HQQ", bits, K, N).T
    want = torch.round(W.float() * s.T.repeat_interleave(g, 1) + z.T.repeat_interleave(g, 1)).clamp(0, 2 ** bits - 1)
    assert torch.equal(codes.float(), want)
    assert torch.equal(scales, (1.0 / s).half()) and torch.equal(zeros, z.half())


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_quantize_linear_runs_on_the_fused_routes(bits):
    from qllm_amd.quantization import quantize_linear
    K, N, g = 256, 128, 64
    gen = torch.Generator().manual_seed(bits)
    lin = torch.nn.Linear(K, N, bias=True).half()
    lin.weight.data = (0.02 * torch.randn((N, K), generator=gen)).half()
    lin.bias.data = (0.5 * torch.randn(N, generator=gen)).half()
    bias = lin.bias.data.clone()
    layer = quantize_linear(lin, bits, g, device=DEV)
    assert lin.weight.numel() == 0                                # the fp16 weight is gone
    assert layer.bits == bits and layer.groupsize == g and torch.equal(layer.bias.cpu(), bias)
    qw, sc, qz = layer.qweight.cpu().numpy(), layer.scales.cpu().numpy(), layer.qzeros.cpu().numpy()
    for m in (1, 33):
        x = (torch.randn((m, K), generator=gen)).half()
        y = layer(x.to(DEV)).cpu().numpy()
        y_ref = O.forward("HQQ", x.numpy(), qw, sc, qz, None, bias.numpy(), bits, g, K).numpy()
        assert O.rel_err(y, y_ref) <= 1e-2, (bits, m, O.rel_err(y, y_ref))
    plan = ops.plan_describe([layer.decode_descriptor()], 1)
    if bits in (3, 4):
        assert plan.startswith("strip") and "layout=strip-major" in plan, plan     # the native fused route
    else:
        assert plan.startswith("bitgemv"), plan


def test_quantize_model_mixed_3_4_bits_survives_save_and_load(tmp_path):
    from test_loader_repack_cpu import _tiny_llama
    from qllm_amd.modeling import base
    from qllm_amd.modeling.q_layers import QuantLinearHQQ
    from qllm_amd.quantization import quantize_model
    from qllm_amd.utils import modelutils
    import transformers
    tiny = _tiny_llama()
    # the same weights in a model built the way the loader builds one (fp16 default dtype, no .half() afterwards): .half() also rounds
    # the rotary table, which no checkpoint stores -- logits before and after could then only agree at position 0
    torch.set_default_dtype(torch.float16)
    try:
        model = transformers.AutoModelForCausalLM.from_config(tiny.config)
    finally:
        torch.set_default_dtype(torch.float32)
    model.load_state_dict(tiny.state_dict())
    kinds = {"q_proj": 3, "k_proj": 3, "gate_proj": 3, "up_proj": 3}         # v / o / down keep 4 bits
    model = quantize_model(model, 4, 64, bits_by_layer=kinds, device=DEV).eval()
    layers = modelutils.find_layers(model, [QuantLinearHQQ])
    assert len(layers) == 14 and "lm_head" not in layers
    assert all(l.bits == kinds.get(n.rsplit(".", 1)[1], 4) for n, l in layers.items())
    assert not any(isinstance(m, torch.nn.Linear) for n, m in model.named_modules() if ".layers." in n)
    ids = torch.randint(0, 128, (2, 6), generator=torch.Generator().manual_seed(0)).to(DEV)
    with torch.no_grad():
        before = model(ids).logits
    assert torch.isfinite(before).all()
    d = str(tmp_path / "hqq_mixed")
    base.save_quantized(model, d)
    assert json.load(open(os.path.join(d, "quantize_config.json")))["version"] == "HQQ"
    by_layer = json.load(open(os.path.join(d, "quant_config_by_layer.json")))
    assert {v["wbits"] for v in by_layer.values()} == {3, 4} and len(by_layer) == 14
    loaded = base.load_quantized(d, device=DEV)
    assert {n: l.bits for n, l in modelutils.find_layers(loaded, [QuantLinearHQQ]).items()} == {n: l.bits for n, l in layers.items()}
    with torch.no_grad():
        after = loaded(ids).logits
    assert torch.equal(before, after)
    a, b = model.state_dict(), loaded.state_dict()
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
