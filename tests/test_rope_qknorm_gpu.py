"""-m gpu: Qwen3's q_norm / k_norm and rotary embedding as one kernel (qllm_rope_qknorm, csrc/rope_qknorm.hip) through ops.rope_qknorm and
the modules.  Shapes (B, S, Hq, Hk): (1, 1, 3, 1) -- one token, half a wave of work; (2, 5, 4, 2) -- [B, S, D] tables; (1, 2048, 40, 8) at
D = 128 -- 98304 heads of 8 lanes, more than the capped grid's 256 x 8 x 256 threads: the grid-stride loop."""
import functools

import pytest
import torch

from decode_loop_cases import LAYERS, M_DEVICE, batch_inputs, count_calls, error, float64_copy, run
from test_rope_cpu import module_dicts
from test_rope_qknorm_cpu import tiny_qwen3

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-6
SMALL = [(d, shape) for shape in ((1, 1, 3, 1), (2, 5, 4, 2)) for d in (64, 128)]
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])


@functools.lru_cache(maxsize=None)
def _inputs(dtype, d, shape):
    """CPU tensors q [B, S, Hq, D], k [B, S, Hk, D] (O(1), one head scaled by 2^-6 and one by 2^6), weights in [0.5, 1.5], cos, sin [B, S, D]."""
    b, s, hq, hk = shape
    g = torch.Generator().manual_seed(1000 * d + 10 * hq + s)
    q, k = torch.randn(b, s, hq, d, generator=g), torch.randn(b, s, hk, d, generator=g)
    for x in (q, k):
        x[:, :, 0] *= 2.0 ** -6
        if x.shape[2] > 1:
            x[:, :, -1] *= 2.0 ** 6
    wq, wk = torch.rand(d, generator=g) + 0.5, torch.rand(d, generator=g) + 0.5
    ang = torch.rand(b, s, d // 2, generator=g) * 6.2832
    ang = torch.cat((ang, ang), -1)
    return tuple(t.to(dtype) for t in (q, k, wq, wk, ang.cos(), ang.sin()))


@pytest.mark.parametrize("form", ["dense", "fused", "inplace"])
@pytest.mark.parametrize("d,shape", SMALL + [(128, (1, 2048, 40, 8))], ids=str)
@DTYPES
def test_bit_for_bit_the_composition_of_rmsnorm_and_rope(dtype, d, shape, form):
    """dense: [B, H, S, D] views, as the modules hand them over; fused: slices of one [B, S, (Hq + 2 Hk) D] buffer whose third part is NaN."""
    from qllm_amd import ops
    q, k, wq, wk, cos, sin = (t.to(DEV) for t in _inputs(dtype, d, shape))
    b, s, hq, hk = shape
    want = ops.rope(ops.rmsnorm(q, wq, EPS), ops.rmsnorm(k, wk, EPS), cos, sin, 2)
    if form == "dense":
        got = [o.transpose(1, 2) for o in ops.rope_qknorm(q.transpose(1, 2), k.transpose(1, 2), wq, wk, EPS, cos, sin)]
    elif form == "fused":
        buf = torch.full((b, s, (hq + 2 * hk) * d), float("nan"), dtype=dtype, device=DEV)
        buf[..., :hq * d], buf[..., hq * d:(hq + hk) * d] = q.view(b, s, -1), k.view(b, s, -1)
        got = ops.rope_qknorm(buf[..., :hq * d].view(b, s, hq, d), buf[..., hq * d:(hq + hk) * d].view(b, s, hk, d), wq, wk, EPS, cos, sin, 2)
    else:
        got = (q.clone(), k.clone())
        assert all(o is g for o, g in zip(ops.rope_qknorm(*got, wq, wk, EPS, cos, sin, 2, out=got), got))
    for g, w in zip(got, want):
        assert bool(torch.isfinite(w.float()).all()) and g.shape == w.shape and torch.equal(g, w), int((g != w).sum())


@pytest.mark.parametrize("d,shape", SMALL, ids=str)
@DTYPES
def test_against_float64_within_the_derived_bound(dtype, d, shape):
    """|out - ref| <= 4.5 u (|y cos| + |rot(y) sin|) + tiny, u = 2^-11 / 2^-8, y the float64 normed value, tiny the smallest normal: one
    rounding each for h, y and the product, one for the sum, half a unit for second-order terms; rstd's fp32 error is negligible."""
    from qllm_amd import ops
    q, k, wq, wk, cos, sin = _inputs(dtype, d, shape)
    got = ops.rope_qknorm(*(t.to(DEV) for t in (q, k, wq, wk)), EPS, cos.to(DEV), sin.to(DEV), 2)
    u, tiny = (2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8), torch.finfo(dtype).tiny
    c, s = cos.double().unsqueeze(2), sin.double().unsqueeze(2)
    for out, x, w in zip(got, (q.double(), k.double()), (wq, wk)):
        y = w.double() * x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + EPS)
        rot = torch.cat((-y[..., d // 2:], y[..., :d // 2]), -1)
        ratio = (out.cpu().double() - (y * c + rot * s)).abs() / (4.5 * u * ((y * c).abs() + (rot * s).abs()) + tiny)
        print(f"rope_qknorm {dtype} D={d} {shape}: max |err| / bound {ratio.max().item():.3f}")
        assert ratio.max().item() <= 1.0


def _counted(monkeypatch, model):
    """`count_calls` plus the rope_qknorm kernel ("qknorm") and the eager forward of the q_norm / k_norm class on [B, S, H, D] ("eager_norm")."""
    from qllm_amd import ops
    calls, norm = count_calls(monkeypatch), type(model.model.layers[0].self_attn.q_norm)
    calls.update(qknorm=0, eager_norm=0)

    def counting(name, real, when=lambda *a: True):
        def op(*a, **kw):
            calls[name] += when(*a)
            return real(*a, **kw)
        return op
    monkeypatch.setattr(ops, "rope_qknorm", counting("qknorm", ops.rope_qknorm))
    monkeypatch.setattr(norm, "forward", counting("eager_norm", norm.forward, lambda self, x: x.dim() == 4))
    return calls


@pytest.mark.parametrize("layer_types", [("full_attention", "full_attention"), ("full_attention", "sliding_attention")], ids=["full", "sliding"])
def test_tiny_qwen3_runs_one_kernel_per_layer_and_step(layer_types, monkeypatch):
    """A 5-token prefill and 4 decode steps with install_fused_rope, then with install_fused_attention on top: E(fused) <= M_DEVICE x
    E(unfused) against a float64 copy, one rope_qknorm call per layer and forward, no eager q/k norm, no plain rope kernel, and with the
    attention install one attention kernel per layer and decode step."""
    from qllm_amd.modeling.q_layers import install_fused_attention, install_fused_rope, uninstall_fused_attention, uninstall_fused_rope
    model = tiny_qwen3(device=DEV, layer_types=layer_types)
    inp, before = batch_inputs("unpadded", steps=4), module_dicts(model)
    reference = run(float64_copy(model), inp)
    e_unfused = error(run(model, inp, device=DEV), reference)
    calls = _counted(monkeypatch, model)
    assert install_fused_rope(model) == LAYERS
    for with_attention in (False, True):
        assert not with_attention or install_fused_attention(model) == LAYERS
        calls.update(dict.fromkeys(calls, 0))
        e_fused = error(run(model, inp, device=DEV, calls=calls), reference)
        print(f"tiny qwen3 {layer_types[1]} attention={with_attention}: E(unfused) {e_unfused:.3e} E(fused) {e_fused:.3e}")
        assert calls == dict(qknorm=LAYERS * 5, eager_norm=0, rope=0, attn=LAYERS * 4 * with_attention), calls
        assert e_unfused > 0 and e_fused <= M_DEVICE * e_unfused
    assert uninstall_fused_attention(model) == LAYERS and uninstall_fused_rope(model) == LAYERS and module_dicts(model) == before


@pytest.mark.parametrize("order", ["norm_first", "rope_first"])
def test_install_orders_with_the_norm_installs_restore_everything(order, monkeypatch):
    """make_quant_norm replaces q_norm and k_norm by class name (9 norms; install_fused_norm folds nothing on dense linears).  norm_first:
    the kernel still finds their weight and epsilon.  rope_first, the rope install taken away again: what replaced them serves
    [B, S, H, D] -- no eager norm runs.  Either way uninstalling puts every module back."""
    from qllm_amd.modeling.q_layers import QuantLinearGPTQ, install_fused_norm, install_fused_rope, make_quant_norm, uninstall_fused_norm, uninstall_fused_rope
    model = tiny_qwen3(device=DEV)
    inp, before = batch_inputs("single", steps=4), module_dicts(model)
    reference = run(float64_copy(model), inp)
    e_unfused = error(run(model, inp, device=DEV), reference)
    calls = _counted(monkeypatch, model)
    if order == "rope_first":
        assert install_fused_rope(model) == LAYERS
    assert install_fused_norm(model, [QuantLinearGPTQ]) == 0 and make_quant_norm(model) == 1 + 4 * LAYERS
    assert (uninstall_fused_rope if order == "rope_first" else install_fused_rope)(model) == LAYERS
    assert error(run(model, inp, device=DEV), reference) <= M_DEVICE * e_unfused
    assert (calls["qknorm"], calls["eager_norm"]) == ((LAYERS * 5, 0) if order == "norm_first" else (0, 0)), calls
    assert uninstall_fused_norm(model) == 1 + 4 * LAYERS and (order == "rope_first" or uninstall_fused_rope(model) == LAYERS)
    assert module_dicts(model) == before
