"""-m gpu: the routed experts at decode as two kernels (csrc/moe_decode.hip) through ops.moe_gate_up / ops.moe_down and QuantExperts.
Shapes (E, top_k, H, I): (4, 2, 256, 384); (8, 8, 512, 128) -- every expert hit; (6, 3, 1152, 640) -- 9 and 5 groups: the wave split of K
and of (slot, K) is uneven.  Id rows: descending ids, the last expert, different experts per token, one slot equal to E (the sentinel)."""
import functools

import pytest
import torch

import exact_inputs as X
from gpu_util import synth, to_layer
from test_moe_decode_cpu import tiny_checkpoint

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(4, 2, 256, 384), (8, 8, 512, 128), (6, 3, 1152, 640)]
DTYPES = pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
CASES = pytest.mark.parametrize("t", [1, 3, 4])
WEIGHTS = pytest.mark.parametrize("w32", [True, False], ids=["w_f32", "w_act"])
_r = lambda v, dtype: v.to(dtype).double()   # noqa: E731  rounded to the activation type


def _ids(e, top_k, t):
    """[t, top_k] int64: row 0 descending from the last expert, row 1 ascending from 0, row 2 with the sentinel E in its last slot, row 3 odd."""
    rows = [[(e - 1 - j) % e for j in range(top_k)], list(range(top_k)), [(j + 1) % e for j in range(top_k - 1)] + [e],
            [(e - 2 - 2 * j) % e for j in range(top_k)] if 2 * top_k <= e else list(range(top_k))[::-1]]
    return torch.tensor(rows[:t] if t > 1 else rows[:1], dtype=torch.int64)


@functools.lru_cache(maxsize=None)
def _experts(shape, exact):
    """(QuantExperts on the device with its stacks built, W64 [3][E] float64 on the CPU, the largest scale): GPTQ layers, exact ones
    (integers, power-of-two scales: W is s (q - z)) or realistic ones (W: what ops.dequant returns)."""
    from qllm_amd import ops
    from qllm_amd.modeling.q_layers import QuantExperts
    e, _, h, i = shape
    layers, w64, smax = [], [[], [], []], 0.0
    for ex in range(e):
        trio = []
        for kind, (k, n) in enumerate(((h, i), (h, i), (i, h))):
            d = (X.synth_exact if exact else synth)("GPTQ", 4, 128, k, n, seed=100 * ex + kind)
            trio.append(to_layer(d, DEV))
            smax = max(smax, float(d["scales"].max()))
            w64[kind].append(X.layer_w64(d) if exact else ops.dequant(trio[-1]._descriptor(None, 0), torch.device(DEV)).double().cpu())
        layers.append(trio)
    mod = QuantExperts(("w1", "w3", "w2"), layers, torch.nn.SiLU())
    mod._stacks = mod._build_stacks()
    assert mod._stacks, "the layers must stack"
    return mod, w64, smax


def _down_model(h, ids, wts, w_down, e, dtype):
    """float64 with the contract's roundings: round(d), round(round(d) * w) with the product in fp32, adds in ascending id, one rounding each."""
    t, top_k = ids.shape
    y = torch.zeros(t, w_down[0].shape[1], dtype=torch.float64)
    for tt in range(t):
        for j in sorted(range(top_k), key=lambda j: (int(ids[tt, j]), j)):
            ex = int(ids[tt, j])
            if 0 <= ex < e:
                p = (_r(h[tt * top_k + j].double() @ w_down[ex], dtype).float() * wts[tt, j].float()).double()
                y[tt] = _r(y[tt] + _r(p, dtype), dtype)
    return y


@WEIGHTS
@CASES
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@DTYPES
def test_exact_inputs_give_the_contract_bit_for_bit(dtype, shape, t, w32):
    """Every fp32 sum is exact, so each kernel has ONE right answer.  A: integer x (SiLU of the rounded gate by torch on the device: the eager
    rounding the contract names).  B: integer h, random weights whose products and adds round: a wrong expert, slot or order changes bits."""
    from qllm_amd import ops
    (e, top_k, hid, inter), (mod, w64, _) = shape, _experts(shape, True)
    gate, up, down, azb = mod._stacks
    g = torch.Generator().manual_seed(7 * t + top_k)
    ids = _ids(e, top_k, t)
    x = torch.randint(-2, 3, (t, hid), generator=g).to(dtype)
    got = ops.moe_gate_up(x.to(DEV), ids.to(DEV), gate, up)
    hin = torch.randint(-2, 3, (t * top_k, inter), generator=g).to(dtype)
    wts = torch.rand(t, top_k, generator=g).to(torch.float32 if w32 else dtype)
    y = ops.moe_down(hin.to(DEV), ids.to(DEV), wts.to(DEV), down)
    for slot in range(t * top_k):
        ex = int(ids.view(-1)[slot])
        if ex == e:
            continue
        xs = x[slot // top_k].double()
        gh, uh = (xs @ w64[0][ex]).to(dtype), (xs @ w64[1][ex]).to(dtype)
        want = (torch.nn.functional.silu(gh.to(DEV)).cpu().double() * uh.double()).to(dtype)
        assert torch.equal(got[slot].cpu(), want), (slot, ex, X.mismatches(got[slot:slot + 1].cpu(), want[None])[1])
    want_y = _down_model(hin, ids, wts, w64[2], e, dtype).to(dtype)
    assert torch.equal(y.cpu(), want_y), X.mismatches(y.cpu(), want_y)


def _bound_and_ref(x, ids, wts, w64, scales_max, e, dtype):
    """float64 y and the bound on |y_kernel - y|, followed through the contract's rounding points.  u: unit roundoff of the activation
    type; per matvec over K terms: K 2^-24 sum |x w| for the fp32 accumulation in any order, plus sum |x| dW with dW = 30 * 2^-11 s_max --
    ops.dequant's W carries three fp16 roundings (q s, z s, their difference; q, z <= 15) the kernels' unrounded W does not.  SiLU has slope
    <= 1.1; every rounding adds u times the value; the adds of the routed sum add u times the running sum of magnitudes."""
    u, f32 = (2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8), 2.0 ** -24
    t, top_k = ids.shape
    y, by = torch.zeros(t, x.shape[1], dtype=torch.float64), torch.zeros(t, x.shape[1], dtype=torch.float64)

    def matvec(v, ev, w, smax):   # value, and bound given the input's own error ev
        val = v @ w
        return val, (ev + (v.shape[0] * f32) * v.abs()) @ w.abs() + (v.abs().sum() + ev.sum()) * 30 * 2.0 ** -11 * smax
    for tt in range(t):
        mags = torch.zeros_like(y[tt])
        for j in range(top_k):
            ex = int(ids[tt, j])
            if not 0 <= ex < e:
                continue
            xs = x[tt].double()
            (gv, bg), (uv, bu) = matvec(xs, torch.zeros_like(xs), w64[0][ex], scales_max), matvec(xs, torch.zeros_like(xs), w64[1][ex], scales_max)
            bg, bu = bg + u * gv.abs(), bu + u * uv.abs()
            sv = torch.nn.functional.silu(gv)
            bs = 1.1 * bg + u * (sv.abs() + 1.1 * bg)
            hv = sv * uv
            bh = bs * uv.abs() + sv.abs() * bu + bs * bu
            bh = bh + u * (hv.abs() + bh)
            dv, bd = matvec(hv, bh, w64[2][ex], scales_max)
            bd = bd + u * (dv.abs() + bd)
            wv = wts[tt, j].double().abs()
            bp = bd * wv + (u + f32) * (dv.abs() + bd) * wv
            y[tt] += dv * wts[tt, j].double()
            by[tt] += bp
            mags += dv.abs() * wv + bp
        by[tt] += top_k * u * mags
    return y, by + torch.finfo(dtype).tiny


@WEIGHTS
@CASES
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@DTYPES
def test_realistic_values_within_the_derived_bound_on_both_routes(dtype, shape, t, w32):
    from qllm_amd import ops
    (e, top_k, hid, inter), (mod, w64, smax) = shape, _experts(shape, False)
    gate, up, down, azb = mod._stacks
    g = torch.Generator().manual_seed(11 * t + top_k)
    ids = _ids(e, top_k, t)
    x = torch.randn(t, hid, generator=g).to(dtype)
    wts = torch.softmax(torch.randn(t, top_k, generator=g), -1).to(torch.float32 if w32 else dtype)
    ref, bound = _bound_and_ref(x, ids, wts, w64, smax, e, dtype)
    xd, idd, wd = x.to(DEV), ids.to(DEV), wts.to(DEV)
    fused = ops.moe_down(ops.moe_gate_up(xd, idd, gate, up), idd, wd, down)
    loop = mod.forward_loop(xd, idd, wd)
    r_fused, r_loop = (((o.cpu().double() - ref).abs() / bound).max().item() for o in (fused, loop))
    print(f"moe_decode {dtype} {shape} T={t} w32={w32}: max |err| / bound fused {r_fused:.4f} loop {r_loop:.4f}")
    assert r_loop <= 1.0, "the bound is wrong: the unfused loop misses it"
    assert r_fused <= 1.0
    assert torch.equal(mod(xd, idd, wd), fused if t == 1 or 2 * t * top_k <= e else loop)   # the route moe_plan names, the same bits again


@DTYPES
def test_a_captured_step_follows_the_contents_of_ids_and_weights(dtype):
    from qllm_amd import ops
    e, top_k, hid, _ = SHAPES[0]
    gate, up, down, _ = _experts(SHAPES[0], False)[0]._stacks
    g = torch.Generator().manual_seed(5)
    x = torch.randn(3, hid, generator=g).to(dtype).to(DEV)
    eager = lambda x, ids, wts: ops.moe_down(ops.moe_gate_up(x, ids, gate, up), ids, wts, down)   # noqa: E731  (the module would loop here)
    ids_a, ids_b = _ids(e, top_k, 3).to(DEV), _ids(e, top_k, 4)[1:].contiguous().to(DEV)
    w_a, w_b = (torch.softmax(torch.randn(3, top_k, generator=g), -1).to(DEV) for _ in range(2))
    ids, wts = ids_a.clone(), w_a.clone()
    eager(x, ids, wts), torch.cuda.synchronize()       # warm-up outside the capture
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = eager(x, ids, wts)
    ids.copy_(ids_b), wts.copy_(w_b)
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager(x, ids_b, w_b)) and not torch.equal(out, eager(x, ids_a, w_a))


def _logits_close(got, want, label):
    """8 fp16 units at the logits' size.  NOT derived from check 2's bound, which cannot be followed through attention, norms
    and lm_head: chosen, on this reasoning -- both routes round to fp16 at the same points and differ in fp32 summation order (the
    attention kernel: in its fp32 softmax), so single values flip by one unit on the way and a few such flips meet in a logit."""
    diff, tol = (got.float() - want.float()).abs().max().item(), 8 * 2.0 ** -11 * want.float().abs().max().item()
    print(f"{label}: max |difference| {diff:.3e} allowed {tol:.3e}")
    assert bool(torch.isfinite(got).all()) and diff <= tol


@pytest.mark.parametrize("family", ["mixtral", "qwen3_moe"])
def test_a_quantized_checkpoint_loads_decodes_in_two_launches_per_block_and_takes_the_attention_installs(family, tmp_path, monkeypatch):
    """The installs: fuse_rope + fuse_attention, a 6-token prompt and one decode step through a cache -- for Mixtral behind a sliding window
    of 4, which the restated forward has to hand on -- against the same checkpoint loaded without them."""
    from qllm_amd import ops
    from qllm_amd.modeling.base import load_quantized
    from qllm_amd.modeling.q_layers import QuantExperts
    tiny_checkpoint(str(tmp_path), family)
    model, installed = load_quantized(str(tmp_path), device=DEV), load_quantized(str(tmp_path), device=DEV, fuse_rope=True, fuse_attention=True)
    assert model.quant_experts == 2 and model.load_report == dict(quantized_layers=2 * 4 * 3, unexpected_keys=[])
    assert (installed.quant_experts, installed.fused_ropes, installed.fused_attentions) == (2, 2, 2)
    prompt, nxt = torch.tensor([[5, 9, 33, 2, 17, 40]], device=DEV), torch.tensor([[7]], device=DEV)
    calls = dict(moe=0, linear=0)
    for key, names in (("moe", ("moe_gate_up", "moe_down")), ("linear", ("linear_forward", "linear_forward_grouped"))):
        for name in names:
            real = getattr(ops, name)
            monkeypatch.setattr(ops, name, lambda *a, _real=real, _key=key, **kw: (calls.__setitem__(_key, calls[_key] + 1), _real(*a, **kw))[1])
    with torch.no_grad():
        fused = model(nxt).logits                              # one decode step
        assert calls == dict(moe=2 * 2, linear=0)              # two blocks, two launches each, and no other matvec of the library
        monkeypatch.setenv("QLLM_FUSE_MOE", "0")
        _logits_close(fused, model(nxt).logits, family)
        assert calls == dict(moe=4, linear=2 * 2 * 3)          # per block two hit experts, three layers each
        monkeypatch.delenv("QLLM_FUSE_MOE")
        for step in range(2):
            outs = [m(prompt, use_cache=True) if step == 0 else m(nxt, past_key_values=m.moe_test_cache, use_cache=True) for m in (model, installed)]
            model.moe_test_cache, installed.moe_test_cache = (o.past_key_values for o in outs)
            _logits_close(outs[1].logits, outs[0].logits, f"{family} installs step {step}")
    assert all(m._stacks for m in model.modules() if isinstance(m, QuantExperts))
