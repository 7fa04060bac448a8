"""The fused residual add of the o_proj / down_proj decode launches without a GPU: the two additive C symbols (exported, declared, bound;
ABI still 7), what qllm_residual_describe serves and refuses on hand-made native descriptors (fake, aligned, never-dereferenced pointers),
the argument checks of qllm_linear_forward_residual, the host logic of forward_residual / forward_swiglu_residual /
install_fused_residual against a fake `ops`, and the compiler's resource report: every RESID instantiation (csrc/strip1_resid.hip,
csrc/strip1_swiglu_resid.hip) free of scratch and spills, and the kernels of strip1.hip / strip1_swiglu.hip / strip1_norm.hip exactly what
they were before the RESID constant existed."""
import ctypes as C
import inspect
import json
import os
import re

import pytest
import torch

from kernel_resources import resources
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import _hip_forward, fused, fused_mlp, fused_norm, fused_residual
from strip1_families import check_family
from test_swiglu_cpu import TABLE_K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPTQ, NATIVE, NATIVE_F16Z = _lib.LAYOUT_GPTQ, _lib.LAYOUT_NATIVE, _lib.LAYOUT_NATIVE_F16Z
NAMES = ("qllm_linear_forward_residual", "qllm_residual_describe")
INV, UNS = _lib.QLLM_ERR_INVALID, _lib.QLLM_ERR_UNSUPPORTED


@pytest.fixture(scope="module")
def lib():
    if not _lib.is_built():
        import __graft_entry__
        __graft_entry__.build()
    return _lib.load()


def W(K, N=4096, g=128, bits=4, layout=NATIVE, zeros=4096):
    return _lib.QllmWeight(4096, 4096, zeros, None, None, K, N, g, bits, layout, 0)


# ---- symbols -----------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_declared_and_bound(lib):
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qllm_mi355x.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS
        assert C.cast(getattr(lib, name), C.c_void_p).value
        assert getattr(lib, name).argtypes is not None
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION
    assert all(hasattr(ops, n) and n in ops.__all__ for n in ("linear_forward_residual", "linear_forward_swiglu_residual", "residual_describe"))


# ---- what is served ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", TABLE_K)
def test_describe_names_the_plain_calls_plan(lib, K):
    for N in (256, 8192):
        for w in (W(K, N), W(K, N, layout=NATIVE_F16Z)):
            plan = ops.plan_describe([w], 1)
            assert plan.startswith("strip1 nw="), (K, N, plan)
            assert ops.residual_describe(w, 1) == "residual " + plan
            assert ops.residual_describe(w, 1, swiglu=True) == "residual swiglu " + plan == "residual " + ops.swiglu_describe(w, 1)
    for w, tag in ((W(K, g=64), " g64 "), (W(K, bits=3), " bits=3 "), (W(K, g=64, bits=3, layout=NATIVE_F16Z), " g64 bits=3 ")):
        plan = ops.plan_describe([w], 1)
        if plan.startswith("strip1 "):
            assert ops.residual_describe(w, 1) == "residual " + plan and tag in plan
            assert ops.residual_describe(w, 1, True) == "residual swiglu " + plan
        else:   # (beyond the form's K: 24576 with 64-wide groups, 16384 with 3 bits)
            assert K > 16384 and ops.residual_describe(w, 1).startswith("refused: ") and ops.residual_describe(w, 1, True).startswith("refused: ")


REFUSED = ((W(4096), 2),                        # two rows
           (W(4096), 4),
           (W(4096, layout=GPTQ), 1),           # the reference layout
           (W(4096, bits=8, layout=GPTQ), 1),   # 8 bits
           (W(4096, bits=8), 1),
           (W(192, g=64), 1))                   # K / 32 < 8 k-steps


def test_refusals(lib):
    for w, m in REFUSED:
        for sw in (False, True):
            text = ops.residual_describe(w, m, sw)
            assert text.startswith("refused: "), (w.K, w.bits, w.group_size, w.layout, m, text)


def test_a_knob_that_takes_the_shape_off_the_kernel_turns_the_answer_into_a_refusal(lib):
    w = W(11008)
    assert ops.residual_describe(w, 1) == "residual strip1 nw=15 round=24 grid=strips x 1 layout=strip-major"
    try:
        ops.set_knob("QLLM_STRIP1", 0)
        assert ops.residual_describe(w, 1).startswith("refused: ") and ops.residual_describe(w, 1, True).startswith("refused: ")
        assert not ops.plan_describe([w], 1).startswith("strip1 ")
    finally:
        ops.reset_knobs()
    assert ops.residual_describe(w, 1, True).startswith("residual swiglu strip1 ")


def test_describe_arguments(lib):
    buf = C.create_string_buffer(640)
    w = W(4096)
    assert lib.qllm_residual_describe(C.byref(w), 0, 0, buf, 640) == INV
    assert lib.qllm_residual_describe(None, 1, 0, buf, 640) == INV
    assert lib.qllm_residual_describe(C.byref(w), 1, 0, None, 640) == INV
    assert lib.qllm_residual_describe(C.byref(w), 1, 0, buf, 8) == INV


def test_invalid_arguments_are_reported_before_any_device_work(lib):
    """Only where no HIP device is visible: a slip that turned one of these refusals into a launch would run a kernel on fake pointers."""
    if torch.cuda.is_available():
        pytest.skip("a HIP device is visible: the forward entry is not called with fake pointers")
    w = W(4096, 256)
    x, up, r, y = 4096, 1 << 16, 1 << 20, 1 << 21     # (x / up: 8 KB each, residual / y: 512 bytes each)

    def call(xx=x, uu=None, rr=r, yy=y, m=1, dt=_lib.DT_F16, act=_lib.ACT_SILU, ww=w):
        p = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
        return lib.qllm_linear_forward_residual(C.byref(ww) if ww is not None else None, p(xx), p(uu), p(rr), p(yy), m, dt, act, None)

    def named(rc, *words):
        return rc == INV and all(wd in _lib.last_error() for wd in words)

    assert named(call(xx=None), "x", "NULL") and named(call(rr=None), "residual", "NULL") and named(call(yy=None), "y", "NULL")
    assert call(ww=None) == INV
    assert named(call(m=0), "M must be")
    assert named(call(dt=7), "act_dtype")
    assert named(call(xx=x + 8), "x", "aligned") and named(call(uu=up + 8), "up", "aligned") and named(call(rr=r + 1), "residual", "aligned")
    assert named(call(yy=x), "alias", "x") and named(call(uu=up, yy=up), "alias", "up")
    assert named(call(yy=x + 4096), "alias")                       # inside x's row
    assert named(call(yy=r + 2), "residual", "overlap") and named(call(yy=r - 2), "residual", "overlap")   # y overlapping residual, not equal to it
    assert named(call(uu=up, act=1), "act=1")
    # a residual two bytes off a 16-byte boundary is fine (element alignment); every valid call on a refused shape is UNSUPPORTED, y == residual included
    for ww, m in REFUSED:
        for uu in (None, up):
            for rr, yy in ((r, y), (r, r), (r + 2, y)):
                assert call(uu=uu, rr=rr, yy=yy, m=m, ww=ww) == UNS, (ww.K, ww.bits, ww.layout, m, _lib.last_error())
                assert "fused residual" in _lib.last_error() or (ww.bits == 8 and ww.layout == NATIVE)   # (8 native bits: the descriptor's own refusal)
    assert call(uu=None, act=1, ww=REFUSED[0][0], m=2) == UNS       # (act is read with `up` only)
    try:
        ops.set_knob("QLLM_STRIP1", 0)
        assert call(yy=r) == UNS and call(uu=up) == UNS
    finally:
        ops.reset_knobs()


# ---- host logic against a fake `ops` -----------------------------------------------------------------------------------------------------
class _Q(torch.nn.Module, _hip_forward.HipForwardMixin):
    """A q_layer as far as the fused residual code looks at it: forward(x) = x @ w, on any device."""
    act_order = None
    bits, groupsize = 4, 128

    def __init__(self, k, n, native=True, seed=0):
        super().__init__()
        self.infeatures, self.outfeatures, self.native = k, n, native
        self.w = (torch.randn(k, n, generator=torch.Generator().manual_seed(seed + n)) * 0.1).half()
        self.own = 0

    def _layout_name(self):
        return "HQQ"

    def native_descriptor(self, add_zero_bias=0):
        return self if self.native else None

    def decode_descriptor(self, g_idx=None, add_zero_bias=0):
        return self

    def forward(self, x):
        self.own += 1
        return (x.float() @ self.w.float()).to(x.dtype)


def _fake_ops(monkeypatch, refuse=False, refuse_swiglu=False):
    """The two fused entries and ops.linear_forward_swiglu computed by torch on whatever device, `_fused_tensors_ok` without its device
    test (the real one is handed back as calls["real_ok"])."""
    calls = {"plain": 0, "swiglu": 0, "mlp": 0}

    def plain(w, x2d, r2d, out=None):
        calls["plain"] += 1
        if refuse:
            raise ops.QllmUnsupported(2, "fused residual: refused")
        assert out is None                                         # module calls never write in place
        return r2d + (x2d.float() @ w.w.float()).to(x2d.dtype)

    def swiglu(w, g2d, u2d, r2d, out=None):
        calls["swiglu"] += 1
        if refuse_swiglu:
            raise ops.QllmUnsupported(2, "fused residual: refused")
        assert out is None
        return r2d + ((torch.nn.functional.silu(g2d) * u2d).float() @ w.w.float()).to(g2d.dtype)

    def mlp(w, g2d, u2d, out=None):
        calls["mlp"] += 1
        return ((torch.nn.functional.silu(g2d) * u2d).float() @ w.w.float()).to(g2d.dtype)

    monkeypatch.setattr(_hip_forward.ops, "linear_forward_residual", plain)
    monkeypatch.setattr(_hip_forward.ops, "linear_forward_swiglu_residual", swiglu)
    monkeypatch.setattr(_hip_forward.ops, "linear_forward_swiglu", mlp)
    real = _hip_forward._fused_tensors_ok
    monkeypatch.setattr(_hip_forward, "_fused_tensors_ok",
                        lambda *ts: ts[0].dtype in (torch.float16, torch.bfloat16) and all(t.dtype == ts[0].dtype for t in ts)
                        and not (torch.is_grad_enabled() and any(t.requires_grad for t in ts)))
    calls["real_ok"] = real
    return calls


def _rnd(*shape, seed=0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)).half()


def test_forward_residual_remembers_a_refusal_and_falls_back_to_the_eager_add(monkeypatch):
    calls = _fake_ops(monkeypatch, refuse=True, refuse_swiglu=True)
    q = _Q(16, 8)
    x, r = _rnd(1, 1, 16, seed=1), _rnd(1, 1, 8, seed=2)
    g, u = _rnd(1, 1, 16, seed=3), _rnd(1, 1, 16, seed=4)
    with torch.no_grad():
        want, want_sw = r + q(x), r + q.forward_swiglu(g, u)
        assert calls["mlp"] == 1
        for _ in range(3):
            assert torch.equal(q.forward_residual(x, r), want)
            assert torch.equal(q.forward_swiglu_residual(g, u, r), want_sw)
    assert calls["plain"] == 1 and calls["swiglu"] == 1               # asked once each, remembered
    assert q._residual_refused and q._swiglu_residual_refused
    q._invalidate()                                                   # new buffers: asked again
    assert not q._residual_refused and not q._swiglu_residual_refused
    with torch.no_grad():
        q.forward_residual(x, r)
    assert calls["plain"] == 2


def test_forward_residual_does_not_try_what_the_entry_cannot_take(monkeypatch):
    calls = _fake_ops(monkeypatch)
    x, r = _rnd(1, 16, seed=1), _rnd(1, 8, seed=2)
    g, u = _rnd(1, 16, seed=3), _rnd(1, 16, seed=4)
    with torch.no_grad():
        q = _Q(16, 8)
        want = r + q(x)
        assert torch.equal(q.forward_residual(x, r), want) and calls["plain"] == 1          # served: the fused entry, not the layer's forward
        own = q.own
        assert torch.equal(q.forward_swiglu_residual(g, u, r), r + q.forward_swiglu(g, u)) and calls["swiglu"] == 1 and q.own == own
        n = dict(calls)
        assert torch.equal(_Q(16, 8, native=False).forward_residual(x, r), want)             # no native copy
        ao = _Q(16, 8)
        ao.act_order = True
        assert torch.equal(ao.forward_residual(x, r), want)                                   # act-order
        assert torch.equal(q.forward_residual(x, r.float()), r.float() + q(x))                # dtypes disagree
        xt = _rnd(16, 2, seed=5).t()[:1]
        assert torch.equal(q.forward_residual(xt, r), r + q(xt))                              # not contiguous
        assert torch.equal(q.forward_residual(x.float(), r.float()), r.float() + q(x.float()))   # not an activation type of the kernels
        x2, r2 = _rnd(2, 16, seed=6), _rnd(2, 8, seed=7)
        assert q.residual_max_m == 1
        assert torch.equal(q.forward_residual(x2, r2), r2 + q(x2))                            # two rows: above the cap
        assert torch.equal(q.forward_residual(x, r2), r2 + q(x))                              # a residual of another leading shape: broadcast, eagerly
        assert torch.equal(q.forward_swiglu_residual(g, _rnd(1, 16, seed=8).float(), r), r + q.forward_swiglu(g, _rnd(1, 16, seed=8).float()))
        assert {k: calls[k] for k in ("plain", "swiglu")} == {k: n[k] for k in ("plain", "swiglu")}
    xg = x.clone().float().requires_grad_().half()
    q.forward_residual(xg, r)                                                                 # grad mode with an input to differentiate
    assert calls["plain"] == n["plain"]
    # CPU tensors, with the real device test: never sent
    assert not calls["real_ok"](x, r)
    monkeypatch.setattr(_hip_forward, "_fused_tensors_ok", calls["real_ok"])
    with torch.no_grad():
        assert torch.equal(q.forward_residual(x, r), want) and calls["plain"] == n["plain"]
    assert isinstance(_hip_forward.HipForwardMixin.residual_max_m, int)


# ---- install_fused_residual against local classes of the whitelisted names ------------------------------------------------------------------
class LlamaRMSNorm(torch.nn.Module):
    def __init__(self, k, eps=1e-5):
        super().__init__()
        self.weight = torch.nn.Parameter((torch.randn(k, generator=torch.Generator().manual_seed(k)) * 0.1 + 1).half())
        self.variance_epsilon = eps

    def forward(self, hidden_states):
        dt = hidden_states.dtype
        h = hidden_states.to(torch.float32)
        h = h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + self.variance_epsilon)
        return self.weight * h.to(dt)


class LlamaAttention(torch.nn.Module):
    def __init__(self, k, o_proj=None):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj = _Q(k, 32, seed=1), _Q(k, 16, seed=2), _Q(k, 16, seed=3)
        self.o_proj = o_proj if o_proj is not None else _Q(32, k, seed=4)
        self.fail = False
        self.skip_o = False
        self.seen = None

    def forward(self, hidden_states, scale=1.0, **kwargs):
        self.seen = dict(kwargs, scale=scale)
        x = hidden_states
        mix = self.q_proj(x) * 0.1 + torch.cat([self.k_proj(x), self.v_proj(x)], -1) * 0.1
        if self.fail:
            raise RuntimeError("attention failed")
        if self.skip_o:
            return mix[..., :x.shape[-1]] * scale, None
        return self.o_proj(mix * scale), None


class LlamaMLP(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _Q(k, 32, seed=5), _Q(k, 32, seed=6), _Q(32, k, seed=7)
        self.act_fn = torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class LlamaDecoderLayer(torch.nn.Module):
    def __init__(self, k=16, o_proj=None):
        super().__init__()
        self.self_attn, self.mlp = LlamaAttention(k, o_proj), LlamaMLP(k)
        self.input_layernorm, self.post_attention_layernorm = LlamaRMSNorm(k), LlamaRMSNorm(k)

    def forward(self, hidden_states: torch.Tensor, scale: float = 1.0, **kwargs) -> torch.Tensor:
        residual = hidden_states
        hidden_states = self.input_layernorm(hidden_states)
        hidden_states, _ = self.self_attn(hidden_states=hidden_states, scale=scale, **kwargs)
        hidden_states = residual + hidden_states
        residual = hidden_states
        hidden_states = self.post_attention_layernorm(hidden_states)
        hidden_states = self.mlp(hidden_states)
        return residual + hidden_states


class MistralDecoderLayer(LlamaDecoderLayer):
    """A tuple-returning layer of an older release: not guessed at."""

    def forward(self, hidden_states: torch.Tensor, scale: float = 1.0, **kwargs) -> tuple:
        return (LlamaDecoderLayer.forward(self, hidden_states, scale, **kwargs),)


class GemmaDecoderLayer(LlamaDecoderLayer):
    pass


def _model():
    m = torch.nn.Module()
    m.a = LlamaDecoderLayer()
    m.b = MistralDecoderLayer()                                    # annotated to return a tuple
    m.c = LlamaDecoderLayer(o_proj=torch.nn.Linear(32, 16).half())   # o_proj is no q_layer
    m.d = GemmaDecoderLayer()                                      # not on the list
    m.e = LlamaDecoderLayer()
    return m


def _dicts(m):
    return {n: dict(mod.__dict__) for n, mod in m.named_modules()}


def test_install_patches_only_verified_layers_and_uninstall_restores(monkeypatch):
    _fake_ops(monkeypatch)
    m = _model()
    x = _rnd(1, 1, 16, seed=9)
    with torch.no_grad():
        want = {n: getattr(m, n)(x) for n in "ace"}
    before = _dicts(m)
    assert fused_residual.install_fused_residual(m, [_Q]) == 2
    for n in "ae":
        layer = getattr(m, n)
        assert "forward" in layer.__dict__ and "forward" in layer.self_attn.o_proj.__dict__ and "forward" in layer.mlp.down_proj.__dict__
        assert "forward" not in layer.self_attn.q_proj.__dict__ and "forward" not in layer.mlp.gate_proj.__dict__
    for n in "bcd":
        assert not any("forward" in mod.__dict__ or fused_residual._ARMED in mod.__dict__ for mod in getattr(m, n).modules()), n
    assert fused_residual.install_fused_residual(m, [_Q]) == 0      # already installed
    assert fused_residual.install_fused_residual(m, [_Q], layer_types=[GemmaDecoderLayer]) == 0   # not on fused_norm's list: still not patched
    with torch.no_grad():
        for n in "ace":
            assert torch.equal(getattr(m, n)(x), want[n]), n
    assert fused_residual.uninstall_fused_residual(m) == 2
    for q in (mod for mod in m.modules() if isinstance(mod, _Q)):
        q.own = before[[n for n, mod in m.named_modules() if mod is q][0]]["own"]   # (the test layer's own call counter)
    assert _dicts(m) == before
    assert fused_residual.uninstall_fused_residual(m) == 0
    # an instance forward that was there before comes back as it was
    mine = lambda hidden_states, **kw: hidden_states  # noqa: E731
    m.a.forward = mine
    down = m.a.mlp.down_proj
    own_swiglu = lambda gate, up: down(torch.nn.functional.silu(gate) * up) + 1  # noqa: E731
    down.forward_swiglu = own_swiglu                               # ... an instance forward_swiglu too, and it is what the wrapper falls back to
    assert fused_residual.install_fused_residual(m, [_Q], layer_types=["LlamaDecoderLayer"]) == 2
    assert m.a.forward is not mine and down.forward_swiglu is not own_swiglu
    g = _rnd(1, 32, seed=20)
    with torch.no_grad():
        assert torch.equal(down.forward_swiglu(g, g), own_swiglu(g, g))   # nothing armed
    fused_residual.uninstall_fused_residual(m)
    assert m.a.forward is mine and down.forward_swiglu is own_swiglu


def test_the_patched_forward_is_as_strict_about_its_arguments_as_the_class(monkeypatch):
    _fake_ops(monkeypatch)
    m = _model()
    x = _rnd(1, 1, 16, seed=21)
    fused_residual.install_fused_residual(m, [_Q])
    with torch.no_grad():
        with pytest.raises(TypeError):
            m.a(x, 0.5, 3)                                          # one positional argument too many
        with pytest.raises(TypeError):
            m.a(x, 0.5, scale=0.5)                                  # a parameter given twice
    o_slot, d_slot = m.a.__dict__[fused_residual._LAYER][1:3]
    assert o_slot.residual is None and d_slot.residual is None

    class KwOnly(torch.nn.Module):
        def forward(self, hidden_states: torch.Tensor, *, scale: float = 1.0, **kwargs) -> torch.Tensor:
            return hidden_states

    class VarArgs(torch.nn.Module):
        def forward(self, hidden_states: torch.Tensor, *rest, **kwargs) -> torch.Tensor:
            return hidden_states

    class NoDefault(torch.nn.Module):
        def forward(self, hidden_states: torch.Tensor, mask, **kwargs) -> torch.Tensor:
            return hidden_states

    assert all(fused_residual._signature_names(c) is None for c in (KwOnly, VarArgs, NoDefault, MistralDecoderLayer))
    assert fused_residual._signature_names(LlamaDecoderLayer) == {"scale": 1.0}


def test_the_armed_residual_is_consumed_once_and_the_fused_entries_are_reached(monkeypatch):
    calls = _fake_ops(monkeypatch)
    m = _model()
    x = _rnd(1, 1, 16, seed=10)
    x3 = _rnd(1, 3, 16, seed=11)
    with torch.no_grad():
        want, want3, want_scaled = m.a(x), m.a(x3), m.a(x, 0.5, flag=7)
        fused_residual.install_fused_residual(m, [_Q])
        got = m.a(x)
        assert calls["plain"] == 2 and calls["swiglu"] == 0          # o_proj and, behind the eager silu(g) * u, down_proj
        assert torch.equal(got, want)
        o_slot, d_slot = m.a.__dict__[fused_residual._LAYER][1:3]
        assert o_slot.residual is None and d_slot.residual is None and o_slot.consumed and d_slot.consumed
        own = m.a.self_attn.o_proj.own
        y = m.a.self_attn.o_proj(_rnd(1, 1, 32, seed=12))             # a call outside the layer: nothing armed, the layer's own forward
        assert calls["plain"] == 2 and m.a.self_attn.o_proj.own == own + 1 and y.shape == (1, 1, 16)
        # arguments reach self_attn as the class passes them: positional, keyword, defaults
        m.a(x, 0.5, flag=7)
        assert m.a.self_attn.seen == {"scale": 0.5, "flag": 7}
        m.a(x)
        assert m.a.self_attn.seen == {"scale": 1.0}
        assert torch.equal(m.a(x, 0.5, flag=7), want_scaled) and torch.equal(m.a(x, scale=0.5), want_scaled)
        # three rows: above the cap, the eager add inside the wrapper -- bit for bit, no fused call
        n = calls["plain"]
        assert torch.equal(m.a(x3), want3) and calls["plain"] == n
        # with the fused MLP installed the armed down_proj is reached through forward_swiglu
        assert fused_mlp.install_fused_mlp(m, [_Q]) == 5
        n = calls["plain"]
        got = m.a(x)
        assert calls["plain"] == n + 1 and calls["swiglu"] == 1 and calls["mlp"] == 0
        assert torch.equal(got, want)
        assert torch.equal(m.a(x3), want3) and calls["swiglu"] == 1 and calls["mlp"] == 0   # three rows: forward_swiglu's own rules (one row), then the add
        # install order: the MLP first, then the residual
        m2 = _model()
        fused_mlp.install_fused_mlp(m2, [_Q])
        fused_residual.install_fused_residual(m2, [_Q])
        s = calls["swiglu"]
        assert torch.equal(m2.a(x), want) and calls["swiglu"] == s + 1
        fused_mlp.uninstall_fused_mlp(m2)
        assert torch.equal(m2.a(x), want) and calls["swiglu"] == s + 1


def test_the_armed_residual_is_cleared_after_an_exception_and_added_when_nobody_took_it(monkeypatch):
    calls = _fake_ops(monkeypatch)
    m = _model()
    x = _rnd(1, 1, 16, seed=13)
    with torch.no_grad():
        m.a.self_attn.skip_o = True
        want_skip = m.a(x)
        m.a.self_attn.skip_o = False
        fused_residual.install_fused_residual(m, [_Q])
        o_slot, d_slot = m.a.__dict__[fused_residual._LAYER][1:3]
        m.a.self_attn.fail = True
        with pytest.raises(RuntimeError, match="attention failed"):
            m.a(x)
        assert o_slot.residual is None and d_slot.residual is None and calls["plain"] == 0
        m.a.self_attn.fail = False
        y = m.a.self_attn.o_proj(_rnd(1, 1, 32, seed=14))             # the next call of o_proj finds nothing armed
        assert calls["plain"] == 0 and y.shape == (1, 1, 16)
        # an attention that never calls o_proj: the layer adds the residual itself
        m.a.self_attn.skip_o = True
        assert torch.equal(m.a(x), want_skip)
        assert not o_slot.consumed and d_slot.consumed and calls["plain"] == 1   # (down_proj's only)
        # a leading shape that is not the q_layer's input: ignored, not consumed, disarmed
        o_slot.arm(_rnd(1, 2, 16, seed=15))
        m.a.self_attn.o_proj(_rnd(1, 1, 32, seed=16))
        assert not o_slot.consumed and o_slot.residual is None and calls["plain"] == 1


def test_composes_with_the_fused_norm_in_any_order(monkeypatch):
    _fake_ops(monkeypatch)
    x = _rnd(1, 1, 16, seed=17)
    outs = []
    for order in ((), ("norm", "resid"), ("resid", "norm")):
        m = _model()
        for layer in (m.a, m.e):
            fused.install_sibling_groups(layer, [_Q])
        for what in order:
            if what == "norm":
                fused_norm.install_fused_norm(m, [_Q])
            else:
                assert fused_residual.install_fused_residual(m, [_Q]) == 2
        with torch.no_grad():
            outs.append(m.a(x))                                      # (CPU: the norm's kernels do not apply, its original module computes)
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_the_environment_switch_makes_install_a_no_op(monkeypatch):
    monkeypatch.setenv("QLLM_FUSE_RESIDUAL", "0")
    m = _model()
    before = _dicts(m)
    assert fused_residual.install_fused_residual(m, [_Q]) == 0
    assert _dicts(m) == before


def test_load_quantized_keeps_the_fusion_opt_in():
    from qllm_amd.modeling import base, q_layers
    params = inspect.signature(base.load_quantized).parameters
    assert params["fuse_residual"].default is False
    assert q_layers.install_fused_residual is fused_residual.install_fused_residual
    assert q_layers.uninstall_fused_residual is fused_residual.uninstall_fused_residual


def test_the_installed_transformers_decoder_layers_meet_the_contract():
    """The three whitelisted classes of the installed release take hidden_states first and are annotated to return torch.Tensor."""
    from transformers.models.llama.modeling_llama import LlamaDecoderLayer as L
    from transformers.models.mistral.modeling_mistral import MistralDecoderLayer as M
    from transformers.models.qwen2.modeling_qwen2 import Qwen2DecoderLayer as Q2
    for cls in (L, M, Q2):
        d = fused_residual._signature_names(cls)
        assert d is not None and list(d)[:2] == ["attention_mask", "position_ids"], cls


# ---- resources ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src", ["strip1_resid.hip", "strip1_swiglu_resid.hip"])
def test_every_resid_instantiation_is_scratch_free_and_the_table_is_whole(src):
    """Every (NW, MAXS) pair of csrc/strip1_forms.hpp's table, in every one-row form of the plain family (strip1_families.py)."""
    check_family(src)


@pytest.mark.parametrize("src", ["strip1.hip", "strip1_swiglu.hip", "strip1_norm.hip"])
def test_the_existing_kernels_are_what_they_were(src):
    """The RESID constant must not leak into strip1_kernel / strip1_swiglu_kernel / strip1_norm_kernel: same kernels, same registers,
    spills, scratch and LDS as recorded from the commit before it existed (tests/golden/strip1_resources_before_residual.json)."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "strip1_resources_before_residual.json")))
    now = resources(src)
    assert sorted(now) == sorted(rec[src])
    for name, r in now.items():
        assert [r[f] for f in rec["fields"]] == rec[src][name], name
