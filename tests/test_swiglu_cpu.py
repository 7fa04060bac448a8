"""The fused SwiGLU down-projection without a GPU: the two additive C symbols (exported, declared, bound; ABI still 7), what
qllm_swiglu_describe serves and refuses on hand-made native descriptors (fake, aligned, never-dereferenced pointers), the argument checks
of qllm_linear_forward_swiglu, the host logic of install_fused_mlp / forward_swiglu against a fake `ops`, and the compiler's resource
report for every SWIGLU instantiation (csrc/strip1_swiglu.hip)."""
import ctypes as C
import os
import re

import pytest
import torch

from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import _hip_forward, fused_mlp
from strip1_families import check_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPTQ, NATIVE, NATIVE_F16Z = _lib.LAYOUT_GPTQ, _lib.LAYOUT_NATIVE, _lib.LAYOUT_NATIVE_F16Z


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
    for name in ("qllm_linear_forward_swiglu", "qllm_swiglu_describe"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.EXPORTS
        assert C.cast(getattr(lib, name), C.c_void_p).value
        assert getattr(lib, name).argtypes is not None
    assert re.search(r"#define\s+QLLM_ACT_SILU\s+0\b", header) and _lib.ACT_SILU == 0
    assert lib.qllm_abi_version() == 7 == _lib.ABI_VERSION


# ---- what is served ----------------------------------------------------------------------------------------------------------------------
# one K per row of strip1_shape's table (csrc/strip1.hip), and the two odd wave counts
TABLE_K = (1024, 2048, 4096, 6144, 8192, 12288, 16384, 20480, 24576, 28672, 32768, 3584, 11008)


@pytest.mark.parametrize("K", TABLE_K)
def test_describe_names_the_plain_calls_plan(lib, K):
    for N in (256, 8192):   # at most one strip per CU / more strips than CUs: K <= 4096 has a form for each
        for w in (W(K, N), W(K, N, layout=NATIVE_F16Z)):
            for m in (1, 4):
                plan = ops.plan_describe([w], m)
                text = ops.swiglu_describe(w, m)
                if m == 4 and K > 16384:
                    assert not plan.startswith("strip1 ") and text.startswith("refused: "), (K, N, m, plan, text)
                    continue
                assert plan.startswith("strip1 nw="), (K, N, m, plan)
                assert text == "swiglu " + plan, (K, N, m)
                assert ("exact" in text) != (" grid=strips" in text and "exact" not in text)
                assert (" rows=4 " in text) == (m == 4)
    # 64-wide groups and 3 bits at one row
    for w, tag in ((W(K, g=64), " g64 "), (W(K, bits=3), " bits=3 "), (W(K, g=64, bits=3, layout=NATIVE_F16Z), " g64 bits=3 ")):
        plan = ops.plan_describe([w], 1)
        if plan.startswith("strip1 "):
            assert ops.swiglu_describe(w, 1) == "swiglu " + plan and tag in plan
        else:   # (beyond the form's K: 24576 with 64-wide groups, 16384 with 3 bits)
            assert K > 16384 and ops.swiglu_describe(w, 1).startswith("refused: ")


def test_refusals(lib):
    for w, m in ((W(4096, layout=GPTQ), 1),        # the reference layout
                 (W(4096), 5),                     # five rows
                 (W(4096, g=64), 2),               # 64-wide groups at two rows
                 (W(4096, bits=3), 2),             # 3 bits at two rows
                 (W(4096, bits=8, layout=GPTQ), 1),
                 (W(4096, bits=8), 1),             # (the native layout does not hold 8 bits at all)
                 (W(192, g=64), 1)):               # K / 32 < 8 k-steps
        text = ops.swiglu_describe(w, m)
        assert text.startswith("refused: "), (w.K, w.bits, w.group_size, w.layout, m, text)
    fake = C.c_void_p(4096)
    w = W(4096)
    assert ops.swiglu_describe(w, 1).startswith("swiglu strip1 ")
    rc = lib.qllm_linear_forward_swiglu(C.byref(w), fake, fake, C.c_void_p(8192), 1, _lib.DT_F16, 1, None)   # act = 1: not SiLU
    assert rc == _lib.QLLM_ERR_UNSUPPORTED and "act=1" in _lib.last_error()
    for ww, m in ((W(4096, layout=GPTQ), 1), (W(4096), 5), (W(4096, g=64), 2)):   # the forward entry refuses the same, before any device work
        rc = lib.qllm_linear_forward_swiglu(C.byref(ww), fake, fake, C.c_void_p(8192), m, _lib.DT_F16, _lib.ACT_SILU, None)
        assert rc == _lib.QLLM_ERR_UNSUPPORTED and "fused SwiGLU" in _lib.last_error()


def test_a_knob_that_takes_the_shape_off_the_kernel_turns_the_answer_into_a_refusal(lib):
    w = W(11008)
    assert ops.swiglu_describe(w, 1) == "swiglu strip1 nw=15 round=24 grid=strips x 1 layout=strip-major"
    try:
        ops.set_knob("QLLM_STRIP1", 0)
        assert ops.swiglu_describe(w, 1).startswith("refused: ")
        assert ops.swiglu_describe(w, 4).startswith("refused: ")
    finally:
        ops.reset_knobs()
    assert ops.swiglu_describe(w, 1).startswith("swiglu strip1 ")
    try:
        ops.set_knob("QLLM_STRIP1_MAX_M", 1)
        assert ops.swiglu_describe(w, 4).startswith("refused: ") and ops.swiglu_describe(w, 1).startswith("swiglu ")
    finally:
        ops.reset_knobs()


def test_invalid_arguments_are_reported_before_any_device_work(lib):
    w = W(4096)
    fake, y = C.c_void_p(4096), C.c_void_p(8192)
    call = lambda g, u, yy, m, dt=_lib.DT_F16: lib.qllm_linear_forward_swiglu(C.byref(w), g, u, yy, m, dt, _lib.ACT_SILU, None)  # noqa: E731
    assert call(None, fake, y, 1) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error()
    assert call(fake, None, y, 1) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error()
    assert call(fake, fake, None, 1) == _lib.QLLM_ERR_INVALID and "NULL" in _lib.last_error()
    assert call(fake, fake, y, 0) == _lib.QLLM_ERR_INVALID and "M must be" in _lib.last_error()
    assert call(fake, fake, y, 1, 7) == _lib.QLLM_ERR_INVALID and "act_dtype" in _lib.last_error()
    assert call(C.c_void_p(4104), fake, y, 1) == _lib.QLLM_ERR_INVALID and "aligned" in _lib.last_error()
    assert call(fake, C.c_void_p(4104), y, 1) == _lib.QLLM_ERR_INVALID and "aligned" in _lib.last_error()
    assert call(fake, fake, fake, 1) == _lib.QLLM_ERR_INVALID and "alias" in _lib.last_error()
    assert lib.qllm_linear_forward_swiglu(None, fake, fake, y, 1, _lib.DT_F16, 0, None) == _lib.QLLM_ERR_INVALID
    buf = C.create_string_buffer(640)
    assert lib.qllm_swiglu_describe(C.byref(w), 0, buf, 640) == _lib.QLLM_ERR_INVALID
    assert lib.qllm_swiglu_describe(None, 1, buf, 640) == _lib.QLLM_ERR_INVALID


# ---- host logic against a fake `ops` -----------------------------------------------------------------------------------------------------
class _Q(torch.nn.Module, _hip_forward.HipForwardMixin):
    """A q_layer as far as forward_swiglu looks at it."""
    act_order = None

    def __init__(self, k, n, native=True):
        super().__init__()
        self.infeatures, self.outfeatures, self.native = k, n, native
        self.own = []

    def _layout_name(self):
        return "HQQ"

    def native_descriptor(self, add_zero_bias=0):
        return ("native", self.outfeatures) if self.native else None

    def forward(self, x):
        self.own.append(x)
        return x[..., :1].expand(x.shape[:-1] + (self.outfeatures,)) * 0 + 7.0


def _fake_ops(monkeypatch, refuse_from):
    calls = []

    def fake(w, g2d, u2d, out=None):
        calls.append(g2d.shape[0])
        if g2d.shape[0] >= refuse_from:
            raise ops.QllmUnsupported(2, "fused SwiGLU: not this many rows")
        return torch.full((g2d.shape[0], w[1]), 3.0)

    monkeypatch.setattr(_hip_forward.ops, "linear_forward_swiglu", fake)
    return calls


def test_forward_swiglu_remembers_a_refusal_and_falls_back_to_the_layers_own_forward(monkeypatch):
    calls = _fake_ops(monkeypatch, refuse_from=5)
    rnd = lambda *shape: torch.randn(*shape).half()  # noqa: E731
    q = _Q(16, 8)
    q.swiglu_max_m = 64                                            # (the modules' measured cutoff is one row: not what is tested here)
    g1, u1 = rnd(1, 1, 16), rnd(1, 1, 16)
    y = q.forward_swiglu(g1, u1)
    assert y.shape == (1, 1, 8) and float(y[0, 0, 0]) == 3.0 and calls == [1] and not q.own
    g6, u6 = rnd(2, 3, 16), rnd(2, 3, 16)
    y = q.forward_swiglu(g6, u6)                                   # six rows: asked once, refused, the path of today
    assert calls == [1, 6] and y.shape == (2, 3, 8) and float(y[0, 0, 0]) == 7.0
    assert len(q.own) == 1 and torch.equal(q.own[0], torch.nn.functional.silu(g6) * u6)
    q.forward_swiglu(g6, u6)
    q.forward_swiglu(rnd(8, 16), rnd(8, 16))
    assert calls == [1, 6] and len(q.own) == 3                     # remembered: nothing from six rows up is asked again
    assert float(q.forward_swiglu(rnd(4, 16), rnd(4, 16))[0, 0]) == 3.0 and calls == [1, 6, 4]   # smaller still tries
    q.forward_swiglu(rnd(5, 16), rnd(5, 16))
    assert calls == [1, 6, 4, 5] and q._swiglu_refused_from == 5
    q.forward_swiglu(rnd(5, 16), rnd(5, 16))
    assert calls == [1, 6, 4, 5]
    q._invalidate()                                                # new buffers: asked again
    assert q._swiglu_refused_from > 5


def test_forward_swiglu_does_not_try_what_the_entry_cannot_take(monkeypatch):
    calls = _fake_ops(monkeypatch, refuse_from=10 ** 9)
    g, u = torch.randn(1, 16).half(), torch.randn(1, 16).half()
    assert float(_Q(16, 8, native=False).forward_swiglu(g, u)[0, 0]) == 7.0          # no native copy
    ao = _Q(16, 8)
    ao.act_order = True
    assert float(ao.forward_swiglu(g, u)[0, 0]) == 7.0                                # act-order
    q = _Q(16, 8)
    assert float(q.forward_swiglu(g, u.double())[0, 0]) == 7.0                        # dtypes disagree
    assert float(q.forward_swiglu(torch.randn(16, 2).half().t()[:1], u)[0, 0]) == 7.0        # not contiguous
    assert float(q.forward_swiglu(g.float(), u.float())[0, 0]) == 7.0 and calls == []  # not an activation type of the kernels
    assert float(q.forward_swiglu(g, u)[0, 0]) == 3.0 and calls == [1]
    assert q.swiglu_max_m == 1                                                        # the measured cutoff: two rows are not sent
    g2 = torch.randn(2, 16).half()
    assert float(q.forward_swiglu(g2, g2.clone())[0, 0]) == 7.0 and calls == [1]


class LlamaMLP(torch.nn.Module):
    def __init__(self, act=None, down=None, up=None):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _Q(16, 32), (up or _Q(16, 32)), (down or _Q(32, 16))
        self.act_fn = torch.nn.SiLU() if act is None else act

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class Qwen2MLP(LlamaMLP):
    pass


class GemmaMLP(LlamaMLP):
    pass


def _model():
    m = torch.nn.Module()
    m.a = LlamaMLP()
    m.b = Qwen2MLP(act=torch.nn.functional.silu)
    m.c = LlamaMLP(act=torch.nn.GELU())                              # not SiLU
    m.d = LlamaMLP(down=torch.nn.Linear(32, 16))                     # down_proj is no q_layer
    m.e = GemmaMLP()                                                 # not on the list
    m.f = LlamaMLP(up=torch.nn.Linear(16, 32))
    from transformers.activations import ACT2FN
    m.g = LlamaMLP(act=ACT2FN["silu"])                               # what transformers puts into a LlamaMLP
    return m


def test_install_patches_only_whitelisted_silu_mlps_of_three_q_layers(monkeypatch):
    calls = _fake_ops(monkeypatch, refuse_from=10 ** 9)
    m = _model()
    x = torch.randn(1, 16).half()
    assert float(m.a(x)[0, 0]) == 7.0 and calls == []
    assert fused_mlp.install_fused_mlp(m, [_Q]) == 3
    assert all("forward" in getattr(m, n).__dict__ for n in "abg")
    assert all("forward" not in getattr(m, n).__dict__ for n in "cdef")
    assert float(m.a(x)[0, 0]) == 3.0 and float(m.b(x)[0, 0]) == 3.0 and calls == [1, 1]
    assert float(m.c(x)[0, 0]) == 7.0 and float(m.e(x)[0, 0]) == 7.0 and calls == [1, 1]
    assert fused_mlp.install_fused_mlp(m, [_Q]) == 0                 # already installed: nothing to do
    assert fused_mlp.install_fused_mlp(m, [_Q], mlp_types=[GemmaMLP, "NoSuchMLP"]) == 1 and float(m.e(x)[0, 0]) == 3.0
    assert fused_mlp.uninstall_fused_mlp(m) == 4
    assert all("forward" not in getattr(m, n).__dict__ for n in "abcdefg")
    assert float(m.a(x)[0, 0]) == 7.0 and float(m.e(x)[0, 0]) == 7.0 and len(calls) == 3
    assert fused_mlp.uninstall_fused_mlp(m) == 0


def test_the_environment_switch_makes_install_a_no_op(monkeypatch):
    monkeypatch.setenv("QLLM_FUSE_MLP", "0")
    m = _model()
    assert fused_mlp.install_fused_mlp(m, [_Q]) == 0 and "forward" not in m.a.__dict__


def test_load_quantized_keeps_the_fusion_opt_in():
    import inspect
    from qllm_amd.modeling import base
    assert inspect.signature(base.load_quantized).parameters["fuse_mlp"].default is False


# ---- resources ---------------------------------------------------------------------------------------------------------------------------
def test_every_swiglu_instantiation_is_scratch_free_and_the_table_is_whole():
    """Every (NW, MAXS) pair of csrc/strip1_forms.hpp's table, in every form of the plain family, four-row forms included (strip1_families.py)."""
    check_family("strip1_swiglu.hip")
