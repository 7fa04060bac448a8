"""RMSNorm -- standalone (qllm_rmsnorm) and fused into the q/k/v and gate/up launches (qllm_linear_forward_rmsnorm) -- without a GPU: the
three additive C symbols (exported, declared, bound; ABI still 7), what qllm_rmsnorm_describe serves and refuses on hand-made native
descriptors (fake, aligned, never-dereferenced pointers), the argument checks of both entries, the host logic of install_fused_norm /
PreNorm / make_quant_norm against a fake `ops`, and the compiler's resource report: every NORM instantiation (csrc/strip1_norm.hip) free
of scratch and spills, and the kernels of strip1.hip / strip1_swiglu.hip exactly what they were before the NORM constant existed."""
import ctypes as C
import json
import os
import re

import pytest
import torch

from kernel_resources import resources
from qllm_amd import _lib, ops
from qllm_amd.modeling.q_layers import _hip_forward, fused, fused_norm
from strip1_families import check_family

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GPTQ, NATIVE, NATIVE_F16Z = _lib.LAYOUT_GPTQ, _lib.LAYOUT_NATIVE, _lib.LAYOUT_NATIVE_F16Z
NAMES = ("qllm_rmsnorm", "qllm_linear_forward_rmsnorm", "qllm_rmsnorm_describe")


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
    assert all(hasattr(ops, n) for n in ("rmsnorm", "linear_forward_rmsnorm", "rmsnorm_describe"))


# ---- what is served ----------------------------------------------------------------------------------------------------------------------
def test_describe_names_the_plain_grouped_calls_plan(lib):
    qkv = [W(4096)] * 3
    text = ops.rmsnorm_describe(qkv, 1)
    assert text.startswith("rmsnorm strip1 nw=8 round=16 exact"), text
    assert text == "rmsnorm " + ops.plan_describe(qkv, 1) and "grid=strips x 3" in text
    # one K per row of the batch-1 kernel's shape table, the two odd wave counts, one layer / two / three of different widths
    for K in (256, 1024, 2048, 4096, 6144, 8192, 12288, 16384, 18944, 20480, 24576, 28672, 32768, 3584, 11008):
        for group in ([W(K, 256)], [W(K, 256), W(K, 256)], [W(K, 512), W(K, 256), W(K, 256)], [W(K, 8192, layout=NATIVE_F16Z)] * 2):
            plan = ops.plan_describe(group, 1)
            assert plan.startswith("strip1 nw="), (K, plan)
            assert ops.rmsnorm_describe(group, 1) == "rmsnorm " + plan, (K, len(group))
    assert " nw=7 round=16 exact" in ops.rmsnorm_describe([W(3584, 8192)], 1)
    assert " nw=15 round=24 " in ops.rmsnorm_describe([W(11008, 256)] * 2, 1)
    # 64-wide groups (K % 128 == 64 too) and 3 bits
    for group, tag in (([W(5120, 256, g=64)] * 2, " g64 "), ([W(4544, 256, g=64)], " g64 "), ([W(5120, 256, bits=3)] * 2, " bits=3 "),
                       ([W(3584, 256, g=64, bits=3, layout=NATIVE_F16Z)], " g64 bits=3 ")):
        text = ops.rmsnorm_describe(group, 1)
        assert text == "rmsnorm " + ops.plan_describe(group, 1) and text.startswith("rmsnorm strip1 ") and tag in text, text


def test_refusals(lib):
    for group, m in (([W(4096)] * 3, 2),                                  # two rows: the four-row forms are not built
                     ([W(4096)], 4),
                     ([W(4096, layout=GPTQ)] * 2, 1),                     # a reference-layout descriptor
                     ([W(4096), W(4096, layout=GPTQ)], 1),
                     ([W(4096, bits=8, layout=GPTQ)], 1),                 # an 8-bit layer
                     ([W(4096, bits=8)], 1),
                     ([W(4096), W(2048)], 1),                             # members of different K
                     ([W(4096), W(4096, g=64)], 1),
                     ([W(4096, g=32)] * 2, 1),                            # 32-wide groups: not the batch-1 kernel's
                     ([W(192, g=64)], 1),                                 # K / 32 < 8 k-steps
                     ([W(65536)], 1)):                                    # beyond the shape table
        text = ops.rmsnorm_describe(group, m)
        assert text.startswith("refused: "), (m, [(w.K, w.bits, w.group_size, w.layout) for w in group], text)
    fake = C.c_void_p(4096)
    for group, m in (([W(4096)] * 3, 2), ([W(4096, layout=GPTQ)] * 2, 1), ([W(4096), W(2048)], 1)):   # the forward entry refuses the same
        n = len(group)
        ys = (C.c_void_p * n)(*[8192 + 65536 * i for i in range(n)])
        rc = lib.qllm_linear_forward_rmsnorm((_lib.QllmWeight * n)(*group), ys, n, fake, C.c_void_p(1 << 20), 1e-5, m, _lib.DT_F16, None, None)
        assert rc == _lib.QLLM_ERR_UNSUPPORTED and "fused RMSNorm" in _lib.last_error()


def test_a_knob_that_takes_the_shape_off_the_kernel_turns_the_answer_into_a_refusal(lib):
    group = [W(4096)] * 3
    assert ops.rmsnorm_describe(group, 1).startswith("rmsnorm strip1 ")
    try:
        ops.set_knob("QLLM_STRIP1", 0)
        assert ops.rmsnorm_describe(group, 1).startswith("refused: ")
        assert not ops.plan_describe(group, 1).startswith("strip1 ")
    finally:
        ops.reset_knobs()
    assert ops.rmsnorm_describe(group, 1).startswith("rmsnorm strip1 ")


def test_invalid_arguments_are_reported_before_any_device_work(lib):
    INV = _lib.QLLM_ERR_INVALID
    x, wn, y = C.c_void_p(4096), C.c_void_p(1 << 20), C.c_void_p(1 << 21)
    norm = lambda xx, ww, yy, m=1, k=4096, dt=_lib.DT_F16, r=None: lib.qllm_rmsnorm(xx, ww, yy, m, k, 1e-5, dt, r, None)  # noqa: E731
    assert norm(None, wn, y) == INV and "NULL" in _lib.last_error()
    assert norm(x, None, y) == INV and "NULL" in _lib.last_error()
    assert norm(x, wn, None) == INV and "NULL" in _lib.last_error()
    assert norm(x, wn, y, m=0) == INV and norm(x, wn, y, k=0) == INV
    assert norm(x, wn, y, k=4100) == INV and "multiple of 8" in _lib.last_error()
    assert norm(x, wn, y, dt=7) == INV and "act_dtype" in _lib.last_error()
    for bad in ((C.c_void_p(4104), wn, y), (x, C.c_void_p(4104), y), (x, wn, C.c_void_p(4104))):
        assert norm(*bad) == INV and "aligned" in _lib.last_error()
    assert norm(x, wn, y, r=C.c_void_p(4098)) == INV and "rstd_out" in _lib.last_error()
    assert norm(x, wn, y, k=65544) == _lib.QLLM_ERR_UNSUPPORTED and "65536" in _lib.last_error()

    group = [W(4096), W(4096)]
    arr = (_lib.QllmWeight * 2)(*group)
    ys = lambda a=1 << 21, b=1 << 22: (C.c_void_p * 2)(a, b)  # noqa: E731
    fwd = lambda yy, xx, ww, m=1, dt=_lib.DT_F16, r=None, a=arr, n=2: lib.qllm_linear_forward_rmsnorm(a, yy, n, xx, ww, 1e-5, m, dt, r, None)  # noqa: E731
    assert fwd(ys(), None, wn) == INV and "NULL" in _lib.last_error()
    assert fwd(ys(), x, None) == INV and "NULL" in _lib.last_error()
    assert fwd(None, x, wn) == INV and fwd(ys(), x, wn, a=None) == INV
    assert fwd(ys(None), x, wn) == INV and "NULL" in _lib.last_error()
    assert fwd(ys(), x, wn, m=0) == INV and "M must be" in _lib.last_error()
    assert fwd(ys(), x, wn, dt=7) == INV and "act_dtype" in _lib.last_error()
    assert fwd(ys(), C.c_void_p(4104), wn) == INV and "aligned" in _lib.last_error()
    assert fwd(ys(), x, C.c_void_p(4104)) == INV and "aligned" in _lib.last_error()
    assert fwd(ys(b=4096), x, wn) == INV and "alias" in _lib.last_error()            # a y aliasing x
    assert fwd(ys(a=1 << 20), x, wn) == INV and "alias" in _lib.last_error()         # ... or the norm's weight
    assert fwd(ys(), x, wn, r=C.c_void_p(4098)) == INV and "rstd_out" in _lib.last_error()
    assert fwd(ys(), x, wn, n=0) == INV and fwd(ys(), x, wn, n=9) == INV
    buf = C.create_string_buffer(768)
    assert lib.qllm_rmsnorm_describe(arr, 2, 0, buf, 768) == INV
    assert lib.qllm_rmsnorm_describe(None, 2, 1, buf, 768) == INV
    assert lib.qllm_rmsnorm_describe(arr, 0, 1, buf, 768) == INV


# ---- host logic against a fake `ops` and local classes of the whitelisted names ----------------------------------------------------------
class _Q(torch.nn.Module, _hip_forward.HipForwardMixin):
    """A q_layer as far as fused_norm and SiblingGroup look at it: forward(x) = x @ w, on any device."""
    act_order = None
    bits, groupsize = 4, 128

    def __init__(self, k, n, seed=0):
        super().__init__()
        self.infeatures, self.outfeatures = k, n
        self.w = torch.randn(k, n, generator=torch.Generator().manual_seed(seed + n)).half()
        self.seen = []

    def _layout_name(self):
        return "HQQ"

    def decode_descriptor(self, g_idx=None, add_zero_bias=0):
        return self

    def forward(self, x):
        self.seen.append(x)
        return (x.float() @ self.w.float()).to(x.dtype)


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


class GemmaRMSNorm(LlamaRMSNorm):
    pass


class NoEpsNorm(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(k).half())

    def forward(self, x):
        return x * self.weight


NoEpsNorm.__name__ = "LlamaRMSNorm"   # (the whitelisted name, but no variance_epsilon)


class LlamaAttention(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = _Q(k, 32, 1), _Q(k, 16, 2), _Q(k, 16, 3), _Q(32, k, 4)

    def forward(self, x):
        return self.o_proj(self.q_proj(x) * 0.01 + torch.cat([self.k_proj(x), self.v_proj(x)], -1) * 0.01)


class LlamaMLP(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _Q(k, 32, 5), _Q(k, 32, 6), _Q(32, k, 7)

    def forward(self, x):
        return self.down_proj(torch.nn.functional.silu(self.gate_proj(x) * 0.05) * self.up_proj(x) * 0.05)


class LlamaDecoderLayer(torch.nn.Module):
    def __init__(self, k=16, norm=LlamaRMSNorm):
        super().__init__()
        self.self_attn, self.mlp = LlamaAttention(k), LlamaMLP(k)
        self.input_layernorm, self.post_attention_layernorm = norm(k), norm(k)

    def forward(self, x):
        x = x + self.self_attn(self.input_layernorm(x))
        return x + self.mlp(self.post_attention_layernorm(x))


class GemmaDecoderLayer(LlamaDecoderLayer):
    pass


def _model():
    m = torch.nn.Module()
    m.a = LlamaDecoderLayer()
    m.b = GemmaDecoderLayer(norm=GemmaRMSNorm)                      # not on the list
    m.c = LlamaDecoderLayer()
    m.c.self_attn.k_proj = torch.nn.Linear(16, 16).half()          # k_proj is no q_layer: the attention pair is left alone, the MLP's is not
    m.d = LlamaDecoderLayer(norm=NoEpsNorm)                        # a norm without variance_epsilon
    m.norm = LlamaRMSNorm(16)                                      # the final norm: make_quant_norm's
    for layer in (m.a, m.b, m.c, m.d):
        fused.install_sibling_groups(layer, [_Q])
    return m


def _patched(mod):
    return "forward" in mod.__dict__


def _fake_ops(monkeypatch, refuse=False):
    """ops.rmsnorm / ops.linear_forward_rmsnorm computed by torch on whatever device, `_kernel_applies` without its device test."""
    calls = {"rmsnorm": 0, "fused": 0}

    def rmsnorm(x, weight, eps, out=None, return_rstd=False):
        calls["rmsnorm"] += 1
        h = x.float()
        return weight * (h * torch.rsqrt(h.pow(2).mean(-1, keepdim=True) + eps)).to(x.dtype)

    def fused_entry(descs, x2d, weight, eps, outs=None, return_rstd=False):
        calls["fused"] += 1
        if refuse:
            raise ops.QllmUnsupported(2, "fused RMSNorm: refused")
        xn = rmsnorm(x2d, weight, eps)
        calls["rmsnorm"] -= 1
        return [(xn.float() @ d.w.float()).to(x2d.dtype) for d in descs]

    monkeypatch.setattr(fused_norm.ops, "rmsnorm", rmsnorm)
    monkeypatch.setattr(fused_norm.ops, "linear_forward_rmsnorm", fused_entry)
    monkeypatch.setattr(fused_norm, "_kernel_applies", lambda x, w: x.dtype == w.dtype and not (torch.is_grad_enabled() and x.requires_grad))
    return calls


def test_install_patches_only_whitelisted_structurally_verified_layers_and_uninstall_restores():
    m = _model()
    before = {n: mod.__dict__.get("forward") for n, mod in m.named_modules()}
    keys = sorted(m.state_dict().keys())
    assert fused_norm.install_fused_norm(m, [_Q]) == 3              # a: both pairs; c: the MLP's only
    assert _patched(m.a.input_layernorm) and _patched(m.a.post_attention_layernorm)
    assert all(_patched(getattr(m.a.self_attn, n)) for n in ("q_proj", "k_proj", "v_proj")) and not _patched(m.a.self_attn.o_proj)
    assert _patched(m.a.mlp.gate_proj) and _patched(m.a.mlp.up_proj) and not _patched(m.a.mlp.down_proj)
    assert not any(_patched(mod) for mod in m.b.modules())          # Gemma: untouched
    assert not _patched(m.c.input_layernorm) and not _patched(m.c.self_attn.q_proj) and _patched(m.c.post_attention_layernorm)
    assert not any(_patched(mod) for mod in m.d.modules())          # no variance_epsilon: untouched
    assert not _patched(m.norm)
    assert sorted(m.state_dict().keys()) == keys                    # the norms stay in place
    assert m.a.self_attn.q_proj.__dict__[fused_norm._PRENORM][0] is m.a.self_attn.v_proj.__dict__[fused_norm._PRENORM][0]   # one PreNorm per pair
    assert fused_norm.install_fused_norm(m, [_Q]) == 0              # already installed
    assert fused_norm.make_quant_norm(m) == 2                       # m.norm and c's input_layernorm; Gemma's and the eps-less ones are not touched
    assert _patched(m.norm) and _patched(m.c.input_layernorm) and not _patched(m.b.input_layernorm) and not _patched(m.d.input_layernorm)
    assert fused_norm.uninstall_fused_norm(m) == 5
    assert {n: mod.__dict__.get("forward") for n, mod in m.named_modules()} == before
    assert not any(fused_norm._PRENORM in mod.__dict__ or fused_norm._ORIGINAL in mod.__dict__ for mod in m.modules())
    assert fused_norm.uninstall_fused_norm(m) == 0
    assert fused_norm.install_fused_norm(m, [_Q], layer_types=[GemmaDecoderLayer]) == 0   # listed, but its norm class is not: still not guessed at


def test_a_refused_group_computes_what_the_unpatched_layer_computes_and_is_asked_once(monkeypatch):
    calls = _fake_ops(monkeypatch, refuse=True)
    m = _model()
    x = torch.randn(1, 1, 16, generator=torch.Generator().manual_seed(1)).half()
    x3 = torch.randn(1, 3, 16, generator=torch.Generator().manual_seed(2)).half()
    with torch.no_grad():
        want, want3 = m.a(x), m.a(x3)
        assert fused_norm.install_fused_norm(m, [_Q]) == 3
        assert torch.equal(m.a(x.clone()), want)
        assert calls["fused"] == 2                                  # one attempt per pair ...
        pre = m.a.self_attn.q_proj.__dict__[fused_norm._PRENORM][0]
        assert pre.refused and m.a.mlp.up_proj.__dict__[fused_norm._PRENORM][0].refused
        assert torch.equal(m.a(x.clone()), want) and torch.equal(m.a(x3), want3)
        assert calls["fused"] == 2                                  # ... remembered
        assert calls["rmsnorm"] == 6                                # one norm kernel per pair and forward, shared by the siblings
    # CPU tensors as they are (the kernels do not apply): the original module computes the norm, bit for bit the unpatched layer
    monkeypatch.undo()
    with torch.no_grad():
        assert torch.equal(m.a(x), want) and torch.equal(m.a(x3), want3)


def test_the_fused_launch_serves_one_row_and_parks_the_siblings(monkeypatch):
    calls = _fake_ops(monkeypatch)
    m = _model()
    x = torch.randn(1, 1, 16, generator=torch.Generator().manual_seed(3)).half()
    x2 = torch.randn(1, 2, 16, generator=torch.Generator().manual_seed(4)).half()
    with torch.no_grad():
        want, want2 = m.a(x), m.a(x2)
        fused_norm.install_fused_norm(m, [_Q])
        g = m.a.self_attn.q_proj._siblings
        n0 = g.grouped_launches
        assert torch.equal(m.a(x), want)
        assert calls == {"rmsnorm": 0, "fused": 2} and g.grouped_launches == n0 + 1 and not g._parked   # one launch per norm, outputs consumed
        assert torch.equal(m.a(x2), want2) and calls["fused"] == 2 and calls["rmsnorm"] == 2           # two rows: the standalone kernel
        # only q_proj, or v_proj first: the same values
        attn = m.a.self_attn
        q = attn.q_proj(x)
        v_first = attn.v_proj(x.clone())
        xx = x.clone()
        v, k, q2 = attn.v_proj(xx), attn.k_proj(xx), attn.q_proj(xx)
        assert torch.equal(q, q2) and torch.equal(v, v_first)
        fused_norm.uninstall_fused_norm(m)
        xn = m.a.input_layernorm(x)
        assert torch.equal(q, attn.q_proj(xn)) and torch.equal(v, attn.v_proj(xn)) and torch.equal(k, attn.k_proj(xn))
    # grad mode with an input to differentiate, a group switched off, max rows 0: not sent to the fused entry
    fused_norm.install_fused_norm(m, [_Q])
    n = calls["fused"]
    m.a.self_attn.q_proj(x.clone().float().requires_grad_().half())
    assert calls["fused"] == n
    with torch.no_grad():
        m.a.self_attn.q_proj._siblings.enabled = False
        m.a.self_attn.q_proj(x.clone())
        assert calls["fused"] == n
        monkeypatch.setattr(fused_norm.PreNorm, "norm_max_m", 0)
        m.a.mlp.gate_proj(x.clone())
        assert calls["fused"] == n


def test_prenorm_apply_hands_out_one_tensor_per_input_version(monkeypatch):
    _fake_ops(monkeypatch)
    m = _model()
    fused_norm.install_fused_norm(m, [_Q])
    pre = m.a.self_attn.q_proj.__dict__[fused_norm._PRENORM][0]
    x = torch.randn(2, 16).half()
    with torch.no_grad():
        a = pre.apply(x)
        assert pre.apply(x) is a
        x.mul_(2)                                                   # in place: a new version, a new result
        b = pre.apply(x)
        assert b is not a and pre.apply(x) is b
        assert pre.apply(x.clone()) is not b
        assert pre._x() is None or pre._x() is not x                # (held weakly: the clone above is gone)


def test_make_quant_norm_runs_the_kernel_where_it_applies(monkeypatch):
    calls = _fake_ops(monkeypatch)
    m = _model()
    x = torch.randn(3, 16).half()
    with torch.no_grad():
        want = m.norm(x)
        assert fused_norm.make_quant_norm(m) == 5                   # every whitelisted norm with an epsilon: a's two, c's two, m.norm -- not b's, not d's
        assert torch.equal(m.norm(x), want) and calls["rmsnorm"] == 1
        assert m.norm(x.float()).dtype == torch.float32 and calls["rmsnorm"] == 1      # fp32 input against fp16 weight: the original forward


def test_the_environment_switch_makes_install_a_no_op(monkeypatch):
    monkeypatch.setenv("QLLM_FUSE_NORM", "0")
    m = _model()
    assert fused_norm.install_fused_norm(m, [_Q]) == 0 and fused_norm.make_quant_norm(m) == 0
    assert not any(_patched(mod) for mod in m.modules())


def test_load_quantized_keeps_the_fusion_opt_in():
    import inspect
    from qllm_amd.modeling import base
    params = inspect.signature(base.load_quantized).parameters
    assert params["fuse_norm"].default is False and params["fuse_mlp"].default is False
    assert isinstance(fused_norm.PreNorm.norm_max_m, int)


# ---- resources ---------------------------------------------------------------------------------------------------------------------------
def test_every_norm_instantiation_is_scratch_free_and_the_table_is_whole():
    """Every (NW, MAXS) pair of csrc/strip1_forms.hpp's table, in every one-row form of the plain family (strip1_families.py)."""
    check_family("strip1_norm.hip")
    for n, r in resources("rmsnorm.hip").items():                                 # the standalone kernel's forms
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (n, r)


@pytest.mark.parametrize("src", ["strip1.hip", "strip1_swiglu.hip"])
def test_the_existing_kernels_are_what_they_were(src):
    """The NORM constant must not leak into strip1_kernel / strip1_swiglu_kernel: same kernels, same registers, spills, scratch and LDS as
    recorded from the commit before it existed (tests/golden/strip1_resources_before_norm.json)."""
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "strip1_resources_before_norm.json")))
    now = resources(src)
    assert sorted(now) == sorted(rec[src])
    for name, r in now.items():
        assert [r[f] for f in rec["fields"]] == rec[src][name], name
