"""The five opt-in installs of q_layers (fused MLP, norm, residual, rope, attention) against one fake Llama-shaped model, without a GPU:
install -> uninstall is an exact round trip in every install order, uninstalled in the reverse and in the same order -- every module's
`__dict__` holds exactly the keys it held, an instance forward that was there before is the same object again -- and an install on top
of itself patches nothing.  What the patched forwards compute is the business of each fusion's own file; nothing is called here."""
import itertools

import pytest
import torch

from qllm_amd.modeling.q_layers import (_hip_forward, fused, install_fused_attention, install_fused_mlp, install_fused_norm,
                                        install_fused_residual, install_fused_rope, uninstall_fused_attention, uninstall_fused_mlp,
                                        uninstall_fused_norm, uninstall_fused_residual, uninstall_fused_rope)


# the three globals fused_rope's restated attention forward looks up in the module of the attention class
def apply_rotary_pos_emb(q, k, cos, sin, unsqueeze_dim=1):
    return q, k


def eager_attention_forward(module, query, key, value, attention_mask, **kwargs):
    return value.transpose(1, 2), None


class ALL_ATTENTION_FUNCTIONS:
    @staticmethod
    def get_interface(name, default):
        return default


class _Q(torch.nn.Module, _hip_forward.HipForwardMixin):
    """A q_layer as far as the installs look at it."""
    act_order = None
    bits, groupsize = 4, 128

    def __init__(self, k, n):
        super().__init__()
        self.infeatures, self.outfeatures = k, n

    def _layout_name(self):
        return "HQQ"

    def decode_descriptor(self, g_idx=None, add_zero_bias=0):
        return self

    def forward(self, x):
        return x.new_zeros(x.shape[:-1] + (self.outfeatures,))


class LlamaRMSNorm(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.weight = torch.nn.Parameter(torch.ones(k).half())
        self.variance_epsilon = 1e-5

    def forward(self, hidden_states):
        return hidden_states * self.weight


class LlamaAttention(torch.nn.Module):
    def __init__(self, k, layer_idx):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = _Q(k, k), _Q(k, k // 2), _Q(k, k // 2), _Q(k, k)
        self.head_dim, self.layer_idx, self.config, self.scaling, self.attention_dropout = 8, layer_idx, None, 8 ** -0.5, 0.0

    def forward(self, hidden_states, position_embeddings=None, attention_mask=None, past_key_values=None, **kwargs):
        return self.o_proj(self.q_proj(hidden_states)), None


class LlamaMLP(torch.nn.Module):
    def __init__(self, k):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _Q(k, 2 * k), _Q(k, 2 * k), _Q(2 * k, k)
        self.act_fn = torch.nn.SiLU()

    def forward(self, x):
        return self.down_proj(self.act_fn(self.gate_proj(x)) * self.up_proj(x))


class LlamaDecoderLayer(torch.nn.Module):
    def __init__(self, layer_idx, k=16):
        super().__init__()
        self.self_attn, self.mlp = LlamaAttention(k, layer_idx), LlamaMLP(k)
        self.input_layernorm, self.post_attention_layernorm = LlamaRMSNorm(k), LlamaRMSNorm(k)

    def forward(self, hidden_states: torch.Tensor, attention_mask=None, **kwargs) -> torch.Tensor:
        hidden_states = hidden_states + self.self_attn(self.input_layernorm(hidden_states), attention_mask=attention_mask, **kwargs)[0]
        return hidden_states + self.mlp(self.post_attention_layernorm(hidden_states))


INSTALLS = {   # name: (install, uninstall, how many modules of the two-layer model either counts)
    "mlp": (lambda m: install_fused_mlp(m, [_Q]), uninstall_fused_mlp, 2),
    "norm": (lambda m: install_fused_norm(m, [_Q]), uninstall_fused_norm, 4),
    "residual": (lambda m: install_fused_residual(m, [_Q]), uninstall_fused_residual, 2),
    "rope": (install_fused_rope, uninstall_fused_rope, 2),
    "attention": (install_fused_attention, uninstall_fused_attention, 2),
}


def _model():
    """Two decoder layers with their sibling groups.  Every module of the first that an install patches already has an instance forward
    of its own (down_proj an instance forward_swiglu too); the second has none.  -> (model, {(module, attribute name): what was set})."""
    m = torch.nn.Module()
    m.layers = torch.nn.ModuleList([LlamaDecoderLayer(0), LlamaDecoderLayer(1)])
    assert fused.install_sibling_groups(m, [_Q]) == 4
    first = m.layers[0]
    preset = {}
    for mod in (first, first.self_attn, first.mlp, first.input_layernorm, first.post_attention_layernorm, first.self_attn.q_proj,
                first.self_attn.o_proj, first.mlp.gate_proj, first.mlp.down_proj):
        preset[mod, "forward"] = mod.forward = lambda *a, _cls_forward=type(mod).forward, _mod=mod, **kw: _cls_forward(_mod, *a, **kw)
    down = first.mlp.down_proj
    preset[down, "forward_swiglu"] = down.forward_swiglu = lambda gate, up, _down=down: _down(torch.nn.functional.silu(gate) * up)
    return m, preset


@pytest.mark.parametrize("uninstall_order", ["reverse", "same"])
def test_install_then_uninstall_is_an_exact_round_trip_in_every_order(uninstall_order):
    m, preset = _model()      # ONE model through all 120 orders: a round trip that left anything behind would meet the next one
    keys = {name: set(mod.__dict__) for name, mod in m.named_modules()}
    orders = list(itertools.permutations(INSTALLS))
    assert len(orders) == 120
    for order in orders:
        for name in order:
            install, _, count = INSTALLS[name]
            assert install(m) == count, (order, name)
            assert install(m) == 0, (order, name)               # already in place: nothing is patched twice
        assert all(mod.__dict__[attr] is not had for (mod, attr), had in preset.items()), order
        assert all("forward" in layer.__dict__ and "forward" in layer.self_attn.__dict__ and "forward" in layer.mlp.__dict__ for layer in m.layers)
        for name in (reversed(order) if uninstall_order == "reverse" else order):
            _, uninstall, count = INSTALLS[name]
            assert uninstall(m) == count, (order, name)
        assert {name: set(mod.__dict__) for name, mod in m.named_modules()} == keys, order
        assert all(mod.__dict__[attr] is had for (mod, attr), had in preset.items()), order
    assert all(uninstall(m) == 0 for _, uninstall, _ in INSTALLS.values())
