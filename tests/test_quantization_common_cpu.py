"""quantization/_common.py: capturing what a model hands its first decoder block, on a toy model (no GPU, no library)."""
import pytest
import torch

from qllm_amd.quantization._common import capture_first_block_inputs, decoder_blocks


class _Block(torch.nn.Module):
    def forward(self, hidden, scale, shift=0.0, use_cache=None):
        return hidden * scale + shift


class _Toy(torch.nn.Module):
    def __init__(self, fail_at=None, reach=True):
        super().__init__()
        self.embed = torch.nn.Embedding(16, 4)
        self.layers = torch.nn.ModuleList([_Block(), _Block()])
        self.fail_at, self.reach, self.calls = fail_at, reach, 0

    def forward(self, ids, use_cache=True):
        self.calls += 1
        if self.calls == self.fail_at:
            raise KeyError("the model's own failure")
        hidden = self.embed(ids)
        if self.reach:
            for block in self.layers:
                hidden = block(hidden, 2.0, shift=1.0, use_cache=use_cache)
        return hidden


IDS = torch.arange(15).view(3, 5)


def test_one_input_per_calibration_row_with_the_args_and_kwargs():
    model = _Toy()
    prefix, blocks = decoder_blocks(model)
    assert prefix == "layers" and blocks is model.layers
    original = list(blocks)
    inps, args, kwargs = capture_first_block_inputs(model, blocks, IDS, "cpu")
    assert len(inps) == 3 and all(tuple(x.shape) == (1, 5, 4) for x in inps)
    for j, x in enumerate(inps):
        assert torch.equal(x, model.embed(IDS[j:j + 1]))
    assert args == (2.0,) and kwargs == {"shift": 1.0, "use_cache": False}
    assert len(blocks) == 2 and all(a is b for a, b in zip(blocks, original))


def test_the_blocks_are_back_when_the_forward_raises_something_else():
    model = _Toy(fail_at=2)
    _, blocks = decoder_blocks(model)
    original = list(blocks)
    with pytest.raises(KeyError, match="own failure"):
        capture_first_block_inputs(model, blocks, IDS, "cpu")
    assert len(blocks) == 2 and all(a is b for a, b in zip(blocks, original))


def test_a_forward_that_never_reaches_the_blocks_is_an_error():
    model = _Toy(reach=False)
    _, blocks = decoder_blocks(model)
    original = list(blocks)
    with pytest.raises(RuntimeError, match="the decoder blocks were not reached"):
        capture_first_block_inputs(model, blocks, IDS, "cpu")
    assert all(a is b for a, b in zip(blocks, original))
