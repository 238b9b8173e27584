"""generate(step="fused") on the CPU reference path (f32): the same composition in the same order, so the same tokens."""
import pytest
import torch

from distributed_tensorflow_amd import context
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2


def test_fused_step_gives_the_default_tokens_on_the_cpu():
    with context.device("cpu"):
        initializers.set_seed(0)
        model = GPT2(vocab=200, ctx=96, hidden=128, layers=2, heads=2)
        ids = torch.arange(10).reshape(2, 5) * 7 % 200
        want = model.generate(ids, 12)
        assert torch.equal(model.generate(ids, 12, step="fused"), want)
        assert torch.equal(model.generate(ids, 12, step="fused", sampler="fused", prefill_chunk=2), want)
        with pytest.raises(ValueError):
            model.generate(ids, 1, step="persistent")
