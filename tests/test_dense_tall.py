"""ops.dense_tall and generate(step="tall") on CPU tensors: the explicit torch path, the default route's results."""
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2


@pytest.mark.parametrize("act", [None, "relu", "gelu"])
def test_dense_tall_on_cpu_is_linear_plus_activation(act):
    x, w, b = torch.randn(2, 40, 24), torch.randn(40, 24), torch.randn(40)
    ref = torch.nn.functional.linear(x, w, b)
    if act:
        ref = torch.relu(ref) if act == "relu" else torch.nn.functional.gelu(ref, approximate="tanh")
    torch.testing.assert_close(ops.dense_tall(x, w, b, act), ref, rtol=1e-5, atol=1e-5)


def test_generate_tall_on_cpu_returns_the_default_tokens_and_other_steps_raise():
    initializers.set_seed(0)
    with context.device("cpu"):
        model = GPT2(vocab=200, ctx=96, hidden=128, layers=2, heads=2)
        ids = torch.randint(0, 200, (20, 5))
        assert torch.equal(model.generate(ids, 6, step="tall"), model.generate(ids, 6))
        with pytest.raises(ValueError):
            model.generate(ids, 6, step="taller")
