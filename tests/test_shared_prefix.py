"""generate(num_return_sequences=G) and KVCache.fork on the CPU: the forked route equals repeated prompts exactly."""
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2


@pytest.fixture(scope="module")
def model():
    with context.device("cpu"):
        initializers.set_seed(0)
        torch.manual_seed(0)
        return GPT2(vocab=200, ctx=96, hidden=128, layers=2, heads=2)


def test_samples_equal_repeated_prompts(model):
    torch.manual_seed(1)
    ids = torch.randint(1, 200, (2, 6))
    kw = dict(prompt_lens=torch.tensor([6, 4]), temperature=0.8, top_k=8, seed=1, sampler="fused")
    with context.device("cpu"):
        a = model.generate(ids, 7, num_return_sequences=3, **kw)
        cache = model.last_generation["cache"]
        b = model.generate(ids.repeat_interleave(3, 0), 7, prompt_lens=kw.pop("prompt_lens").repeat_interleave(3), **kw)
    assert tuple(a.shape) == (6, 13) and torch.equal(a, b)
    assert len({tuple(r) for r in a[:3].tolist()}) > 1, "the samples of one prompt are all the same"
    assert cache.group == 3 and cache.batch == 6 and cache.lens.tolist() == [13] * 3 + [11] * 3
    assert cache.plens.tolist() == [6, 4]


def test_refusals(model):
    ids = torch.randint(1, 200, (2, 4))
    with context.device("cpu"):
        model.generate(ids, 2)
        filled = model.last_generation["cache"]
        for kw in (dict(cache=filled), dict(prefill_chunk=2), dict(step="fused"), dict(kv_dtype="fp8")):
            with pytest.raises(ValueError):
                model.generate(ids, 2, num_return_sequences=2, **kw)
        with pytest.raises(ValueError):
            model.generate(ids, 2, num_return_sequences=17)
        fork = filled.fork(2)
        qkv = torch.randn(4, 2, 3 * 128)
        with pytest.raises(ValueError):
            fork.attend(0, qkv[:, :1], fused=True)
        with pytest.raises(ValueError):
            fork.attend_chunk(0, qkv)
        for G in (1, 17):
            with pytest.raises(ValueError):
                filled.fork(G)
        with pytest.raises(ValueError):
            model.new_cache(2, 8, "cpu").fork(2)
        with pytest.raises(ValueError):
            ops.KVCache(1, 1, 2, 64, "cpu", kv_dtype="fp8").fork(2)
