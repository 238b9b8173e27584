"""KV-cached GPT-2 generation on the GPU (bf16): the cached step against the f32 CPU reference, measured by the
error of the existing full-forward GPU path against that same reference, and hipGraph replay against eager steps.

Token equality with the recompute path is not asserted here: bf16 error is of the order of the top-1 / top-2 margins
of this tiny model (tests/test_generate.py asserts it in f32).
"""
import pytest
import torch

from distributed_tensorflow_amd import context
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2

pytestmark = pytest.mark.gpu
VOCAB, CTX = 200, 96
CFG = dict(vocab=VOCAB, ctx=CTX, hidden=128, layers=2, heads=2)


@pytest.fixture(scope="module")
def models(cuda):
    """The tiny model on the GPU and an f32 CPU copy of the same weights."""
    initializers.set_seed(0)
    torch.manual_seed(0)
    probe = torch.randint(0, VOCAB, (1, 4))
    with context.device(cuda), torch.no_grad():
        gpu = GPT2(**CFG)
        gpu(probe.to(cuda), training=False)   # builds the layers
    with context.device("cpu"), torch.no_grad():
        cpu = GPT2(**CFG)
        cpu(probe, training=False)
        cpu.set_weights(gpu.get_weights())
    return gpu, cpu


def test_teacher_forced_logits_track_the_full_forward(cuda, models):
    """Prefill 5 tokens, feed 24 fixed tokens through the cached step; each step's logits against the f32 CPU
    reference must stay within 1.5x of the error of the full-forward GPU path on the same positions (the decode
    kernels round in a different order from the prefill kernels, not more coarsely)."""
    gpu, cpu = models
    torch.manual_seed(1)
    seq = torch.randint(0, VOCAB, (2, 29))
    with context.device("cpu"), torch.no_grad():
        ref = cpu(seq, training=False).float()[:, 5:, :VOCAB]
    dseq = seq.to(cuda)
    with context.device(cuda), torch.no_grad():
        full = gpu(dseq, training=False).float()[:, 5:, :VOCAB].cpu()
        cache = gpu.new_cache(2, 29, cuda)
        gpu(dseq[:, :5], training=False, cache=cache)
        cache.advance(5)
        steps = []
        for t in range(5, 29):
            steps.append(gpu(dseq[:, t:t + 1].contiguous(), training=False, cache=cache))
            cache.advance(1)
        cached = torch.cat(steps, 1).float()[:, :, :VOCAB].cpu()
    err_full = (full - ref).abs().max().item()
    err_cached = (cached - ref).abs().max().item()
    print(f"max |logits - f32 CPU reference| over 24 positions: full forward {err_full:.5f}, "
          f"cached steps {err_cached:.5f} (ratio {err_cached / err_full:.3f}, logit scale {ref.abs().max():.3f})")
    assert err_cached <= 1.5 * err_full, (err_cached, err_full)
    assert cache.lens.tolist() == [29, 29]


@pytest.mark.parametrize("B", [1, 3])
def test_graph_replay_equals_eager_steps(cuda, models, B):
    gpu, _ = models
    torch.manual_seed(2 + B)
    new, pad = 12, 0
    ids = torch.randint(1, VOCAB, (B, 5), device=cuda)
    plens = [5, 3, 4][:B]
    for b in range(B):
        ids[b, plens[b]:] = pad
    kw = dict(prompt_lens=torch.tensor(plens), pad_token_id=pad)
    with context.device(cuda):
        a = gpu.generate(ids, new, graph=True, **kw)
        ga = gpu.last_generation
        b_ = gpu.generate(ids, new, graph=False, **kw)
        gb = gpu.last_generation
    assert ga["step"] is not None and ga["step"].captured, "the one-token step was not captured"
    assert gb["step"] is None
    assert torch.equal(a, b_)
    assert torch.equal(ga["logits"].view(torch.int16), gb["logits"].view(torch.int16))
    want = [p + new for p in plens]
    assert ga["cache"].lens.tolist() == want and gb["cache"].lens.tolist() == want
    assert a.dtype == torch.int64 and tuple(a.shape) == (B, 5 + new)
    assert int(a.max()) < VOCAB and int(a.min()) >= 0
    for b in range(B):
        assert torch.equal(a[b, :plens[b]], ids[b, :plens[b]]), "prompt not preserved"
        assert (a[b, plens[b] + new:] == pad).all(), "tail is not padding"


def test_fp8_model_decodes_in_bf16(cuda, models):
    """An fp8=True model generates from the bf16 shadows of its weights: the same kernels, hence the same tokens and
    logits bit for bit as the bf16 model with those weights."""
    gpu, _ = models
    torch.manual_seed(12)
    ids = torch.randint(0, VOCAB, (2, 5), device=cuda)
    with context.device(cuda):
        f8 = GPT2(fp8=True, **CFG)
        f8.generate(ids, 1, graph=False)   # builds the layers
        ours, theirs = f8.get_weights(), gpu.get_weights()
        assert len(ours) == len(theirs)
        f8.set_weights(theirs)
        a = f8.generate(ids, 6, graph=False)
        la = f8.last_generation["logits"]
        b = gpu.generate(ids, 6, graph=False)
        lb = gpu.last_generation["logits"]
    assert torch.equal(a, b)
    assert torch.equal(la.view(torch.int16), lb.view(torch.int16))


def test_sampling_and_eos_on_the_gpu(cuda, models):
    gpu, _ = models
    torch.manual_seed(9)
    ids = torch.randint(0, VOCAB, (2, 5), device=cuda)
    with context.device(cuda):
        a = gpu.generate(ids, 8, temperature=0.9, top_k=10, seed=4, graph=False)
        b = gpu.generate(ids, 8, temperature=0.9, top_k=10, seed=4, graph=False)
        g = gpu.generate(ids, 8, graph=False)
        eos = int(g[0, 5])
        e = gpu.generate(ids, 8, eos_token_id=eos, pad_token_id=199, graph=False)
    assert torch.equal(a, b) and int(a.max()) < VOCAB
    assert int(e[0, 5]) == eos and (e[0, 6:] == 199).all()
