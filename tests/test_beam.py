"""Beam search on the CPU reference path: GPT2.generate(num_beams=) with ops.beam_select and KVCache.reorder in torch."""
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2

VOCAB = 200
CFG = dict(vocab=VOCAB, ctx=96, hidden=128, layers=2, heads=2)


def forced_scores(logits, beams, plens, n_new, eos):
    """Sum over each row's new tokens (up to and including eos) of log_softmax(logits [rows, S, VOCAB])[position - 1]."""
    lp = torch.log_softmax(logits.double(), -1)
    tot = torch.zeros(beams.shape[0], dtype=torch.float64)
    for b in range(beams.shape[0]):
        for p in range(int(plens[b]), int(plens[b]) + n_new):
            tot[b] += lp[b, p - 1, beams[b, p]]
            if int(beams[b, p]) == eos:
                break
    return tot


@pytest.fixture(scope="module")
def model():
    initializers.set_seed(0)
    torch.manual_seed(0)
    with context.device("cpu"), torch.no_grad():
        m = GPT2(**CFG)
        m(torch.randint(0, VOCAB, (1, 4)), training=False)
    return m


def test_beam_scores_are_the_forced_log_probabilities(model):
    torch.manual_seed(3)
    ids, plens, G, n_new = torch.randint(0, VOCAB, (2, 12)), torch.tensor([12, 7]), 4, 8
    with context.device("cpu"), torch.no_grad():
        model.generate(ids, n_new, prompt_lens=plens, num_beams=G)
        eos = int(model.last_generation["beams"][0, 12 + 2])   # a token the best beam does produce
        best = model.generate(ids, n_new, prompt_lens=plens, num_beams=G, eos_token_id=eos, pad_token_id=VOCAB - 1)
        got = model.last_generation
        full = model(got["beams"], training=False).float()[..., :VOCAB]
    beams, scores = got["beams"], got["beam_scores"]
    assert tuple(best.shape) == (2, 20) and torch.equal(best, beams[::G]) and (beams == eos).any()
    want = forced_scores(full, beams, plens.repeat_interleave(G), n_new, eos)
    assert (scores.double() - want).abs().max() <= 1e-4, (scores, want)   # f32 sums of 8 terms of magnitude < 8
    assert (scores.reshape(2, G)[:, :-1] >= scores.reshape(2, G)[:, 1:]).all()


def test_one_step_is_the_top_tokens_of_the_prompt_logits(model):
    torch.manual_seed(4)
    ids, G = torch.randint(0, VOCAB, (2, 9)), 5
    with context.device("cpu"), torch.no_grad():
        model.generate(ids, 1, num_beams=G)
        got = model.last_generation
        top = torch.log_softmax(model(ids, training=False).float()[:, -1, :VOCAB], -1).topk(G, -1)
    assert torch.equal(got["beams"][:, -1].reshape(2, G), top.indices)
    assert torch.allclose(got["beam_scores"].reshape(2, G), top.values, atol=1e-5)


@pytest.mark.parametrize("kw", [dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(repetition_penalty=1.2),
                                dict(sampler="fused"), dict(num_return_sequences=2), dict(prefill_chunk=4),
                                dict(step="fused"), dict(kv_dtype="fp8"), dict(num_beams=1), dict(num_beams=17),
                                dict(cache=object()), dict(vocab=65544)])
def test_refused_combinations(model, kw):
    if "vocab" in kw:
        with context.device("cpu"):
            model, kw = GPT2(vocab=kw["vocab"], ctx=8, hidden=64, layers=1, heads=1), {}
    with pytest.raises(ValueError):
        model.generate(torch.zeros(1, 4, dtype=torch.long), 2, **{"num_beams": 4, **kw})
