"""Appending multi-token chunks to a filled KV cache on the CPU reference path (f32): call(..., append=True),
GPT2.extend (chunked, ragged) and generate(cache=..., prefill_chunk=...) against the full forward and the recompute
loop. The tiny model and the recompute loop are those of tests/test_generate.py."""
import pytest
import torch

from distributed_tensorflow_amd import context
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2

VOCAB, CTX, NEW = 200, 96, 24
MARGIN = 5e-3  # top-1 / top-2 logit gap the recompute path must keep for a token-for-token comparison to be meaningful
CPU = torch.device("cpu")


def _setup(seed):
    with context.device("cpu"):
        initializers.set_seed(seed)
        torch.manual_seed(seed)
        model = GPT2(vocab=VOCAB, ctx=CTX, hidden=128, layers=2, heads=2)
        ids = torch.randint(0, VOCAB, (2, 5))
    return model, ids


def _recompute(model, ids, n):
    """Full forward, argmax of the last position, concatenate. Also returns the smallest top-1 / top-2 margin seen."""
    margin = float("inf")
    with context.device("cpu"), torch.no_grad():
        for _ in range(n):
            lg = model(ids, training=False)[:, -1, :VOCAB].float()
            top = lg.topk(2, -1).values
            margin = min(margin, float((top[:, 0] - top[:, 1]).min()))
            ids = torch.cat([ids, lg.argmax(-1, keepdim=True)], 1)
    return ids, margin


_CACHE = {}


def _case(seed):
    if seed not in _CACHE:
        model, ids = _setup(seed)
        ref, margin = _recompute(model, ids, NEW)
        _CACHE[seed] = (model, ids, ref, margin)
    return _CACHE[seed]


def _prefilled(model, seq, n, capacity):
    """A cache holding the first n tokens of seq."""
    cache = model.new_cache(seq.shape[0], capacity, CPU)
    model(seq[:, :n], training=False, cache=cache)
    cache.advance(n)
    return cache


def test_append_logits_match_full_forward():
    model, _, ref, _ = _case(1)
    seq = ref[:, :12]
    with context.device("cpu"), torch.no_grad():
        full = model(seq, training=False)
        cache = model.new_cache(2, 12, CPU)
        lg = model(seq[:, :5], training=False, cache=cache)
        cache.advance(5)
        assert torch.allclose(lg, full[:, :5], atol=1e-4)
        lg = model(seq[:, 5:12], training=False, cache=cache, append=True)
        cache.advance(7)
    assert tuple(lg.shape) == tuple(full[:, 5:12].shape)
    assert torch.allclose(lg, full[:, 5:12], atol=1e-4)
    assert cache.lens.tolist() == [12, 12]


def test_append_with_empty_cache_is_the_prefill_and_one_token_is_the_step():
    model, _, ref, _ = _case(1)
    seq = ref[:, :8]
    with context.device("cpu"), torch.no_grad():
        full = model(seq, training=False)
        cache = model.new_cache(2, 8, CPU)
        lg = model(seq[:, :7], training=False, cache=cache, append=True)   # empty cache: today's prefill
        cache.advance(7)
        assert torch.allclose(lg, full[:, :7], atol=1e-4)
        lg = model(seq[:, 7:8], training=False, cache=cache, append=True)  # one token: today's step
        assert torch.allclose(lg[:, 0], full[:, 7], atol=1e-4)


@pytest.mark.parametrize("chunk", [1, 2, 3, 7])
def test_extend_chunk_size_does_not_matter(chunk):
    model, _, ref, _ = _case(1)
    seq = ref[:, :12]
    with context.device("cpu"):
        one = _prefilled(model, seq, 5, 12)
        want = model.extend(seq[:, 5:12], one)
        cache = _prefilled(model, seq, 5, 12)
        got = model.extend(seq[:, 5:12], cache, chunk=chunk)
        full = model(seq, training=False)
    assert tuple(got.shape) == (2, model.vocab_p)
    assert torch.allclose(got, want, atol=1e-4)
    assert torch.allclose(want, full[:, 11], atol=1e-4)
    assert cache.lens.tolist() == [12, 12] and one.lens.tolist() == [12, 12]


def test_extend_into_an_empty_cache_in_pieces():
    model, _, ref, _ = _case(2)
    seq = ref[:, :11]
    with context.device("cpu"):
        full = model(seq, training=False)
        cache = model.new_cache(2, 11, CPU)
        got = model.extend(seq, cache, chunk=4)
    assert torch.allclose(got, full[:, 10], atol=1e-4)
    assert cache.lens.tolist() == [11, 11]


def _ragged(model, seq, start, chunk):
    """Rows 0 / 1 get 4 / 2 new tokens behind `start` cached ones (row 1 right-padded); each row against a single-row
    run of its own valid tokens."""
    pad = 199
    new = seq[:, start:start + 4].clone()
    new[1, 2:] = pad
    with context.device("cpu"):
        cache = _prefilled(model, seq, start, CTX)
        got = model.extend(new, cache, new_lens=torch.tensor([4, 2]), chunk=chunk)
        assert cache.lens.tolist() == [start + 4, start + 2]
        for b, n in ((0, 4), (1, 2)):
            one = _prefilled(model, seq[b:b + 1], start, CTX)
            want = model.extend(seq[b:b + 1, start:start + n], one)
            assert torch.allclose(got[b], want[0], atol=1e-4), (b, chunk)
    return cache


@pytest.mark.parametrize("chunk", [None, 3])
def test_extend_ragged_rows_match_single_row_runs(chunk):
    model, _, ref, _ = _case(0)
    cache = _ragged(model, ref, 5, chunk)
    # the pad K/V that row 1 stored past its end are rewritten by what follows: a further turn of both rows equals
    # single-row runs again
    with context.device("cpu"):
        nxt = ref[:, 20:23]
        got = model.extend(nxt, cache)
        hist = torch.cat([ref[1:2, :7], nxt[1:2]], 1)
        want = model(hist, training=False)[:, -1]
    assert torch.allclose(got[1], want[0], atol=1e-4)


@pytest.mark.parametrize("chunk", [None, 1, 2])
def test_extend_ragged_rows_near_the_context_end(chunk):
    """Row 0 ends exactly at ctx; the pad positions of row 1 pass the position table (clamped on the device), in
    multi-token pieces and in single-token ones (chunk=1: row 1 is full, its pad token sits at position ctx)."""
    model, _, _, _ = _case(0)
    torch.manual_seed(5)
    seq = torch.randint(0, VOCAB, (2, CTX))
    pad = 199
    with context.device("cpu"):
        cache = _prefilled(model, seq, CTX - 4, CTX)
        model.extend(seq[:, CTX - 4:CTX - 2], cache, new_lens=torch.tensor([0, 2]), chunk=chunk)  # row 0: nothing
        assert cache.lens.tolist() == [CTX - 4, CTX - 2]
        # row 1's two pad tokens sit at positions CTX and CTX + 1 (in single-token pieces: both at CTX)
        new = torch.full((2, 4), pad)
        new[0] = seq[0, CTX - 4:]
        new[1, :2] = seq[1, CTX - 2:]
        got = model.extend(new, cache, new_lens=torch.tensor([4, 2]), chunk=chunk)
        assert cache.lens.tolist() == [CTX, CTX]
        full = model(seq, training=False)
    assert torch.allclose(got, full[:, -1], atol=1e-4)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_continuation_reproduces_the_greedy_run(seed):
    model, ids, ref, margin = _case(seed)
    print(f"seed {seed}: min top-1/top-2 margin of the recompute path {margin:.4f}")
    assert margin >= MARGIN, f"precondition: recompute margin {margin}"
    with context.device("cpu"):
        first = model.generate(ids, 8)
        assert torch.equal(first, ref[:, :13])
        cache = model.last_generation["cache"]
        assert cache.lens.tolist() == [13, 13]
        out = model.generate(ref[:, 13:17], 12, cache=cache)
        assert out.dtype == torch.int64 and tuple(out.shape) == (2, 16)
        assert torch.equal(out, ref[:, 13:29])
        assert model.last_generation["cache"] is cache and cache.lens.tolist() == [29, 29]
        chunked = model.generate(ids, NEW, prefill_chunk=2)
    assert torch.equal(chunked, ref)


def test_generate_with_a_cache_checks_its_arguments():
    model, ids, ref, _ = _case(0)
    with context.device("cpu"):
        model.generate(ids, 8)
        cache = model.last_generation["cache"]          # 13 tokens, capacity 64
        assert cache.capacity == 64
        with pytest.raises(ValueError):
            model.generate(ref[:, 13:17], 64 - 13 - 4 + 1, cache=cache)      # capacity overflow
        with pytest.raises(ValueError):
            model.generate(ref[:1, 13:17], 4, cache=cache)                   # batch mismatch
        big = model.new_cache(2, 2 * CTX, CPU)
        model.extend(ref[:, :13], big)
        with pytest.raises(ValueError):
            model.generate(ref[:, 13:17], CTX - 13 - 4 + 1, cache=big)       # context overflow
        assert big.lens.tolist() == [13, 13], "a refused call must not touch the cache"
        out = model.generate(ref[:, 13:17], CTX - 13 - 4, cache=big)         # exactly full: fine
    assert tuple(out.shape) == (2, CTX - 13)
