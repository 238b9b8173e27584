"""The sampling rule of ops/sample.py on the CPU (sample_reference, the host replica of the fused kernel): every clause
on hand-built rows, the accuracy of the integer masses, the quality of the hash draw, and GPT2.generate on the fused
route with the tiny model of tests/test_generate.py."""
import numpy as np
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops import sample as S

NINF = float("-inf")
TOP = (1 << 32) - 1


def _state(B, width=4, pos=0):
    return (torch.zeros(B, width, dtype=torch.int64), torch.full((B,), pos, dtype=torch.int64),
            torch.zeros(B, dtype=torch.bool))


def _one(row, U=0, n=None, width=8, hist=(), **kw):
    """Token of one hand-built row (padded to a multiple of 8) with the injected draw U."""
    n = len(row) if n is None else n
    x = torch.zeros(1, (len(row) + 7) // 8 * 8)
    x[0, :len(row)] = torch.tensor(row, dtype=torch.float32)
    out = torch.zeros(1, width, dtype=torch.int64)
    out[0, :len(hist)] = torch.tensor(list(hist), dtype=torch.int64)
    pos = torch.tensor([len(hist)])
    done = torch.zeros(1, dtype=torch.bool)
    kw.setdefault("temperature", 1.0)
    tok = ops.sample_logits(x, n=n, out=out, pos=pos, done=done, uniform=torch.tensor([U]), **kw)
    return int(tok[0])


def _support(row, **kw):
    """Every token the row can give: the draws at the two ends and a fine sweep between them."""
    us = [0, TOP] + [int(u) for u in np.linspace(0, TOP, 515)]
    return sorted({_one(row, U=u, **kw) for u in us})


def test_table_and_log2e():
    tab = S.mass_table()
    assert tab.shape == (257,) and tab[0] == 1 << 31 and tab[256] == 1 << 30
    assert (np.diff(tab) < 0).all()
    assert S._LOG2E.view(np.uint32) == 0x3FB8AA3B


def test_top_k_keeps_ties_at_the_kth_value():
    row = [3.0, 1.0, 2.0, 2.0, 0.5, 2.0, -1.0, 0.0]
    assert _support(row, top_k=1) == [0]
    assert _support(row, top_k=2) == [0, 2, 3, 5]      # the 2nd largest value is 2.0, held three times
    assert _support(row, top_k=4) == [0, 2, 3, 5]
    assert _support(row, top_k=5) == [0, 1, 2, 3, 5]
    assert _support(row, top_k=0) == _support(row, top_k=None) == _support(row, top_k=8) == list(range(8))


def test_top_p_threshold_and_ties():
    # masses 2^31 * (1, 1/2, 1/2, 1/4, 1/4): exact in the table (t = 0, 1, 2 at idx = rem = 0)
    ln2 = float(np.log(2.0))
    row = [0.0, -ln2, -ln2, -2 * ln2, -2 * ln2, NINF, NINF, NINF]
    q = S.masses(np.array(row, dtype=np.float32))
    assert q[0] == 1 << 31 and q[5] == 0
    W = int(q.sum())
    frac = [int(q[0]) / W, int(q[:3].sum()) / W]
    assert _support(row, top_p=frac[0] - 0.01) == [0]
    assert _support(row, top_p=frac[0] + 0.01) == [0, 1, 2]       # needs part of the tie: all of it is kept
    assert _support(row, top_p=frac[1] - 0.01) == [0, 1, 2]
    assert _support(row, top_p=frac[1] + 0.01) == [0, 1, 2, 3, 4]
    assert _support(row, top_p=1.0) == _support(row, top_p=None) == [0, 1, 2, 3, 4]
    assert _support(row, top_p=1e-9) == [0] and _support(row, top_p=0.0) == [0]   # only the maximum survives
    # over the top-k survivors: k = 1 leaves the maximum whatever p is
    assert _support(row, top_k=1, top_p=0.99) == [0]


def test_repetition_penalty_signs_and_out_of_range_ids():
    row = [2.0, -2.0, 1.9, -1.0, 0.0, 0.0, 0.0, 0.0]
    # greedy: 2.0 / 1.25 = 1.6 < 1.9
    assert _one(row, temperature=0.0) == 0
    assert _one(row, temperature=0.0, repetition_penalty=1.25, hist=[0]) == 2
    # ids outside [0, n) are ignored, and so is everything at or past pos
    assert _one(row, temperature=0.0, repetition_penalty=1.25, hist=[-1, 8, 10 ** 6]) == 0
    # a negative logit is multiplied: -1.0 * 4 = -4 falls below -2.0
    neg = [-2.0, -1.0, -3.0, -3.0, -3.0, -3.0, -3.0, -3.0]
    assert _one(neg, temperature=0.0) == 1
    assert _one(neg, temperature=0.0, repetition_penalty=4.0, hist=[1]) == 0
    # the factors are f32(r) and f32(1/r), one multiply each
    x = np.float32(1.7)
    s = S._settings(8, 1.0, None, None, 1.3, 0)
    z = S._pick_row(np.array([x] * 8, dtype=np.float32), dict(s, greedy=True), np.array([0]), None)
    assert z == 1 and s["inv_r"] == np.float32(1 / 1.3) and s["r"] == np.float32(1.3)


def test_draw_ends_and_index_order():
    row = [0.0] * 8
    assert _one(row, U=0) == 0 and _one(row, U=TOP) == 7
    for j in range(8):   # 8 equal masses: floor(U * 8 / 2^32)
        assert _one(row, U=(j << 29)) == j and _one(row, U=((j + 1) << 29) - 1) == j
    assert _one([NINF, NINF, 0.0, NINF, 0.0, NINF, NINF, NINF], U=0) == 2


def test_inf_nan_and_empty_rows():
    nan = float("nan")
    assert _support([NINF, nan, 1.0, nan, 1.0, NINF, NINF, NINF]) == [2, 4]
    assert _one([nan, 5.0, nan, 1.0, 0.0, 0.0, 0.0, 0.0], temperature=0.0) == 1
    for kw in (dict(), dict(top_k=3), dict(top_p=0.5), dict(temperature=0.0)):
        assert _one([NINF] * 8, U=TOP, **kw) == 0
        assert _one([nan] * 8, U=TOP, **kw) == 0
    # entries at or past n do not exist
    assert _support([0.0, 0.0, 0.0, 9.0, 9.0, 9.0, 9.0, 9.0], n=3) == [0, 1, 2]
    # t = 43.3 is outside [0, 40): no mass; t = 28.9 leaves 2^31 * 2^-28.9 = 4 units, reached by the last draw only
    assert _support([0.0, -30.0, -20.0, NINF, NINF, NINF, NINF, NINF]) == [0, 2]
    assert S.masses(np.array([0.0, -30.0, -20.0], dtype=np.float32)).tolist() == [1 << 31, 0, 4]


def test_greedy_tie_takes_the_lowest_index():
    assert _one([1.0, 7.0, 7.0, 7.0, 0.0, 0.0, 0.0, 0.0], temperature=0.0, top_k=3, top_p=0.1) == 1
    assert _one([-0.0, 0.0, -1.0, -1.0, -1.0, -1.0, -1.0, -1.0], temperature=0.0) == 0


def test_done_eos_pad_and_positions():
    x = torch.zeros(4, 8)
    x[:, 3] = 50.0
    out = torch.full((4, 3), 9, dtype=torch.int64)
    pos = torch.tensor([0, 2, 3, 5])
    done = torch.tensor([False, True, False, False])
    tok = ops.sample_logits(x, n=8, temperature=0.0, out=out, pos=pos, done=done, eos=3, pad=6)
    assert tok.tolist() == [3, 6, 3, 3]
    assert done.tolist() == [True, True, True, True]
    assert pos.tolist() == [1, 3, 4, 6]
    assert out.tolist() == [[3, 9, 9], [9, 9, 6], [9, 9, 9], [9, 9, 9]]   # pos at and past the end: nothing written
    tok = ops.sample_logits(x, n=8, temperature=0.0, out=out, pos=pos, done=done, eos=3, pad=6)
    assert tok.tolist() == [6, 6, 6, 6] and out[0].tolist() == [3, 6, 9]
    # eos off: done stays; a pad equal to eos finishes nothing new
    out, pos, done = _state(1)
    ops.sample_logits(x[:1], n=8, temperature=0.0, out=out, pos=pos, done=done, eos=None, pad=6)
    assert not done[0] and out[0, 0] == 3


def test_argument_checks():
    out, pos, done = _state(2)
    ok = dict(out=out, pos=pos, done=done)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 65544), n=65537, **ok)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 12), n=8, **ok)                       # ld % 8
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 8), n=9, **ok)                        # n > ld
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 8), n=8, repetition_penalty=0.0, **ok)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 8, dtype=torch.float64), n=8, **ok)
    ops.sample_logits(torch.zeros(2, 16)[:, :8], n=8, **ok)                    # a strided view is fine


@pytest.mark.parametrize("sigma", [1.0, 4.0, 10.0])
def test_mass_accuracy_against_f64_softmax(sigma):
    rng = np.random.default_rng(int(sigma))
    z = (rng.standard_normal(50257) * sigma).astype(np.float32)
    q = S.masses(z).astype(np.float64)
    z64 = z.astype(np.float64)
    p = np.exp(z64 - z64.max())
    p /= p.sum()
    tv = 0.5 * np.abs(q / q.sum() - p).sum()
    print(f"sigma {sigma}: total variation between q / W and the f64 softmax {tv:.3e}")
    assert tv <= 1e-5
    assert q.max() == 2.0 ** 31 and q.sum() < 2.0 ** 47


def test_hash_draw_frequencies():
    rows, n = 65536, 16
    rng = np.random.default_rng(5)
    z = rng.standard_normal(n).astype(np.float32) * 1.5
    x = torch.from_numpy(z)[None, :].expand(rows, n).contiguous()
    out, pos, done = _state(rows, width=1)
    tok = ops.sample_logits(x, n=n, temperature=1.0, seed=1234, out=out, pos=pos, done=done).numpy()
    q = S.masses(z).astype(np.float64)
    p = q / q.sum()
    freq = np.bincount(tok, minlength=n) / rows
    dev = np.abs(freq - p) / np.sqrt(p * (1 - p) / rows)
    print("deviation of each frequency in binomial standard deviations:", np.round(dev, 2))
    assert (dev <= 5).all()
    # the hash of the rule, spelled out for one row
    assert S.hash_uniform(1234, 0, 0) == S._mix64(S._mix64(1234 + S._G) + S._G) >> 32


# ---------------------------------------------------------------- generate on the fused route (CPU reference path)
VOCAB, CTX, NEW = 200, 96, 24


@pytest.fixture(scope="module")
def tiny():
    with context.device("cpu"):
        initializers.set_seed(0)
        torch.manual_seed(0)
        model = GPT2(vocab=VOCAB, ctx=CTX, hidden=128, layers=2, heads=2)
        ids = torch.randint(0, VOCAB, (2, 5))
    return model, ids


def _gen(model, ids, n=NEW, **kw):
    with context.device("cpu"):
        return model.generate(ids, n, **kw)


def test_generate_fused_is_reproducible_and_seeded(tiny):
    model, ids = tiny
    kw = dict(temperature=0.9, top_p=0.9, repetition_penalty=1.2)
    a = _gen(model, ids, seed=11, **kw)
    b = _gen(model, ids, seed=11, **kw)
    c = _gen(model, ids, seed=12, **kw)
    assert a.dtype == torch.int64 and tuple(a.shape) == (2, 5 + NEW)
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a[:, :5], ids) and int(a.max()) < VOCAB and int(a.min()) >= 0
    assert model.last_generation["cache"].lens.tolist() == [5 + NEW, 5 + NEW]
    assert tuple(model.last_generation["logits"].shape) == (2, model.vocab_p)
    assert model.last_generation["step"] is None


def test_generate_fused_top1_is_greedy(tiny):
    model, ids = tiny
    greedy = _gen(model, ids)
    assert torch.equal(_gen(model, ids, sampler="fused"), greedy)
    assert torch.equal(_gen(model, ids, temperature=0.8, top_k=1, top_p=0.9, seed=3), greedy)
    assert torch.equal(_gen(model, ids, temperature=0.8, top_k=1, seed=3, sampler="fused"), greedy)


def test_generate_fused_ragged_rows_match_rows_alone_at_the_same_index(tiny):
    model, ids = tiny
    pad = 199
    rag = ids.clone()
    rag[1, 3:] = pad
    kw = dict(temperature=0.9, top_p=0.9, repetition_penalty=1.2, seed=5, pad_token_id=pad)
    out = _gen(model, rag, prompt_lens=torch.tensor([5, 3]), **kw)
    assert model.last_generation["cache"].lens.tolist() == [5 + NEW, 3 + NEW]
    # the draw is keyed by the row index, so each row runs alone as both rows of a batch of its own
    for b, L in ((0, 5), (1, 3)):
        alone = _gen(model, rag[b:b + 1, :L].expand(2, L).contiguous(), **kw)
        assert torch.equal(out[b, :L + NEW], alone[b]), f"row {b}"
    assert (out[1, 3 + NEW:] == pad).all()


def test_generate_fused_eos_row_emits_pad(tiny):
    model, ids = tiny
    kw = dict(temperature=0.9, top_p=0.9, repetition_penalty=1.2, seed=11)
    ref = _gen(model, ids, **kw)
    eos, pad = int(ref[0, 7]), 198
    out = _gen(model, ids, eos_token_id=eos, pad_token_id=pad, **kw)
    first = int((ref[0, 5:] == eos).nonzero()[0]) + 5
    assert torch.equal(out[0, :first + 1], ref[0, :first + 1]) and (out[0, first + 1:] == pad).all()


def test_generate_default_route_is_unchanged(tiny):
    """With top_p, repetition_penalty and sampler left alone the torch.Generator route runs: these are the tokens the
    parent commit gives for this model, prompt and seed (temperature=0.8, top_k=20, seed=7)."""
    model, ids = tiny
    out = _gen(model, ids, temperature=0.8, top_k=20, seed=7)
    with context.device("cpu"), torch.no_grad():   # the parent's loop, spelled out with its own aten calls
        gen = torch.Generator(device="cpu")
        gen.manual_seed(7)
        cache = model.new_cache(2, 5 + NEW, "cpu")
        h = model._hidden_cached(ids, cache)
        cache.set_lens(torch.tensor([5, 5]))
        logits = model._lm_head(h[:, -1:, :], decode=True)[:, 0]
        want = [ids]
        for _ in range(NEW):
            lg = logits.float()[:, :VOCAB] / 0.8
            kth = lg.topk(20, -1).values[:, -1:]
            lg = lg.masked_fill(lg < kth, float("-inf"))
            tok = torch.multinomial(torch.softmax(lg, -1), 1, generator=gen)
            want.append(tok)
            logits = model._lm_head(model._hidden_cached(tok, cache), decode=True)[:, 0]
            cache.advance(1)
    assert torch.equal(out, torch.cat(want, 1))
    assert torch.equal(_gen(model, ids, temperature=0.8, top_k=20, seed=7, sampler="torch"), out)


def test_generate_sampler_argument_checks(tiny):
    model, ids = tiny
    with pytest.raises(ValueError):
        _gen(model, ids, sampler="torch", top_p=0.9)
    with pytest.raises(ValueError):
        _gen(model, ids, sampler="torch", repetition_penalty=1.1)
    with pytest.raises(ValueError):
        _gen(model, ids, sampler="beam")
