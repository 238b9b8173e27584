"""Beam search on the GPU: ops.beam_select (csrc/kernels/beam.hip) against an f64 numpy ranking, the slot-indirect
suffix pass of KVCache.fork(beams=True).attend against an f64 softmax, KVCache.reorder against a torch gather, and
GPT2.generate(num_beams=) end to end.

SCORE_TOL, for |value| < 64 (f32 ulp 3.8e-6): two roundings of the value 3.8e-6; lse = m + log(sum), the sum over at
most 86 sequential f32 additions (5.1e-6) of exponentials good to about 3e-6, the log and the add about 2e-6: 1.4e-5,
doubled because the exp / log figures are estimates. ATTN_TOL and its scale are those of tests/test_shared_prefix_gpu.py.
"""
import numpy as np
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops._util import launch_counts, launch_delta
from test_beam import CFG, VOCAB, forced_scores

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
SCORE_TOL = 3e-5
ATTN_TOL = 2e-2
H, CAP, B0 = 2, 384, 2


def ranking(logits, n, scores, done, G, pad):
    """f64: per group the G + 1 best (value, beam, token), ties to the smaller beam * n + token."""
    x = logits.double().cpu().numpy()[:, :n]
    m = x.max(-1, keepdims=True)
    val = scores.double().cpu().numpy()[:, None] + (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True)))
    dn = done.cpu().numpy()
    valid = np.repeat(~dn[:, None], n, 1)
    valid[dn, pad] = True
    val[dn, pad] = scores.double().cpu().numpy()[dn]
    out = []
    for g in range(len(dn) // G):
        v = val[g * G:(g + 1) * G].ravel()
        idx = np.flatnonzero(valid[g * G:(g + 1) * G].ravel())
        top = idx[np.lexsort((idx, -v[idx]))][:G + 1]
        out.append((v[top], top // n, top % n))
    return out


def check_select(logits, n, scores, done, G, eos, pad):
    want = ranking(logits, n, scores, done, G, pad)
    for v, _, _ in want:   # the reference itself separates what the kernel has to separate (exact ties aside)
        gap = (v[:-1] - v[1:])[np.isfinite(v[:-1]) & (v[:-1] != v[1:])]
        assert (gap > 2 * SCORE_TOL).all(), gap
    s, d = scores.clone(), done.clone()
    before = launch_counts()
    parent, token = ops.beam_select(logits, n=n, scores=s, done=d, group=G, eos=eos, pad=pad)
    assert launch_delta(before)["beam_select"] == 1
    for g, (v, par, tok) in enumerate(want):
        rows = slice(g * G, (g + 1) * G)
        assert parent[rows].tolist() == par[:G].tolist() and token[rows].tolist() == tok[:G].tolist(), (g, par, tok)
        got, fin = s[rows].double().cpu().numpy(), np.isfinite(v[:G])
        assert np.array_equal(got[~fin], v[:G][~fin]) and np.abs(got[fin] - v[:G][fin]).max() <= SCORE_TOL
        assert d[rows].tolist() == (done.cpu().numpy()[g * G + par[:G]] | (tok[:G] == eos)).tolist()
    s2 = scores.clone()
    again = ops.beam_select(logits, n=n, scores=s2, done=done.clone(), group=G, eos=eos, pad=pad)
    assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(again[1], token), "two calls differ"


def planted(n, ld, G, dtype, cuda):
    """Random logits with 2 G peaks a row (the top of every row is a handful of well separated values)."""
    x = torch.randn(B0 * G, ld)
    for r in range(B0 * G):
        x[r, torch.randperm(n)[:2 * G]] += 4 + 5 * torch.rand(2 * G)
    return x.to(BF).to(dtype).to(cuda)


@pytest.mark.parametrize("dtype", [BF, torch.float32])
@pytest.mark.parametrize("n,ld", [(200, 200), (50257, 50304)])
@pytest.mark.parametrize("G", [2, 5, 16])
def test_beam_select(cuda, G, n, ld, dtype):
    """Group 0 all live; group 1 with rows 0 and 1 done and a score of -inf on its last row."""
    torch.manual_seed(G * 7 + n)
    logits = planted(n, ld, G, dtype, cuda)
    scores = (-20 * torch.rand(B0 * G)).to(cuda)
    scores[-1] = float("-inf")
    done = torch.zeros(B0 * G, dtype=torch.bool, device=cuda)
    done[G:G + 2] = True
    eos = int(logits[0, :n].argmax())   # a token that wins
    check_select(logits, n, scores, done, G, eos, pad=n - 1)


@pytest.mark.parametrize("case", ["ties", "init"])
def test_beam_select_ties_and_first_step(cuda, case):
    """ties: rows 0 and 1 hold the same logits and the same score, so every candidate of row 0 ties with row 1's and
    the smaller index goes first. init: scores [0, -inf, ...] over G copies of one row give that row's G best."""
    torch.manual_seed(11)
    G, n = 5, 200
    logits = planted(n, n, G, torch.float32, cuda)
    scores = (-20 * torch.rand(B0 * G)).to(cuda)
    if case == "ties":
        logits[1], scores[1] = logits[0], scores[0]
        scores[2:G] = -60.0
    else:
        logits[:G], logits[G:] = logits[0], logits[G]
        scores = torch.tensor([0.0] + [float("-inf")] * (G - 1), device=cuda).repeat(B0)
    done = torch.zeros(B0 * G, dtype=torch.bool, device=cuda)
    check_select(logits, n, scores, done, G, -1, pad=0)


@pytest.mark.parametrize("owns", [(1, 130), (130, 1)])
@pytest.mark.parametrize("plens", [(1, 127), (128, 129)])
@pytest.mark.parametrize("G", [2, 5, 16])
def test_indirect_attend(cuda, G, plens, owns):
    """Group g has owns[g] own positions behind its prefix of plens[g]; own position p of row b is read from the row
    the table names, position lens[b] from row b, and table bytes outside [P, lens) hold 255."""
    torch.manual_seed(G * 1000 + plens[0] + owns[0])
    B = B0 * G
    lens = torch.tensor([plens[b // G] + owns[b // G] for b in range(B)], device=cuda)
    pos = torch.arange(CAP, device=cuda)
    parent = ops.KVCache(1, B0, H, CAP, cuda)
    parent.set_lens(torch.tensor(plens, device=cuda))
    parent.empty = False
    dead = (pos[None, :] >= parent.lens[:, None])[None, :, None, :, None]
    parent.k = torch.randn(1, B0, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    parent.v = torch.randn(1, B0, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    fork, plain = parent.fork(G, beams=True), parent.fork(G)
    P = fork.plens.repeat_interleave(G)
    own = (pos[None, :] >= P[:, None]) & (pos[None, :] < lens[:, None])
    dead = ~(own | (pos[None, :] == lens[:, None]))[None, :, None, :, None]
    plain.k = fork.k = torch.randn(1, B, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    plain.v = fork.v = torch.randn(1, B, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    fork.set_lens(lens)
    plain.set_lens(lens)
    qkv = torch.randn(B, 1, 3 * H * 64, device=cuda).to(BF)
    fork.store(0, qkv)
    assert fork.slots.tolist() == [[b % G] * CAP for b in range(B)]
    assert torch.equal(fork.attend(0, qkv).view(torch.int16), plain.attend(0, qkv).view(torch.int16))
    table = torch.randint(0, G, (B, CAP), device=cuda)
    fork.slots = torch.where(own, table, torch.full_like(table, 255)).to(torch.uint8)
    before = launch_counts()
    out = fork.attend(0, qkv)
    assert launch_delta(before)["attn_decode_beam"] == 1
    src = torch.where(own, torch.arange(B, device=cuda)[:, None] // G * G + table, torch.arange(B, device=cuda)[:, None])
    q = qkv[:, 0, :H * 64].double().reshape(B, H, 64)
    ref = torch.empty_like(q)
    for b in range(B):
        p0, n = int(P[b]), int(lens[b]) + 1
        K = torch.cat([parent.k[0, b // G, :, :p0], fork.k[0, src[b, p0:n], :, pos[p0:n]].transpose(0, 1)], 1).double()
        V = torch.cat([parent.v[0, b // G, :, :p0], fork.v[0, src[b, p0:n], :, pos[p0:n]].transpose(0, 1)], 1).double()
        ref[b] = torch.einsum("hn,hnd->hd", torch.softmax(torch.einsum("hd,hnd->hn", q[b], K) / 8.0, -1), V)
    assert torch.isfinite(out.float()).all()
    ref = ref.reshape(B, 1, H * 64).float()
    assert (out.float() - ref).abs().max() <= ATTN_TOL * (ref.abs().max() + 1e-6)
    assert torch.equal(out.view(torch.int16), fork.attend(0, qkv).view(torch.int16)), "two calls differ in bits"


@pytest.mark.parametrize("G", [2, 5, 16])
def test_reorder_is_a_gather(cuda, G):
    """Group 0 keeps its beams (identity), group 1 draws parents with duplicates; lengths 5 and 70; a history wider
    than the cache (width 300 > capacity 128: more than one block of columns)."""
    torch.manual_seed(G)
    B, width = B0 * G, 300
    base = ops.KVCache(1, B0, 1, 128, cuda)
    base.empty = False
    fork = base.fork(G, beams=True)
    lens = torch.tensor([5] * G + [70] * G, device=cuda)
    fork.set_lens(lens)
    parent = torch.cat([torch.arange(G), torch.randint(0, G, (G,)) // 2]).int().to(cuda)
    slots0 = torch.randint(0, G, (B, 128), device=cuda).to(torch.uint8)
    hist0 = torch.randint(0, 1000, (B, width), device=cuda)
    token = torch.randint(0, 1000, (B,), device=cuda)
    rows = torch.arange(B, device=cuda) // G * G + parent.long()
    p = torch.arange(128, device=cuda)[None, :]
    want_slots = torch.where(p < lens[:, None] - 1, slots0[rows], slots0)
    want_slots = torch.where(p == lens[:, None] - 1, parent.to(torch.uint8)[:, None], want_slots)
    want_hist = hist0[rows].scatter(1, lens[:, None], token[:, None])
    got = []
    for _ in range(2):
        fork.slots, hist = slots0.clone(), hist0.clone()
        fork.reorder(parent, history=hist, token=token)
        got.append((fork.slots, hist))
    assert torch.equal(got[0][0], want_slots) and torch.equal(got[0][1], want_hist)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])


def test_generate_beams_end_to_end(cuda):
    """Every beam's score is the teacher-forced sum of log-probabilities of its own tokens (wrong if the slot table or
    the history were reordered wrongly). Tolerance: 8 new tokens times the per-logit bound of
    tests/test_generate_gpu.py (1.5 x the error of the GPU's full forward against the f32 reference)."""
    initializers.set_seed(0)
    torch.manual_seed(0)
    ids, plens, G, n_new = torch.randint(0, VOCAB, (2, 40)), torch.tensor([40, 33]), 4, 8
    with context.device(cuda), torch.no_grad():
        gpu = GPT2(**CFG)
        dids, dpl = ids.to(cuda), plens.to(cuda)
        gpu.generate(dids, n_new, prompt_lens=dpl, num_beams=G)
        eos = int(gpu.last_generation["beams"][0, 40 + 2])
        kw = dict(prompt_lens=dpl, num_beams=G, eos_token_id=eos, pad_token_id=VOCAB - 1)
        best = gpu.generate(dids, n_new, graph=True, **kw)
        got = gpu.last_generation
        assert got["step"].captured
        before = launch_counts()
        eager = gpu.generate(dids, n_new, graph=False, **kw)
        delta = launch_delta(before)
        eager_beams = gpu.last_generation["beams"]
        full = gpu(got["beams"], training=False).float()[..., :VOCAB].cpu()
    with context.device("cpu"), torch.no_grad():
        cpu = GPT2(**CFG)
        cpu(ids, training=False)
        cpu.set_weights(gpu.get_weights())
        ref = cpu(got["beams"].cpu(), training=False).float()[..., :VOCAB]
    beams, scores = got["beams"].cpu(), got["beam_scores"].cpu()
    assert delta["beam_select"] == n_new and delta["attn_decode_beam"] == n_new * CFG["layers"], delta
    assert torch.equal(best, eager) and torch.equal(got["beams"], eager_beams) and torch.equal(best.cpu(), beams[::G])
    assert tuple(best.shape) == (2, 48) and (beams == eos).any() and got["cache"].slots is not None
    assert (scores.reshape(2, G)[:, :-1] >= scores.reshape(2, G)[:, 1:]).all()
    want = forced_scores(ref, beams, plens.repeat_interleave(G), n_new, eos)
    tol = n_new * 1.5 * (full - ref).abs().max().item()
    err = (scores.double() - want).abs().max().item()
    print(f"max |beam score - forced f32 reference| {err:.5f} (tolerance {tol:.5f})")
    assert err <= tol, (scores, want)
