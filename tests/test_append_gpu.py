"""Multi-token append attention on the GPU (dtf_attn_append, csrc/kernels/attention.hip): S > 1 queries per row behind a
filled KV cache, per-row lengths read on the device. The route is opt-in per cache (chunked=True); a default cache keeps
its refusal. Kernel tests compare against the f32 CPU path of KVCache.attend_chunk, with the training forward on the
same data as the error bar; model tests use the tiny model and the error measure of tests/test_extend_gpu.py."""
import pytest
import torch

from distributed_tensorflow_amd import context, graphs, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops._util import call_log, launch_counts, launch_delta

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
B, H, SMAX = 2, 3, 320          # five 64-key tiles, not a multiple of 128; H is not a power of two
VOCAB, CTX = 200, 96
CFG = dict(vocab=VOCAB, ctx=CTX, hidden=128, layers=2, heads=2)
NAN = float("nan")


def bits(t):
    return t.contiguous().view(torch.int16)


def filled_cache(cuda, lens, seed, poison=True):
    """A chunked one-layer GPU cache with random bf16 K/V below lens[b] and (poison) bf16 NaN at and past it, and the
    f32 CPU cache of the same contents with zeros in place of the NaNs."""
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(1, B, H, SMAX, 64, generator=g).to(BF)
    v = torch.randn(1, B, H, SMAX, 64, generator=g).to(BF)
    cache = ops.KVCache(1, B, H, SMAX, cuda, chunked=True)
    ref = ops.KVCache(1, B, H, SMAX, "cpu")
    cache.k.copy_(k)
    cache.v.copy_(v)
    ref.k.copy_(k.float())
    ref.v.copy_(v.float())
    for b, n in enumerate(lens):
        if poison:
            cache.k[:, b, :, n:] = NAN
            cache.v[:, b, :, n:] = NAN
        ref.k[:, b, :, n:] = 0.0
        ref.v[:, b, :, n:] = 0.0
    cache.set_lens(torch.tensor(lens, device=cuda))
    ref.set_lens(torch.tensor(lens))
    return cache, ref


# every S and every pair of lengths at least once; S = 130 with the empty row and with the exact fit / overflow
CASES = [
    (2, [0, 129]),            # a partial wave; an empty row beside a filled one
    (16, [63, 64]),           # a full wave; the tile boundary
    (17, [1, 300]),           # a second wave with one query
    (17, [303, 308]),         # exact fit, and an overflow whose last 5 positions are dropped
    (64, [256, 261]),         # a full block; exact fit and overflow
    (64, [63, 64]),
    (65, [320, 7]),           # a second block with one query; a full row: every query sees all 320 keys
    (65, [255, 260]),
    (130, [0, 129]),          # three blocks
    (130, [190, 195]),
    (2, [320, 7]),
    (16, [304, 309]),
    (2, [318, 323]),          # exact fit; a length past the capacity is clamped to it
]


@pytest.mark.parametrize("S,lens", CASES, ids=[f"S{s}-{a}-{b}" for s, (a, b) in CASES])
def test_kernel_against_the_f32_reference(cuda, S, lens):
    """store + attend_chunk on a cache whose rows at and past lens[b] hold bf16 NaN before the store. The output is
    finite, one launch of the append kernel is counted, and per batch row the error against the f32 CPU reference is at
    most 1.5x that of the training forward on the same data (both printed). The forward's causal offset is Sk - Sq, so
    it is given the first Sk_b - len queries of a row (all of them unless the row overflows the cache); the queries of
    an overflowing row past those see every key of the cache and are compared with the non-causal forward."""
    cache, ref = filled_cache(cuda, lens, 100 * S + lens[0])
    qkv = torch.randn(B, S, 3 * H * 64, generator=torch.Generator().manual_seed(S)).to(BF)
    ref.store(0, qkv.float())
    want = ref.attend_chunk(0, qkv.float())                       # f32 [B, S, H*64]
    dq = qkv.to(cuda)
    cache.store(0, dq)
    before = launch_counts()
    got = cache.attend_chunk(0, dq)
    d = launch_delta(before)
    assert d["attn_append"] == 1 and sum(d.values()) == 1, d
    assert got.dtype == BF and tuple(got.shape) == (B, S, H * 64)
    got = got.float().cpu()
    assert torch.isfinite(got).all(), "a position at or past lens + S reached the output"
    q = dq[:, :, :H * 64].reshape(B, S, H, 64).transpose(1, 2)    # [B, H, S, 64]
    for b in range(B):
        n = min(lens[b], SMAX)
        skb = min(n + S, SMAX)
        ncmp = skb - n
        k, v = cache.k[0, b:b + 1, :, :skb], cache.v[0, b:b + 1, :, :skb]
        parts = []
        if ncmp > 0:
            parts.append(ops.attention(q[b:b + 1, :, :ncmp], k, v, causal=True))
        if ncmp < S:                                              # skb == SMAX: these queries see all of it
            parts.append(ops.attention(q[b:b + 1, :, ncmp:], k, v, causal=False))
        fwd = torch.cat(parts, 2)[0].transpose(0, 1).reshape(S, H * 64).float().cpu()
        e_fwd = (fwd - want[b]).abs().max().item()
        e_app = (got[b] - want[b]).abs().max().item()
        print(f"S {S} lens {lens[b]}: max |out - f32 reference| append {e_app:.6f}, training forward {e_fwd:.6f} "
              f"(ratio {e_app / max(e_fwd, 1e-30):.3f}, {ncmp} causal / {S - ncmp} overflowed queries)")
        assert e_app <= 1.5 * e_fwd, (b, e_app, e_fwd)


def test_lens_are_read_on_the_device_under_capture(cuda):
    """One captured store + attend_chunk (S = 17), replayed after set_lens to another pair of lengths with new qkv:
    the bits of the eager call on an identical cache. A launch that read lens on the host would replay the lengths of
    the capture."""
    S = 17
    cache, _ = filled_cache(cuda, [SMAX, SMAX], 7, poison=False)      # finite everywhere: any lens is valid
    cache.set_lens(torch.tensor([5, 200], device=cuda))

    def fn(qkv):
        cache.store(0, qkv)
        return cache.attend_chunk(0, qkv)

    step = graphs.CapturedStep(fn, split=False)
    g = torch.Generator().manual_seed(8)
    for _ in range(3):                                                # two eager warm-up calls, then the capture
        step(torch.randn(B, S, 3 * H * 64, generator=g).to(BF).to(cuda))
    assert step.captured
    new_lens = torch.tensor([131, 40], device=cuda)
    qkv = torch.randn(B, S, 3 * H * 64, generator=g).to(BF).to(cuda)
    cache.set_lens(new_lens)
    eager = ops.KVCache(1, B, H, SMAX, cuda, chunked=True)
    eager.k.copy_(cache.k)
    eager.v.copy_(cache.v)
    eager.set_lens(new_lens)
    before = launch_counts()
    got = step(qkv).clone()
    assert launch_delta(before)["attn_append"] == 0, "the call was not a replay"
    eager.store(0, qkv)
    want = eager.attend_chunk(0, qkv)
    torch.cuda.synchronize()
    assert torch.equal(bits(got), bits(want))
    assert torch.equal(bits(cache.k), bits(eager.k)) and torch.equal(bits(cache.v), bits(eager.v))
    # and the lengths matter: the capture's lengths give other bits on the same data
    eager.set_lens(torch.tensor([5, 200], device=cuda))
    eager.store(0, qkv)
    assert not torch.equal(bits(eager.attend_chunk(0, qkv)), bits(want))


def test_the_same_call_twice_gives_the_same_bits(cuda):
    S = 130
    cache, _ = filled_cache(cuda, [129, 60], 9)
    qkv = torch.randn(B, S, 3 * H * 64, generator=torch.Generator().manual_seed(10)).to(BF).to(cuda)
    cache.store(0, qkv)
    a = cache.attend_chunk(0, qkv)
    b = cache.attend_chunk(0, qkv)
    assert torch.equal(bits(a), bits(b))


def test_one_token_on_a_chunked_cache_is_attend(cuda):
    cache, _ = filled_cache(cuda, [129, 300], 11)
    qkv = torch.randn(B, 1, 3 * H * 64, generator=torch.Generator().manual_seed(12)).to(BF).to(cuda)
    cache.store(0, qkv)
    a = cache.attend(0, qkv)
    before = launch_counts()
    b = cache.attend_chunk(0, qkv)
    d = launch_delta(before)
    assert d["attn_decode"] == 1 and d["attn_append"] == 0 and sum(d.values()) == 1, d
    assert torch.equal(bits(a), bits(b))


def test_the_route_is_opt_in(cuda, models):
    """A default KVCache / new_cache on the GPU still raises for S > 1 and stores nothing (the behaviour pinned by
    tests/test_extend_gpu.py, restated next to the new route); another head dim raises ValueError as before."""
    gpu, _ = models
    cache = ops.KVCache(1, B, H, SMAX, cuda)
    assert not cache.chunked
    cache.k.zero_()
    cache.v.zero_()
    k, v = cache.k.clone(), cache.v.clone()
    with pytest.raises(NotImplementedError):
        cache.attend_chunk(0, torch.ones(B, 4, 3 * H * 64, device=cuda, dtype=BF))
    assert torch.equal(bits(cache.k), bits(k)) and torch.equal(bits(cache.v), bits(v))
    with pytest.raises(ValueError):
        ops.KVCache(1, B, H, SMAX, cuda, head_dim=32, chunked=True)
    torch.manual_seed(2)
    seq = torch.randint(0, VOCAB, (2, 12), device=cuda)
    with context.device(cuda), torch.no_grad():
        plain = gpu.new_cache(2, 12, cuda)
        assert not plain.chunked and gpu.new_cache(2, 12, cuda, chunked=True).chunked
        gpu.extend(seq[:, :7], plain)
        k, v = plain.k.clone(), plain.v.clone()
        with pytest.raises(NotImplementedError):
            gpu.extend(seq[:, 7:], plain)
        with pytest.raises(NotImplementedError):
            gpu.generate(seq[:, 7:], 0, cache=plain, prefill_chunk=2)
    assert plain.lens.tolist() == [7, 7]
    assert torch.equal(bits(plain.k), bits(k)) and torch.equal(bits(plain.v), bits(v)), "a refused call stored K/V"


# ---------------------------------------------------------------------------------------------------- model level
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


def poisoned_cache(gpu, batch, capacity, cuda):
    cache = gpu.new_cache(batch, capacity, cuda, chunked=True)
    cache.k.fill_(NAN)
    cache.v.fill_(NAN)
    return cache


@pytest.fixture(scope="module")
def extend_reference(cuda, models):
    """29 tokens per row; logits at positions 4 .. 28 of the f32 CPU model and of the GPU full forward."""
    gpu, cpu = models
    torch.manual_seed(1)
    seq = torch.randint(0, VOCAB, (2, 29))
    with context.device("cpu"), torch.no_grad():
        ref = cpu(seq, training=False).float()[:, 4:, :VOCAB]
    with context.device(cuda), torch.no_grad():
        full = gpu(seq.to(cuda), training=False).float()[:, 4:, :VOCAB].cpu()
    return seq, ref, full


@pytest.mark.parametrize("chunk", [2, 6, None])
def test_extend_in_chunks_tracks_the_full_forward(cuda, models, extend_reference, chunk):
    """5 tokens into the empty cache (all NaN before), then the next 24 in pieces of `chunk`. The returned logits (and
    for chunk=6 the logits after each piece, fed as four calls) against the f32 CPU reference stay within 1.5x of the
    error of the GPU full forward on the same positions."""
    gpu, _ = models
    seq, ref, full = extend_reference
    dseq = seq.to(cuda)
    with context.device(cuda), torch.no_grad():
        cache = poisoned_cache(gpu, 2, 29, cuda)
        gpu.extend(dseq[:, :5], cache)
        if chunk == 6:
            pos = [lo + 5 for lo in range(5, 29, 6)]
            got = [gpu.extend(dseq[:, lo:lo + 6], cache) for lo in range(5, 29, 6)]
            for p, lg in zip(pos, got):
                assert torch.isfinite(lg.float()).all()
                e_full = (full[:, p - 4] - ref[:, p - 4]).abs().max().item()
                e_ext = (lg.float()[:, :VOCAB].cpu() - ref[:, p - 4]).abs().max().item()
                print(f"chunk 6, after the piece ending at {p}: full forward {e_full:.5f}, extend {e_ext:.5f}")
                assert e_ext <= 1.5 * e_full, (p, e_ext, e_full)
            other = poisoned_cache(gpu, 2, 29, cuda)
            gpu.extend(dseq[:, :5], other)
            last = gpu.extend(dseq[:, 5:], other, chunk=6)            # the same pieces in one call: the same bits
            assert torch.equal(bits(last), bits(got[-1]))
            assert other.lens.tolist() == [29, 29]
        else:
            last = gpu.extend(dseq[:, 5:], cache, chunk=chunk)
    assert cache.lens.tolist() == [29, 29]
    assert torch.isfinite(last.float()).all()
    e_full = (full[:, -1] - ref[:, -1]).abs().max().item()
    e_ext = (last.float()[:, :VOCAB].cpu() - ref[:, -1]).abs().max().item()
    print(f"chunk {chunk}: max |logits at 28 - f32 CPU reference| full forward {e_full:.5f}, extend {e_ext:.5f} "
          f"(ratio {e_ext / e_full:.3f}, logit scale {ref.abs().max():.3f})")
    assert e_ext <= 1.5 * e_full, (e_ext, e_full)


@pytest.mark.parametrize("chunk", [None, 3])
def test_ragged_rows_near_the_context_end_in_chunks(cuda, models, chunk):
    """The near-ctx scenario of tests/test_extend_gpu.py on the chunked route: the new_lens=[0, 2] piece, then the
    4-token piece whose pad positions run past the position table. Finite, and within 1.5x of the error of the same
    tokens fed without padding through the same route."""
    gpu, cpu = models
    torch.manual_seed(5)
    seq = torch.randint(0, VOCAB, (2, CTX))
    pad = 199
    with context.device("cpu"), torch.no_grad():
        ref = cpu(seq, training=False).float()[:, -1, :VOCAB]
    dseq = seq.to(cuda)
    with context.device(cuda), torch.no_grad():
        plain = poisoned_cache(gpu, 2, CTX, cuda)
        gpu.extend(dseq[:, :CTX - 4], plain)
        want = gpu.extend(dseq[:, CTX - 4:], plain, chunk=chunk)
        cache = poisoned_cache(gpu, 2, CTX, cuda)
        gpu.extend(dseq[:, :CTX - 4], cache)
        gpu.extend(dseq[:, CTX - 4:CTX - 2], cache, new_lens=torch.tensor([0, 2]), chunk=chunk)  # row 0 takes nothing
        assert cache.lens.tolist() == [CTX - 4, CTX - 2]
        new = torch.full((2, 4), pad, device=cuda)
        new[0] = dseq[0, CTX - 4:]
        new[1, :2] = dseq[1, CTX - 2:]
        got = gpu.extend(new, cache, new_lens=torch.tensor([4, 2]), chunk=chunk)
        torch.cuda.synchronize()
    assert cache.lens.tolist() == [CTX, CTX] and plain.lens.tolist() == [CTX, CTX]
    err_plain = (want.float()[:, :VOCAB].cpu() - ref).abs().max().item()
    err_ragged = (got.float()[:, :VOCAB].cpu() - ref).abs().max().item()
    print(f"chunk {chunk}: max |last logits - f32 CPU reference| unpadded {err_plain:.5f}, ragged {err_ragged:.5f} "
          f"(logit scale {ref.abs().max():.3f})")
    assert torch.isfinite(got.float()).all()
    assert err_ragged <= 1.5 * err_plain, (err_ragged, err_plain)


def test_generate_on_a_chunked_cache_graph_replay_equals_eager_steps(cuda, models):
    gpu, _ = models
    torch.manual_seed(3)
    first = torch.randint(1, VOCAB, (2, 7), device=cuda)
    new_ids = torch.randint(1, VOCAB, (2, 4), device=cuda)
    res = {}
    with context.device(cuda):
        for graph in (True, False):
            cache = poisoned_cache(gpu, 2, 7 + 4 + 6, cuda)
            gpu.extend(first, cache, new_lens=torch.tensor([7, 5]))   # equal starting caches, ragged
            with call_log() as c:
                out = gpu.generate(new_ids, 6, cache=cache, prefill_chunk=4, graph=graph)
            assert c["dtf_attn_append"] == CFG["layers"], c          # the 4 new tokens went in as one piece
            res[graph] = (out, gpu.last_generation)
    (a, ga), (b, gb) = res[True], res[False]
    assert ga["step"] is not None and ga["step"].captured, "the one-token step was not captured"
    assert gb["step"] is None
    assert tuple(a.shape) == (2, 4 + 6) and torch.equal(a[:, :4], new_ids)
    assert torch.equal(a, b)
    assert torch.isfinite(ga["logits"].float()).all()
    assert torch.equal(ga["logits"].view(torch.int16), gb["logits"].view(torch.int16))
    assert ga["cache"].lens.tolist() == gb["cache"].lens.tolist() == [17, 15]


def test_generate_with_prefill_chunk_and_no_cache_runs_on_the_gpu(cuda, models):
    """generate(ids, 4, prefill_chunk=3) builds a chunked cache itself; the logits after the last token against the f32
    CPU model fed the same tokens stay within 1.5x of the error of the GPU full forward on them."""
    gpu, cpu = models
    torch.manual_seed(6)
    ids = torch.randint(1, VOCAB, (2, 8))
    with context.device(cuda), torch.no_grad():
        with call_log() as c:
            out = gpu.generate(ids.to(cuda), 4, prefill_chunk=3)
        lg = gpu.last_generation["logits"].float()[:, :VOCAB].cpu()
        assert gpu.last_generation["cache"].chunked
        full = gpu(out, training=False).float()[:, -1, :VOCAB].cpu()
    assert c["dtf_attn_append"] == 2 * CFG["layers"], c              # pieces of 3, 3, 2: two behind a filled cache
    assert tuple(out.shape) == (2, 12) and torch.equal(out[:, :8].cpu(), ids)
    with context.device("cpu"), torch.no_grad():
        ref = cpu(out.cpu(), training=False).float()[:, -1, :VOCAB]
    e_full = (full - ref).abs().max().item()
    e_gen = (lg - ref).abs().max().item()
    print(f"max |logits after the last token - f32 CPU reference|: full forward {e_full:.5f}, generate {e_gen:.5f}")
    assert torch.isfinite(lg).all()
    assert e_gen <= 1.5 * e_full, (e_gen, e_full)


def test_a_chunked_extend_reaches_the_append_kernel(cuda, models):
    gpu, _ = models
    torch.manual_seed(4)
    seq = torch.randint(0, VOCAB, (2, 11), device=cuda)
    with context.device(cuda), torch.no_grad():
        cache = poisoned_cache(gpu, 2, 11, cuda)
        gpu.extend(seq[:, :5], cache)
        before = launch_counts()
        with call_log() as c:
            gpu.extend(seq[:, 5:], cache)
        d = launch_delta(before)
    assert c["dtf_attn_append"] == 2 and c["dtf_attn_decode"] == 0, c
    assert d["attn_append"] == 2 and d["attn_decode"] == 0, d
    assert cache.lens.tolist() == [11, 11]
