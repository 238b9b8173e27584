"""Continuing a filled KV cache on the GPU (bf16). Behind a filled cache the GPU feeds single tokens (the decode
step's kernels); a multi-token piece there has no kernel and must raise before the cache is touched, never fall back.
The tiny model and the error measure are those of tests/test_generate_gpu.py."""
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2

pytestmark = pytest.mark.gpu
VOCAB, CTX = 200, 96
CFG = dict(vocab=VOCAB, ctx=CTX, hidden=128, layers=2, heads=2)
BF = torch.bfloat16


def bits(t):
    return t.contiguous().view(torch.int16)


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


def test_extend_token_by_token_tracks_the_full_forward(cuda, models):
    """extend: 5 tokens into the empty cache, then 24 single tokens, then the same 24 again as four 6-token calls
    with chunk=1 on a second cache. Each position's logits against the f32 CPU reference must stay within 1.5x of the
    error of the full-forward GPU path on the same positions, and the 6-token calls return the bits of the single
    calls (the same kernels in the same order)."""
    gpu, cpu = models
    torch.manual_seed(1)
    seq = torch.randint(0, VOCAB, (2, 29))
    with context.device("cpu"), torch.no_grad():
        ref = cpu(seq, training=False).float()[:, 4:, :VOCAB]
    dseq = seq.to(cuda)
    with context.device(cuda), torch.no_grad():
        full = gpu(dseq, training=False).float()[:, 4:, :VOCAB].cpu()
        cache = gpu.new_cache(2, 29, cuda)
        got = [gpu.extend(dseq[:, :5], cache)]                        # empty cache: the prefill kernel
        for t in range(5, 29):
            got.append(gpu.extend(dseq[:, t:t + 1], cache))
        other = gpu.new_cache(2, 29, cuda)
        gpu.extend(dseq[:, :5], other)
        for lo in range(5, 29, 6):
            lg = gpu.extend(dseq[:, lo:lo + 6], other, chunk=1)
            assert torch.equal(bits(lg), bits(got[lo + 5 - 4])), f"6-token call at {lo} differs from single calls"
        ext = torch.stack(got, 1).float()[:, :, :VOCAB].cpu()
    assert tuple(ext.shape) == tuple(ref.shape)
    err_full = (full - ref).abs().max().item()
    err_ext = (ext - ref).abs().max().item()
    print(f"max |logits - f32 CPU reference| over 25 positions: full forward {err_full:.5f}, extend {err_ext:.5f} "
          f"(ratio {err_ext / err_full:.3f}, logit scale {ref.abs().max():.3f})")
    assert err_ext <= 1.5 * err_full, (err_ext, err_full)
    assert cache.lens.tolist() == [29, 29] and other.lens.tolist() == [29, 29]


def test_ragged_rows_near_the_context_end_token_by_token(cuda, models):
    """The CPU file's near-ctx scenario on the route the GPU has (chunk=1): row 1 is full two pieces before row 0, so
    its pad tokens are embedded at position ctx, which must be clamped to the table (no read past it, no exception).
    Both rows' last logits against the f32 CPU reference must stay within 1.5x of the error of the same tokens fed
    without padding through the same kernels (both errors printed)."""
    gpu, cpu = models
    torch.manual_seed(5)
    seq = torch.randint(0, VOCAB, (2, CTX))
    pad = 199
    with context.device("cpu"), torch.no_grad():
        ref = cpu(seq, training=False).float()[:, -1, :VOCAB]
    dseq = seq.to(cuda)
    with context.device(cuda), torch.no_grad():
        plain = gpu.new_cache(2, CTX, "cuda")                          # 'cuda' is the current device, cuda:0
        gpu.extend(dseq[:, :CTX - 4], plain)
        want = gpu.extend(dseq[:, CTX - 4:], plain, chunk=1)
        cache = gpu.new_cache(2, CTX, cuda)
        gpu.extend(dseq[:, :CTX - 4], cache)
        gpu.extend(dseq[:, CTX - 4:CTX - 2], cache, new_lens=torch.tensor([0, 2]), chunk=1)   # row 0 takes nothing
        assert cache.lens.tolist() == [CTX - 4, CTX - 2]
        new = torch.full((2, 4), pad, device=cuda)
        new[0] = dseq[0, CTX - 4:]
        new[1, :2] = dseq[1, CTX - 2:]
        got = gpu.extend(new, cache, new_lens=torch.tensor([4, 2]), chunk=1)
        torch.cuda.synchronize()
    assert cache.lens.tolist() == [CTX, CTX] and plain.lens.tolist() == [CTX, CTX]
    err_plain = (want.float()[:, :VOCAB].cpu() - ref).abs().max().item()
    err_ragged = (got.float()[:, :VOCAB].cpu() - ref).abs().max().item()
    print(f"max |last logits - f32 CPU reference|: unpadded {err_plain:.5f}, ragged {err_ragged:.5f} "
          f"(logit scale {ref.abs().max():.3f})")
    assert torch.isfinite(got.float()).all()
    assert err_ragged <= 1.5 * err_plain, (err_ragged, err_plain)


def test_a_multi_token_piece_behind_a_filled_cache_raises_and_changes_nothing(cuda, models):
    gpu, _ = models
    torch.manual_seed(2)
    seq = torch.randint(0, VOCAB, (2, 12), device=cuda)
    with context.device(cuda), torch.no_grad():
        cache = gpu.new_cache(2, 12, cuda)
        gpu.extend(seq[:, :7], cache)
        k, v = cache.k.clone(), cache.v.clone()
        with pytest.raises(NotImplementedError):
            gpu(seq[:, 7:], training=False, cache=cache, append=True)
        with pytest.raises(NotImplementedError):
            gpu.extend(seq[:, 7:], cache)
        with pytest.raises(NotImplementedError):
            gpu.extend(seq[:, 7:], cache, chunk=2)
        with pytest.raises(NotImplementedError):
            gpu.generate(seq[:, 7:], 0, cache=cache)
        with pytest.raises(NotImplementedError):   # the default keeps its parent behaviour (and message class)
            gpu(seq[:, 7:], training=False, cache=cache)
        fresh = gpu.new_cache(2, 12, cuda)
        with pytest.raises(NotImplementedError):   # an empty cache takes one multi-token piece, not two
            gpu.extend(seq, fresh, chunk=5)
        assert fresh.empty and fresh.lens.tolist() == [0, 0]
    assert cache.lens.tolist() == [7, 7]
    assert torch.equal(bits(cache.k), bits(k)) and torch.equal(bits(cache.v), bits(v)), "a refused call stored K/V"


def test_attend_chunk_on_the_gpu(cuda):
    """One query per row is `attend` (same kernel, same bits); more raise; bad arguments raise ValueError first."""
    from distributed_tensorflow_amd.ops._util import launch_counts, launch_delta
    B, H, Smax = 2, 3, 320
    torch.manual_seed(3)
    cache = ops.KVCache(1, B, H, Smax, cuda)
    cache.k.copy_(torch.randn(cache.k.shape, device=cuda))
    cache.v.copy_(torch.randn(cache.v.shape, device=cuda))
    cache.set_lens(torch.tensor([129, 300], device=cuda))
    qkv = torch.randn(B, 1, 3 * H * 64, device=cuda).to(BF)
    cache.store(0, qkv)
    a = cache.attend(0, qkv)
    before = launch_counts()
    b = cache.attend_chunk(0, qkv)
    d = launch_delta(before)
    assert d["attn_decode"] == 1 and sum(d.values()) == 1, d
    assert torch.equal(bits(a), bits(b))
    good = torch.zeros(B, 4, 3 * H * 64, device=cuda, dtype=BF)
    with pytest.raises(NotImplementedError):
        cache.attend_chunk(0, good)
    with pytest.raises(ValueError):
        cache.attend_chunk(0, good[:1])                       # wrong batch
    with pytest.raises(ValueError):
        cache.attend_chunk(0, good[:, :, :3 * 2 * 64])        # wrong width
    for layer in (1, -1):
        with pytest.raises(ValueError):
            cache.attend_chunk(layer, good)                   # no such layer


def test_generate_on_a_cache_graph_replay_equals_eager_steps(cuda, models):
    gpu, _ = models
    torch.manual_seed(3)
    first = torch.randint(1, VOCAB, (2, 7), device=cuda)
    new_ids = torch.randint(1, VOCAB, (2, 4), device=cuda)
    res = {}
    with context.device(cuda):
        for graph in (True, False):
            cache = gpu.new_cache(2, 7 + 4 + 6, cuda)
            gpu.extend(first, cache, new_lens=torch.tensor([7, 5]))   # equal starting caches, ragged
            out = gpu.generate(new_ids, 6, cache=cache, prefill_chunk=1, graph=graph)
            res[graph] = (out, gpu.last_generation)
    (a, ga), (b, gb) = res[True], res[False]
    assert ga["step"] is not None and ga["step"].captured, "the one-token step was not captured"
    assert gb["step"] is None
    assert tuple(a.shape) == (2, 4 + 6) and torch.equal(a[:, :4], new_ids)
    assert torch.equal(a, b)
    assert torch.equal(ga["logits"].view(torch.int16), gb["logits"].view(torch.int16))
    assert ga["cache"].lens.tolist() == gb["cache"].lens.tolist() == [17, 15]
