"""The fp8 KV cache on the GPU (csrc/kernels/attn_decode_fp8.hip, attn_append_kernel<true>) and generate(kv_dtype="fp8").
close(a, b, tol) is max |a-b| <= tol * max |b|; ATTN_TOL is that of tests/test_decode_gpu.py."""
import pytest
import torch

from _fp8ref import NAN_CODE, assert_bytes
from test_kv_fp8 import edge_rows
from test_generate_gpu import models  # noqa: F401  (the tiny GPT-2 on the GPU and its f32 CPU copy)
from distributed_tensorflow_amd import context
from distributed_tensorflow_amd.ops._util import launch_counts, launch_delta
from distributed_tensorflow_amd.ops.decode import KVCache, decode_chunk, kv_quantize_reference

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ATTN_TOL = 2e-2
VOCAB = 200
CFG = dict(vocab=VOCAB, ctx=96, hidden=128, layers=2, heads=2)  # of tests/test_generate_gpu.py


def close(a, b, tol):
    err, ref = (a.double() - b.double()).abs().max().item(), b.double().abs().max().item() + 1e-6
    assert err <= tol * ref, f"max err {err} vs ref scale {ref} (tol {tol})"


def _poisoned(dev, B, H, Smax, keep, K=None, V=None, chunked=False):
    """A one-layer fp8 cache holding K, V [B, H, Smax, 64] (one multi-token store) when given; everything at and past
    row keep[b] is then poisoned (NaN codes, NaN scales) and lens is set to keep."""
    cache = KVCache(1, B, H, Smax, dev, chunked=chunked, kv_dtype="fp8")
    assert cache.capacity == Smax and cache.k.dtype == torch.uint8 and cache.k_scale.shape == (1, B, H, Smax)
    if K is not None:  # qkv [B, Smax, 3*H*64] with a zero query third
        rows = [t.permute(0, 2, 1, 3).reshape(B, Smax, H * 64) for t in (torch.zeros_like(K), K, V)]
        cache.store(0, torch.cat(rows, -1).to(BF).to(dev))
    for b in range(B):
        for codes, sc in ((cache.k, cache.k_scale), (cache.v, cache.v_scale)):
            codes[0, b, :, keep[b]:] = NAN_CODE
            sc[0, b, :, keep[b]:] = float("nan")
    cache.set_lens(torch.tensor(keep, device=dev))
    return cache


def _poison_intact(cache, n):
    for b in range(cache.batch):
        assert (cache.k[0, b, :, n[b]:] == NAN_CODE).all() and (cache.v[0, b, :, n[b]:] == NAN_CODE).all()
        assert cache.k_scale[0, b, :, n[b]:].isnan().all() and cache.v_scale[0, b, :, n[b]:].isnan().all()


def _ref_attend(q, cache, n, scale=0.125):
    """float64 softmax(q K^T scale) V over the first n[b] dequantized rows of layer 0. q [B, H, 64] -> [B, H, 64]."""
    K, V = (t.double() for t in cache.dequantized(0))
    out = torch.empty(q.shape, dtype=torch.float64, device=q.device)
    for b in range(q.shape[0]):
        s = torch.einsum("hd,hsd->hs", q[b].double(), K[b, :, :n[b]]) * scale
        out[b] = torch.einsum("hs,hsd->hd", torch.softmax(s, -1), V[b, :, :n[b]])
    return out


@pytest.mark.parametrize("S,lens", [(1, [0, 70]), (5, [0, 70]), (2, [127, 128])])
def test_store_is_byte_exact_and_writes_nothing_else(cuda, S, lens):
    B, H, Smax = 2, 3, 128
    torch.manual_seed(S)
    x = torch.randn(B, S, 3, H, 64).to(BF)
    e = edge_rows().to(BF)
    x[0, 0, 1, 0], x[0, 0, 1, 1], x[0, 0, 2, 2], x[1, 0, 1, 0] = e[0], e[1], e[2], e[3]
    cache = _poisoned(cuda, B, H, Smax, [0, 0])
    cache.set_lens(torch.tensor(lens, device=cuda))
    want = [t[0].cpu().clone() for t in (cache.k, cache.k_scale, cache.v, cache.v_scale)]
    for b in range(B):
        for s in range(S):
            if lens[b] + s < Smax:
                for third in (1, 2):
                    c, sc = kv_quantize_reference(x[b, s, third])
                    want[2 * third - 2][b, :, lens[b] + s], want[2 * third - 1][b, :, lens[b] + s] = c, sc
    cache.store(0, x.reshape(B, S, -1).to(cuda))
    got = [t[0].cpu() for t in (cache.k, cache.k_scale, cache.v, cache.v_scale)]
    for name, g, w in zip(("K", "V"), got[::2], want[::2]):
        assert_bytes(name, g, w, 0)
    for g, w in zip(got[1::2], want[1::2]):
        assert torch.equal(g.view(torch.int32), w.view(torch.int32)), "scales differ / other scales written"
    assert cache.lens.tolist() == lens


def _length_sets(B, Smax):
    c = decode_chunk()
    want = list(dict.fromkeys(n for n in (1, c - 1, c, c + 1, Smax - 1, Smax, 2 * c, 2 * c + 1, Smax // 2)
                              if 1 <= n <= Smax))
    return [(want[i:i + B] + [want[-1]] * B)[:B] for i in range(0, len(want), B)]


@pytest.mark.parametrize("B,H,Smax", [(2, 3, 320), (1, 1, 64), (5, 2, 128)])
def test_decode_matches_float64_over_the_stored_bytes(cuda, B, H, Smax):
    g = torch.Generator().manual_seed(Smax)
    rowscale = 2.0 ** ((torch.arange(Smax) % 3) - 1.0)[:, None]
    K, V = (torch.randn(B, H, Smax, 64, generator=g) * rowscale for _ in range(2))
    for n_after in _length_sets(B, Smax):
        cache = _poisoned(cuda, B, H, Smax, [n - 1 for n in n_after], K, V)
        qkv = torch.randn(B, 1, 3 * H * 64, generator=g).to(BF).to(cuda)
        cache.store(0, qkv)
        out = cache.attend(0, qkv)
        assert out.dtype == BF and tuple(out.shape) == (B, 1, H * 64) and torch.isfinite(out.float()).all(), n_after
        close(out.view(B, H, 64), _ref_attend(qkv.view(B, 3, H, 64)[:, 0], cache, n_after), ATTN_TOL)
        _poison_intact(cache, n_after)


def test_decode_dominant_key_returns_its_value_row(cuda):
    B, H, Smax, hot = 2, 3, 320, [[3, 200, 131], [127, 128, 255]]
    torch.manual_seed(5)
    K, V = torch.randn(B, H, Smax, 64) * 0.1, torch.randn(B, H, Smax, 64)
    qkv = torch.randn(B, 1, 3 * H * 64).to(BF)
    q = qkv.view(B, 3, H, 64)[:, 0].float()
    for b in range(B):
        for h in range(H):
            K[b, h, hot[b][h]] = q[b, h] * 8.0
            V[b, h, hot[b][h] - 1] *= 4.0
            V[b, h, hot[b][h] + 1] *= 0.25
    cache = _poisoned(cuda, B, H, Smax, [300, 281], K, V)
    cache.set_lens(torch.tensor([299, 280], device=cuda))
    out = cache.attend(0, qkv.to(cuda)).view(B, H, 64).float()
    Vd = cache.dequantized(0)[1]
    for b in range(B):
        for h in range(H):
            want = Vd[b, h, hot[b][h]]
            assert ((out[b, h] - want).abs() <= 2.0 ** -7 * want.abs() + 1e-30).all(), (b, h)


def test_decode_full_cache_repeat_and_counters(cuda):
    B, H, Smax = 2, 2, 128
    torch.manual_seed(6)
    cache = _poisoned(cuda, B, H, Smax, [Smax, Smax], torch.randn(B, H, Smax, 64), torch.randn(B, H, Smax, 64))
    cache.set_lens(torch.tensor([Smax, Smax + 5], device=cuda))
    qkv = torch.randn(B, 1, 3 * H * 64, device=cuda).to(BF)
    before = [t.clone() for t in (cache.k, cache.v, cache.k_scale, cache.v_scale)]
    cache.store(0, qkv)
    assert all(torch.equal(a, b) for a, b in zip(before, (cache.k, cache.v, cache.k_scale, cache.v_scale)))
    counts = launch_counts()
    a = cache.attend(0, qkv)
    d = launch_delta(counts)
    assert d["attn_decode_fp8"] == 1 and d["attn_decode"] == 0 and sum(d.values()) == 1, d
    assert torch.equal(a.view(torch.int16), cache.attend(0, qkv).view(torch.int16))
    close(a.view(B, H, 64), _ref_attend(qkv.view(B, 3, H, 64)[:, 0], cache, [Smax, Smax]), ATTN_TOL)


@pytest.mark.parametrize("lens", [[1, 130], [64, 186]])
@pytest.mark.parametrize("S", [2, 17, 64, 70])
def test_append_is_bitwise_the_bf16_kernel_on_the_dequantized_cache(cuda, S, lens):
    B, H, Smax = 2, 2, 256
    torch.manual_seed(S + lens[0])
    cache = _poisoned(cuda, B, H, Smax, lens, torch.randn(B, H, Smax, 64), torch.randn(B, H, Smax, 64) * 3, chunked=True)
    qkv = torch.randn(B, S, 3 * H * 64, device=cuda).to(BF)
    cache.store(0, qkv)
    _poison_intact(cache, [min(n + S, Smax) for n in lens])
    plain = KVCache(1, B, H, Smax, cuda, chunked=True)
    for dst, deq in zip((plain.k, plain.v), cache.dequantized(0)):
        assert ((deq.to(BF).float() == deq) | deq.isnan()).all(), "dequantized values are not exact in bf16"
        dst[0] = deq.to(BF)
    plain.set_lens(cache.lens)
    counts = launch_counts()
    got = cache.attend_chunk(0, qkv)
    assert launch_delta(counts)["attn_append_fp8"] == 1
    assert torch.equal(got.view(torch.int16), plain.attend_chunk(0, qkv).view(torch.int16))


def test_generate_routes_graph_replay_and_chunked_prefill(cuda, models):  # noqa: F811
    gpu, _ = models
    torch.manual_seed(3)
    ids = torch.randint(1, VOCAB, (2, 5), device=cuda)
    with context.device(cuda), torch.no_grad():
        a = gpu.generate(ids, 8, kv_dtype="fp8", graph=True)
        ga = gpu.last_generation
        b = gpu.generate(ids, 8, kv_dtype="fp8", graph=False)
        gb = gpu.last_generation
        assert ga["step"] is not None and ga["step"].captured and gb["step"] is None
        assert torch.equal(a, b) and torch.equal(ga["logits"].view(torch.int16), gb["logits"].view(torch.int16))
        assert gb["cache"].kv_dtype == "fp8" and gb["cache"].k.dtype == torch.uint8
        gb["cache"].set_lens(torch.tensor([12, 12], device=cuda))
        counts = launch_counts()
        gpu(a[:, 12:13].contiguous(), training=False, cache=gb["cache"])
        d = launch_delta(counts)
        assert d["attn_decode_fp8"] == CFG["layers"] and d["attn_decode"] == 0, d
        counts = launch_counts()
        c = gpu.generate(torch.cat([ids, ids + 1, ids[:, :1]], 1) % VOCAB, 8, kv_dtype="fp8", prefill_chunk=4)  # 4 + 4 + 3
        assert launch_delta(counts)["attn_append_fp8"] > 0 and tuple(c.shape) == (2, 19)


class _Bf16Store(KVCache):
    def store(self, layer, qkv):  # the CPU fp8 cache fed what a bf16 projection would hand it
        super().store(layer, qkv.to(BF).float())


def _teacher_forced(model, dev, seq, cache):
    """Prefill 5 tokens, feed the other 24 through the cached step -> their logits [2, 24, VOCAB] on the CPU."""
    seq = seq.to(dev)
    with context.device(dev), torch.no_grad():
        model(seq[:, :5], training=False, cache=cache)
        cache.advance(5)
        steps = []
        for t in range(5, 29):
            steps.append(model(seq[:, t:t + 1].contiguous(), training=False, cache=cache))
            cache.advance(1)
    return torch.cat(steps, 1).float()[:, :, :VOCAB].cpu()


def test_teacher_forced_logits_track_the_cpu_fp8_cache(cuda, models):  # noqa: F811
    """err_bf16: the bf16-cache GPU path against the CPU reference; err_flip: how far the CPU fp8 reference itself moves
    when the K/V it stores are first rounded to bf16 (one-code flips). Neither involves the new kernels."""
    gpu, cpu = models
    torch.manual_seed(1)
    seq = torch.randint(0, VOCAB, (2, 29))
    ref16 = _teacher_forced(cpu, "cpu", seq, cpu.new_cache(2, 29, "cpu"))
    ref8 = _teacher_forced(cpu, "cpu", seq, cpu.new_cache(2, 29, "cpu", kv_dtype="fp8"))
    flip = _teacher_forced(cpu, "cpu", seq, _Bf16Store(CFG["layers"], 2, CFG["heads"], 29, "cpu", kv_dtype="fp8"))
    err_bf16 = (_teacher_forced(gpu, cuda, seq, gpu.new_cache(2, 29, cuda)) - ref16).abs().max().item()
    err_fp8 = (_teacher_forced(gpu, cuda, seq, gpu.new_cache(2, 29, cuda, kv_dtype="fp8")) - ref8).abs().max().item()
    err_flip = (flip - ref8).abs().max().item()
    print(f"max |logits - CPU reference| over 24 positions: fp8 cache {err_fp8:.5f}, bf16 cache {err_bf16:.5f}, "
          f"CPU fp8 reference moved by bf16-rounded K/V {err_flip:.5f} (logit scale {ref8.abs().max():.3f})")
    assert err_flip > 0
    assert err_fp8 <= 1.5 * (err_bf16 + err_flip), (err_fp8, err_bf16, err_flip)


def test_refusals_leave_the_cache_untouched(cuda, models):  # noqa: F811
    gpu, _ = models
    ids = torch.randint(1, VOCAB, (2, 5), device=cuda)
    with context.device(cuda):
        plain, fp8 = gpu.new_cache(2, 16, cuda), gpu.new_cache(2, 16, cuda, kv_dtype="fp8")
        for kw in (dict(kv_dtype="int8"), dict(kv_dtype="fp8", step="fused"), dict(kv_dtype="fp8", cache=plain)):
            with pytest.raises(ValueError):
                gpu.generate(ids, 4, **kw)
        with pytest.raises(ValueError):
            fp8.attend(0, torch.zeros(2, 1, 3 * 128, device=cuda, dtype=BF), fused=True)
    assert plain.empty and fp8.empty and plain.lens.tolist() == [0, 0] and fp8.lens.tolist() == [0, 0]
