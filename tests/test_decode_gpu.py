"""Decode kernels (csrc/kernels/attn_decode.hip): KV-cache append, split-KV single-token attention and the M <= 16
weight-streaming dense layer, against f32 references.

close(a, b, tol) is max |a-b| <= tol * max |b|, the form of tests/test_attention.py and tests/test_kernels_gpu.py.
"""
import math

import pytest
import torch

from distributed_tensorflow_amd import ops

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ATTN_TOL = 2e-2    # forward tolerance of tests/test_attention.py
DENSE_TOL = 1e-2   # the project's bf16-epilogue tolerance


def close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max err {err} vs ref scale {ref} (tol {tol})"


def bits(t):
    return t.contiguous().view(torch.int16)


def _guarded_cache(B, H, Smax, dev, fill=None):
    """A KVCache (one layer) whose K and V live inside one larger tensor with guard regions before, between and
    after them. Returns (cache, whole buffer)."""
    n = B * H * Smax * 64
    G = 4096
    whole = torch.randn(3 * G + 2 * n, device=dev).to(BF)
    if fill is not None:
        whole.fill_(fill)
    cache = ops.KVCache(1, B, H, Smax, dev)
    assert cache.capacity == Smax
    cache.k = whole[G:G + n].view(1, B, H, Smax, 64)
    cache.v = whole[2 * G + n:2 * G + 2 * n].view(1, B, H, Smax, 64)
    return cache, whole


# ---------------------------------------------------------------------------------------------- kv_store
@pytest.mark.parametrize("S", [1, 5])
def test_kv_store_rows_and_nothing_else(cuda, S):
    B, H, Smax = 2, 3, 128
    torch.manual_seed(S)
    cache, whole = _guarded_cache(B, H, Smax, cuda)
    lens = [0, 70]
    cache.set_lens(torch.tensor(lens, device=cuda))
    qkv = torch.randn(B, S, 3 * H * 64, device=cuda).to(BF)
    before = whole.clone()
    kview, vview = cache.k.clone(), cache.v.clone()
    cache.store(0, qkv)
    x = qkv.view(B, S, 3, H, 64)
    for b in range(B):
        kview[0, b, :, lens[b]:lens[b] + S] = x[b, :, 1].transpose(0, 1)
        vview[0, b, :, lens[b]:lens[b] + S] = x[b, :, 2].transpose(0, 1)
    assert torch.equal(bits(cache.k), bits(kview)), "K rows differ from the source slices / other K bytes changed"
    assert torch.equal(bits(cache.v), bits(vview)), "V rows differ from the source slices / other V bytes changed"
    n, G = B * H * Smax * 64, 4096
    for lo, hi in ((0, G), (G + n, 2 * G + n), (2 * G + 2 * n, 3 * G + 2 * n)):
        assert torch.equal(bits(whole[lo:hi]), bits(before[lo:hi])), "guard region written"
    assert cache.lens.tolist() == lens, "store must not change lens"


def test_kv_store_drops_positions_past_capacity(cuda):
    B, H, Smax, S = 2, 3, 128, 2
    torch.manual_seed(3)
    cache, whole = _guarded_cache(B, H, Smax, cuda)
    cache.set_lens(torch.tensor([127, 128], device=cuda))
    qkv = torch.randn(B, S, 3 * H * 64, device=cuda).to(BF)
    before = whole.clone()
    kview, vview = cache.k.clone(), cache.v.clone()
    cache.store(0, qkv)
    x = qkv.view(B, S, 3, H, 64)
    kview[0, 0, :, 127] = x[0, 0, 1]   # the only row that fits: row 0, token 0
    vview[0, 0, :, 127] = x[0, 0, 2]
    assert torch.equal(bits(cache.k), bits(kview))
    assert torch.equal(bits(cache.v), bits(vview))
    n, G = B * H * Smax * 64, 4096
    for lo, hi in ((0, G), (G + n, 2 * G + n), (2 * G + 2 * n, 3 * G + 2 * n)):
        assert torch.equal(bits(whole[lo:hi]), bits(before[lo:hi])), "guard region written"


# ---------------------------------------------------------------------------------------------- decode attention
def _ref_attend(q, K, V, n, scale):
    """f32 softmax(q K^T scale) V over the first n[b] positions. q [B,H,64], K/V [B,H,Smax,64]."""
    out = torch.empty(q.shape, dtype=torch.float32, device=q.device)
    for b in range(q.shape[0]):
        k, v = K[b, :, :n[b]].float(), V[b, :, :n[b]].float()
        s = torch.einsum("hd,hsd->hs", q[b].float(), k) * scale
        out[b] = torch.einsum("hs,hsd->hd", torch.softmax(s, -1), v)
    return out


def _decode_case(dev, B, H, Smax, n_after, seed=0):
    """Cache holding n_after[b]-1 random positions and NaN everywhere else; append one token, attend.
    Returns (out [B,H,64], reference [B,H,64])."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cache, _ = _guarded_cache(B, H, Smax, dev, fill=float("nan"))
    K = torch.randn(B, H, Smax, 64, generator=g).to(BF).to(dev)
    V = torch.randn(B, H, Smax, 64, generator=g).to(BF).to(dev)
    qkv = torch.randn(B, 1, 3 * H * 64, generator=g).to(BF).to(dev)
    lens = [n - 1 for n in n_after]
    for b in range(B):
        cache.k[0, b, :, :lens[b]] = K[b, :, :lens[b]]
        cache.v[0, b, :, :lens[b]] = V[b, :, :lens[b]]
    cache.set_lens(torch.tensor(lens, device=dev))
    x = qkv.view(B, 3, H, 64)
    for b in range(B):
        K[b, :, lens[b]] = x[b, 1]
        V[b, :, lens[b]] = x[b, 2]
    cache.store(0, qkv)
    out = cache.attend(0, qkv)
    assert tuple(out.shape) == (B, 1, H * 64) and out.dtype == BF
    # everything past each row's length is still NaN (the kernels wrote nothing there)
    for b in range(B):
        assert torch.isnan(cache.k[0, b, :, n_after[b]:].float()).all()
    ref = _ref_attend(x[:, 0], K, V, n_after, 1.0 / 8.0)
    return out.view(B, H, 64), ref, cache, qkv


def _length_sets(B, Smax):
    c = ops.decode.decode_chunk()
    want = [n for n in (1, c - 1, c, c + 1, Smax - 1, Smax, 2 * c, 2 * c + 1, Smax // 2) if 1 <= n <= Smax]
    want = list(dict.fromkeys(want))
    sets = []
    while want:
        row, want = want[:B], want[B:]
        row = row + [row[-1]] * (B - len(row))
        sets.append(row)
    return sets


@pytest.mark.parametrize("B,H,Smax", [(2, 3, 320), (1, 1, 64), (5, 2, 128)])
def test_attn_decode_matches_reference(cuda, B, H, Smax):
    seen = set()
    for i, n_after in enumerate(_length_sets(B, Smax)):
        out, ref, _, _ = _decode_case(cuda, B, H, Smax, n_after, seed=i)
        assert torch.isfinite(out.float()).all(), f"non-finite output at lengths {n_after}"
        close(out, ref, ATTN_TOL)
        seen.update(n_after)
    c = ops.decode.decode_chunk()
    for n in (1, c - 1, c, c + 1, Smax - 1, Smax):
        assert n in seen or not 1 <= n <= Smax


def test_attn_decode_counter_and_bitwise_repeat(cuda):
    from distributed_tensorflow_amd.ops._util import launch_counts, launch_delta
    out, ref, cache, qkv = _decode_case(cuda, 2, 3, 320, [129, 320], seed=11)
    before = launch_counts()
    a = cache.attend(0, qkv)
    d = launch_delta(before)
    assert d["attn_decode"] == 1 and sum(d.values()) == 1, d
    b = cache.attend(0, qkv)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(out.reshape(a.shape)))


def test_attn_decode_dominant_key_returns_its_value_row(cuda):
    B, H, Smax = 2, 3, 320
    torch.manual_seed(5)
    cache = ops.KVCache(1, B, H, Smax, cuda)
    cache.k.copy_(torch.randn(cache.k.shape, device=cuda) * 0.1)
    cache.v.copy_(torch.randn(cache.v.shape, device=cuda))
    qkv = torch.randn(B, 1, 3 * H * 64, device=cuda).to(BF)
    q = qkv.view(B, 3, H, 64)[:, 0]
    hot = [[3, 200, 131], [127, 128, 255]]  # a different key per (b, h), on both sides of the chunk boundaries
    for b in range(B):
        for h in range(H):
            cache.k[0, b, h, hot[b][h]] = q[b, h] * 8.0   # score 8 |q|^2 / 8 ~ 64 against ~N(0, 0.1 |q|)
    cache.set_lens(torch.tensor([299, 280], device=cuda))
    out = cache.attend(0, qkv).view(B, H, 64)
    for b in range(B):
        for h in range(H):
            want = cache.v[0, b, h, hot[b][h]].float()
            got = out[b, h].float()
            assert ((got - want).abs() <= 2.0 ** -7 * want.abs() + 1e-30).all(), (b, h)


def test_attn_decode_full_cache_row(cuda):
    """lens[b] >= Smax before the call: store writes nothing, attend covers the whole cache and stays finite."""
    B, H, Smax = 2, 2, 128
    torch.manual_seed(6)
    cache, whole = _guarded_cache(B, H, Smax, cuda)
    qkv = torch.randn(B, 1, 3 * H * 64, device=cuda).to(BF)
    cache.set_lens(torch.tensor([Smax, Smax + 5], device=cuda))
    before = whole.clone()
    cache.store(0, qkv)
    assert torch.equal(bits(whole), bits(before))
    out = cache.attend(0, qkv).view(B, H, 64)
    assert torch.isfinite(out.float()).all()
    ref = _ref_attend(qkv.view(B, 3, H, 64)[:, 0], cache.k[0], cache.v[0], [Smax, Smax], 1.0 / 8.0)
    close(out, ref, ATTN_TOL)


def test_attn_decode_rejects_other_head_dims(cuda):
    with pytest.raises(ValueError):
        ops.KVCache(1, 1, 2, 64, cuda, head_dim=32)


def test_token_by_token_matches_causal_attention(cuda):
    B, H, S = 2, 2, 70
    torch.manual_seed(7)
    qkv = torch.randn(B, S, 3 * H * 64, device=cuda).to(BF)
    full = ops.attention_packed(qkv, H, causal=True)
    cache = ops.KVCache(1, B, H, S, cuda)
    cache.k.fill_(float("nan"))
    cache.v.fill_(float("nan"))
    outs = []
    for s in range(S):
        step = qkv[:, s:s + 1].contiguous()
        cache.store(0, step)
        outs.append(cache.attend(0, step))
        cache.advance(1)
    got = torch.cat(outs, 1).float()
    err = (got - full.float()).abs().amax((0, 2))
    ref = full.float().abs().amax((0, 2)) + 1e-6
    bad = (err > ATTN_TOL * ref).nonzero()
    assert bad.numel() == 0, f"positions {bad.flatten().tolist()} off: {err[bad.flatten()].tolist()}"
    assert cache.lens.tolist() == [S, S]


# ---------------------------------------------------------------------------------------------- dense_skinny
# the issue's shapes, plus two narrow-K shapes whose N reaches the kernel's 8- and 16-rows-per-block variants (the
# second with N % 16 != 0 and K no multiple of a wave step: both tails)
SKINNY_SHAPES = [(64, 64), (200, 264), (1000, 2048), (1024, 4096), (4104, 72), (16392, 72)]


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("N,K", SKINNY_SHAPES)
def test_dense_skinny_matches_reference_and_dense(cuda, N, K, epilogue):
    from distributed_tensorflow_amd.ops._util import launch_counts, launch_delta
    torch.manual_seed(N + K)
    w = (torch.randn(N, K, device=cuda) / math.sqrt(K)).to(BF)
    w32 = w.float()  # an f32 master whose bf16 shadow is w exactly: ops.dense reads the same weights
    bias = torch.randn(N, device=cuda) if epilogue else None
    act = "gelu" if epilogue else None
    for M in (1, 3, 8, 16):
        x = torch.randn(M, K, device=cuda).to(BF)
        before = launch_counts()
        y = ops.dense_skinny(x, w, bias, act)
        d = launch_delta(before)
        assert d["dense_skinny"] == 1 and sum(d.values()) == 1, d
        assert y.dtype == BF and tuple(y.shape) == (M, N)
        ref = x.float() @ w32.t()
        if epilogue:
            ref = torch.nn.functional.gelu(ref + bias, approximate="tanh")
        close(y, ref, DENSE_TOL)
        close(y, ops.dense(x, w32, bias, act=act), DENSE_TOL)
        assert torch.equal(bits(y), bits(ops.dense_skinny(x, w, bias, act))), "not reproducible run to run"


def test_dense_skinny_rejects_bad_shapes(cuda):
    def run(M, N, K):
        return ops.dense_skinny(torch.zeros(M, K, device=cuda, dtype=BF), torch.zeros(N, K, device=cuda, dtype=BF))
    run(16, 64, 64)
    for M, N, K in ((17, 64, 64), (4, 64, 66), (4, 10, 64)):
        with pytest.raises(RuntimeError):
            run(M, N, K)


@pytest.mark.parametrize("N,K", [(1000, 2048), (200, 264), (4104, 72), (16392, 72)])
def test_dense_skinny_one_hot_rows_return_weight_columns(cuda, N, K):
    """x[m] = e_{k_m} with the k_m spread over the waves and K sub-ranges, and an asymmetric w: out[m, n] = w[n, k_m]
    exactly (any transpose or K-mapping error shows as a wrong element, not as rounding)."""
    torch.manual_seed(9)
    M = 16
    w = torch.randn(N, K, device=cuda).to(BF)
    km = [(m * 131 + 7 + 8 * m) % K for m in range(M)]
    x = torch.zeros(M, K, device=cuda, dtype=BF)
    for m in range(M):
        x[m, km[m]] = 1.0
    y = ops.dense_skinny(x, w)
    assert torch.equal(bits(y), bits(w[:, km].t()))
    y3 = ops.dense_skinny(x[5:8].reshape(1, 3, K), w)   # leading axes are flattened and restored
    assert tuple(y3.shape) == (1, 3, N) and torch.equal(bits(y3[0]), bits(w[:, km[5:8]].t()))
