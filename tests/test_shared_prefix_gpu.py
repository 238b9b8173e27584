"""Shared-prefix decode attention (csrc/kernels/attn_decode_shared.hip) behind KVCache.fork, against an f64 softmax over
[prefix[:P] ; own[P:lens+1]], and generate(num_return_sequences=) against repeated prompts.

close(a, b, tol) and ATTN_TOL are those of tests/test_decode_gpu.py.
"""
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops._util import call_log

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ATTN_TOL = 2e-2
H, CAP, B0 = 2, 384, 2
VOCAB = 200
CFG = dict(vocab=VOCAB, ctx=96, hidden=128, layers=2, heads=2)


def close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max err {err} vs ref scale {ref} (tol {tol})"


def reference(qkv, parent, fork, plens, lens, G):
    """f64 softmax(q K^T / 8) V per (b, h) over the parent's first P rows and the fork's rows P .. lens."""
    q = qkv[:, 0, :H * 64].double().reshape(-1, H, 64)
    out = torch.empty_like(q)
    for b in range(q.shape[0]):
        P, n = plens[b // G], lens[b] + 1
        K = torch.cat([parent.k[0, b // G, :, :P], fork.k[0, b, :, P:n]], 1).double()   # [H, n, 64]
        V = torch.cat([parent.v[0, b // G, :, :P], fork.v[0, b, :, P:n]], 1).double()
        p = torch.softmax(torch.einsum("hd,hnd->hn", q[b], K) / 8.0, -1)
        out[b] = torch.einsum("hn,hnd->hd", p, V)
    return out.reshape(-1, 1, H * 64)


@pytest.mark.parametrize("plens", [(1, 127), (128, 129), (200, 256)])
@pytest.mark.parametrize("G", [2, 5, 16])
def test_fork_store_attend(cuda, G, plens):
    torch.manual_seed(G * 1000 + plens[0])
    B = B0 * G
    lens = []
    for b in range(B):   # P, P + 1, around the next chunk boundary, the last position
        P = plens[b // G]
        edge = (P // 128 + 1) * 128
        lens.append(min([P, P + 1, edge - 1, edge, edge + 1, CAP - 1][b % 6], CAP - 1))
    pos = torch.arange(CAP, device=cuda)
    parent = ops.KVCache(1, B0, H, CAP, cuda)
    parent.set_lens(torch.tensor(plens, device=cuda))
    parent.empty = False
    dead = (pos[None, :] >= parent.lens[:, None])[None, :, None, :, None]            # past plens
    parent.k = torch.randn(1, B0, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    parent.v = torch.randn(1, B0, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    kept = parent.k.view(torch.int16).clone(), parent.v.view(torch.int16).clone()
    fork = parent.fork(G)
    assert fork.batch == B and fork.capacity == CAP and fork.lens.tolist() == [p for p in plens for _ in range(G)]
    fork.set_lens(torch.tensor(lens, device=cuda))
    dead = (pos[None, :] < fork.plens.repeat_interleave(G)[:, None]) | (pos[None, :] > fork.lens[:, None])
    dead = dead[None, :, None, :, None]                                              # below plens, past lens
    fork.k = torch.randn(1, B, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    fork.v = torch.randn(1, B, H, CAP, 64, device=cuda).to(BF).masked_fill(dead, float("nan"))
    qkv = torch.randn(B, 1, 3 * H * 64, device=cuda).to(BF)
    fork.store(0, qkv)
    with call_log() as log:
        out = fork.attend(0, qkv)
    assert log["dtf_attn_decode_shared"] == 1 and log["dtf_attn_decode"] == 0, log
    assert torch.isfinite(out.float()).all()
    close(out, reference(qkv, parent, fork, plens, lens, G), ATTN_TOL)
    assert torch.equal(out.view(torch.int16), fork.attend(0, qkv).view(torch.int16)), "two calls differ in bits"
    assert torch.equal(parent.k.view(torch.int16), kept[0]) and torch.equal(parent.v.view(torch.int16), kept[1])


def test_generate_samples_against_repeated_prompts(cuda):
    initializers.set_seed(0)
    torch.manual_seed(0)
    ids = torch.randint(0, VOCAB, (2, 40))
    with context.device(cuda), torch.no_grad():
        gpu = GPT2(**CFG)
        dids = ids.to(cuda)
        a = gpu.generate(dids, 1, num_return_sequences=4, temperature=0)
        ga = gpu.last_generation
        b = gpu.generate(dids.repeat_interleave(4, 0), 1, temperature=0)
        lb = gpu.last_generation["logits"]
        full = gpu(a, training=False).float()[:, -1, :VOCAB].cpu()
        g6 = gpu.generate(dids, 6, num_return_sequences=4, temperature=0, graph=True)
        assert gpu.last_generation["step"].captured
        e6 = gpu.generate(dids, 6, num_return_sequences=4, temperature=0, graph=False)
    with context.device("cpu"), torch.no_grad():
        cpu = GPT2(**CFG)
        cpu(ids, training=False)
        cpu.set_weights(gpu.get_weights())
        ref = cpu(a.cpu(), training=False).float()[:, -1, :VOCAB]
    assert tuple(a.shape) == (8, 41) and torch.equal(a, b) and torch.equal(g6, e6)
    assert ga["cache"].group == 4 and ga["cache"].prefix.batch == 2 and ga["cache"].lens.tolist() == [41] * 8
    # the bound of tests/test_generate_gpu.py: a cached step's error against the f32 reference within 1.5x of the
    # full-forward GPU path's on the same position
    err_full = (full - ref).abs().max().item()
    err = [(lg.float()[:, :VOCAB].cpu() - ref).abs().max().item() for lg in (ga["logits"], lb)]
    print(f"max |logits - f32 reference|: full forward {err_full:.5f}, shared {err[0]:.5f}, repeated {err[1]:.5f}")
    assert err[0] <= 1.5 * err_full, (err, err_full)
