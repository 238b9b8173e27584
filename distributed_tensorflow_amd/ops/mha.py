"""Scaled dot-product attention.

GPU: one fused HIP kernel per direction (csrc/kernels/attention.hip): online-softmax forward that never
materialises the [S, S] scores, and a deterministic two-kernel backward (dK/dV by key blocks, dQ by
query blocks), with causal and additive key masks and in-kernel dropout on the probabilities. The
packed entry point reads Q/K/V straight out of the fused QKV projection [B, S, 3*H*64] and writes
O as [B, S, H*64], so no head split/merge copies exist; its backward writes one packed dQKV.
Head dims other than 64 use the composed path (MFMA batched GEMM + softmax kernel). CPU: f32 reference.
"""
from __future__ import annotations

import ctypes
import math

import torch

from ._util import BF16, F32, call, on_gpu, ptr, rng_counter, stream
from .linalg import bmm
from .nn import masked_row_softmax, softmax

_seed_counter = [0]

# Backward through a dS^T scratch (dtf_attn_bwd_ds: the dK/dV kernel stores dS, dQ is a memory-bound GEMM over it)
# instead of a dQ kernel that recomputes the scores, probabilities and dP: causal attention only (None; tests set True /
# False to force a path) — measured (tools/bench_attention.py, profiles/r4_attention_bench.txt): GPT-2-medium causal S=1024
# 178 -> 158 us (213 -> 183 with dropout); BERT-base S=512 203 -> 227 us (the dS round trip costs more than the
# recompute saves when no tiles are skipped)
_ATTN_DS = None
# The dS^T scratch is O(B*H*S^2) (GPT-2-medium S=1024 B=8: 268 MB per call); above this many bytes the backward takes
# the O(S) recompute kernel instead, so a long-context run keeps flash attention's memory bound.
DS_SCRATCH_MAX_BYTES = 1 << 30


def ds_scratch_bytes(B, H, Sq, Sk):
    return 2 * B * H * Sk * (-(-Sq // 64) * 64)


def uses_ds_path(causal, B, H, Sq, Sk):
    """True when the attention backward goes through the dS^T scratch (dtf_attn_bwd_ds)."""
    if not (_ATTN_DS or (_ATTN_DS is None and causal)):
        return False
    return ds_scratch_bytes(B, H, Sq, Sk) <= DS_SCRATCH_MAX_BYTES


def _next_seed(seed, device):
    """(host seed, device step-counter pointer or None): see ops.nn._auto_seed."""
    if seed is not None:
        return seed, None
    _seed_counter[0] += 1
    return (_seed_counter[0] * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF, rng_counter(device)


def _layout(ts, heads):
    """How the kernels address ts: (B, H, Sq, Sk, D); the {batch, seq, head} strides (elements) of q (and dq), of k / v
    (and dk / dv) and of o (and dout) as ctypes arrays; the shape of o; and the q, k, v pointers of tensors laid out as
    ts (ts itself, or its gradients). heads > 0: one packed [B, S, 3*H*D] tensor read in place, o [B, S, H*D];
    heads = 0: q, k, v and o [B, H, S, D]."""
    if heads:
        B, S, T = ts[0].shape
        HD = T // 3
        D = HD // heads
        dims, strides, oshape = (B, heads, S, S, D), ((S * T, T, D),) * 2 + ((S * HD, HD, D),), (B, S, HD)
        ptrs = lambda g: [g[0].data_ptr() + 2 * HD * j for j in range(3)]  # noqa: E731
    else:
        B, H, Sq, D = ts[0].shape
        Sk = ts[1].shape[2]
        qs = (H * Sq * D, D, Sq * D)
        dims, strides, oshape = (B, H, Sq, Sk, D), (qs, (H * Sk * D, D, Sk * D), qs), ts[0].shape
        ptrs = lambda g: [ptr(t) for t in g]  # noqa: E731
    return dims, [(ctypes.c_long * 3)(*s) for s in strides], oshape, ptrs


class _FlashFn(torch.autograd.Function):
    """ts: q, k, v [B, H, S, D] (heads = 0), or the packed projection output [B, S, 3*H*D] (heads = H)."""

    @staticmethod
    def forward(ctx, heads, kmask, causal, scale, dropout, seed, ctr, *ts):
        ts = [t.contiguous() for t in ts]
        dims, strides, oshape, ptrs = _layout(ts, heads)
        qs, ks, os_ = map(ctypes.addressof, strides)
        o = torch.empty(oshape, dtype=BF16, device=ts[0].device)
        lse = torch.empty(dims[0] * dims[1], dims[2], dtype=F32, device=o.device)
        call("dtf_attn_fwd", *ptrs(ts), qs, ks, ptr(o), os_, ptr(lse), ptr(kmask), *dims, float(scale), float(dropout),
             seed, int(causal), ctr, stream())
        ctx.save_for_backward(*ts, o, lse, kmask)
        ctx.cfg = (heads, causal, scale, dropout, seed, ctr)
        return o

    @staticmethod
    def backward(ctx, do):
        *ts, o, lse, kmask = ctx.saved_tensors
        heads, causal, scale, dropout, seed, ctr = ctx.cfg
        dims, strides, _, ptrs = _layout(ts, heads)
        qs, ks, os_ = map(ctypes.addressof, strides)
        B, H, Sq, Sk, _ = dims
        do = do.to(BF16).contiguous()
        grads = [torch.empty_like(t) for t in ts]
        dvec = torch.empty(B * H, Sq, dtype=F32, device=o.device)
        args = (*ptrs(ts), qs, ks, ptr(o), ptr(do), os_, ptr(lse), ptr(dvec), *ptrs(grads), ptr(kmask), *dims,
                float(scale), float(dropout), seed, int(causal), ctr)
        if uses_ds_path(causal, B, H, Sq, Sk):
            ds = torch.empty(ds_scratch_bytes(B, H, Sq, Sk) // 2, dtype=BF16, device=o.device)
            call("dtf_attn_bwd_ds", *args, ptr(ds), stream())
        else:
            call("dtf_attn_bwd", *args, stream())
        return (None,) * 7 + tuple(grads)


def _kmask(mask, B, Sk):
    if mask is None:
        return None
    return mask.reshape(B, Sk).float().contiguous()


def attention(q, k, v, causal=False, mask=None, scale=None, dropout=0.0, training=False, seed=None):
    """q, k, v: [B, H, S, D]. mask: optional additive f32 mask broadcastable as [B, 1, 1, Sk]."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    rate = float(dropout) if (dropout and training) else 0.0
    if on_gpu(q):
        if D == 64 and k.shape[2] == v.shape[2]:
            seed, ctr = _next_seed(seed, q.device)
            return _FlashFn.apply(0, _kmask(mask, B, Sk), bool(causal), float(scale), rate, seed, ctr, q.to(BF16),
                                  k.to(BF16), v.to(BF16))
        return _composed(q, k, v, causal, mask, scale, rate)
    p = _reference_probs(q, k, causal, mask, scale)
    if rate:
        p = torch.nn.functional.dropout(p, rate)
    return torch.matmul(p, v.float()).to(q.dtype)


def attention_packed(qkv, heads, causal=False, mask=None, scale=None, dropout=0.0, training=False, seed=None):
    """Self-attention on the fused projection output qkv [B, S, 3*H*D] -> [B, S, H*D]."""
    B, S, T = qkv.shape
    D = T // (3 * heads)
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    rate = float(dropout) if (dropout and training) else 0.0
    if on_gpu(qkv) and D == 64 and qkv.dtype == BF16:
        seed, ctr = _next_seed(seed, qkv.device)
        return _FlashFn.apply(heads, _kmask(mask, B, S), bool(causal), float(scale), rate, seed, ctr, qkv)
    q, k, v = split_qkv(qkv, heads)
    return merge_heads(attention(q, k, v, causal, mask, scale, dropout, training))


def _composed(q, k, v, causal, mask, scale, rate):
    """K3 + K7 composition (batched MFMA GEMMs around the masked softmax kernel)."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    q3 = q.reshape(B * H, Sq, D)
    k3 = k.reshape(B * H, Sk, D)
    v3 = v.reshape(B * H, Sk, D)
    s = bmm(q3, k3, transpose_b=True)
    am = None
    if mask is not None:
        am = mask.reshape(B, Sk).float().repeat_interleave(H, 0).contiguous()
    p = softmax(s.reshape(B * H, Sq, Sk), scale=scale, causal=causal, add_mask=am)
    if rate:
        from .nn import dropout as _drop
        p = _drop(p, rate)
    return bmm(p, v3).reshape(B, H, Sq, D)


def _reference_probs(q, k, causal, mask, scale):
    """f32 softmax(q k^T * scale + masks) of [B, H, S, D] tensors; scale given."""
    B, Sq, Sk = q.shape[0], q.shape[2], k.shape[2]
    s = torch.matmul(q.float(), k.float().transpose(-1, -2)) * scale
    if causal:
        m = torch.ones(Sq, Sk, dtype=torch.bool, device=q.device).tril(Sk - Sq)
        s = s.masked_fill(~m, float("-inf"))
    if mask is not None:
        s = s + mask.reshape(B, 1, 1, Sk).float()
    return masked_row_softmax(s)  # rows with no visible key: 0, as the kernels


def reference_attention(q, k, v, causal=False, mask=None, scale=None, keep_mask=None, keep=1.0):
    """f32 reference with an explicit dropout keep-mask (tests)."""
    scale = scale if scale is not None else 1.0 / math.sqrt(q.shape[-1])
    p = _reference_probs(q, k, causal, mask, scale)
    if keep_mask is not None:
        p = p * keep_mask / keep
    return torch.matmul(p, v.float())


def split_heads(x, heads):
    """[B, S, H*D] -> [B, H, S, D] (contiguous)."""
    B, S, HD = x.shape
    return x.reshape(B, S, heads, HD // heads).permute(0, 2, 1, 3).contiguous()


def merge_heads(x):
    B, H, S, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, S, H * D).contiguous()


def split_qkv(qkv, heads):
    """[B, S, 3*H*D] -> three [B, H, S, D] tensors."""
    B, S, T = qkv.shape
    D = T // (3 * heads)
    x = qkv.reshape(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).contiguous()
    return x[0], x[1], x[2]
