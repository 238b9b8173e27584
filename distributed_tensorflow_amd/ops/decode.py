"""KV-cached decoding: the cache, single-token attention and the M <= 16 dense layer (csrc/kernels/attn_decode.hip).

A decode step computes one token per sequence: its attention reads the keys and values of every earlier position
(a memory-bound stream over the cache) and its projections read every weight once for at most 16 rows of activations
(a weight stream). ``KVCache`` owns K and V of all layers as ``[layers, B, H, Smax, 64]`` bf16, one ``lens[B]`` int64
tensor shared by the layers (valid positions per batch row; also the position ids of the step's embedding) and the
split-KV scratch. Per layer a step calls ``store`` (append at ``lens``), then ``attend``; the caller ``advance``s
``lens`` once per token. Nothing reads a device value on the host, so a step is hipGraph-capturable.
``attend_chunk`` is the same rule for S queries per row (query s sees positions 0 .. min(lens + s, capacity-1)): the
CPU reference of appending a multi-token chunk to a filled cache. On the GPU S == 1 is ``attend``; S > 1 runs the
multi-token append kernel (``dtf_attn_append``, csrc/kernels/attention.hip) on a cache built with ``chunked=True`` and
raises on a default cache (the route is opt-in per cache for now).

``dense_skinny`` is an explicit route: ``ops.dense`` / ``ops.gemm`` dispatch as before and never reach it.
CPU tensors take the explicit f32 torch path.
"""
from __future__ import annotations

import math

import torch

from ._util import BF16, F32, K, bf16_shadow, call, on_gpu, ptr, stream
from .linalg import _act_ref, act_code, dense

HEAD_DIM = 64
PART = 66  # f32 per split-KV partial: running max, running sum, 64 output dims


def decode_chunk():
    """Keys per block of the split-KV pass (the kernel's constant)."""
    return int(K().dtf_attn_decode_chunk())


class KVCache:
    def __init__(self, layers, batch, heads, capacity, device, head_dim=HEAD_DIM, chunked=False):
        self.device = torch.device(device)
        gpu = self.device.type == "cuda"
        if gpu and head_dim != HEAD_DIM:
            raise ValueError(f"KVCache on the GPU supports head dim {HEAD_DIM} only (got {head_dim})")
        self.layers, self.batch, self.heads, self.head_dim = int(layers), int(batch), int(heads), int(head_dim)
        self.capacity = (int(capacity) + 63) // 64 * 64
        shape = (self.layers, self.batch, self.heads, self.capacity, self.head_dim)
        # GPU: uninitialised (the kernels never let a position past lens reach the arithmetic); CPU reference: zeros
        self.k = torch.empty(shape, dtype=BF16, device=self.device) if gpu else torch.zeros(shape, dtype=F32)
        self.v = torch.empty(shape, dtype=BF16, device=self.device) if gpu else torch.zeros(shape, dtype=F32)
        self.lens = torch.zeros(self.batch, dtype=torch.int64, device=self.device)
        self.empty = True  # host-side: nothing stored since the last reset
        # GPU: attend_chunk with S > 1 runs the append kernel (False: it raises); the CPU path takes any S either way
        self.chunked = bool(chunked)
        self.scratch = None
        if gpu:
            self.nchunks = -(-self.capacity // decode_chunk())
            self.scratch = torch.empty(self.batch * self.heads * self.nchunks * PART, dtype=F32, device=self.device)

    def _check(self, layer, qkv, S=None):
        B, s, T = qkv.shape
        if B != self.batch or T != 3 * self.heads * self.head_dim or not 0 <= layer < self.layers:
            raise ValueError(f"qkv {tuple(qkv.shape)} / layer {layer} does not fit the cache "
                             f"(batch {self.batch}, heads {self.heads}, head dim {self.head_dim}, layers {self.layers})")
        if S is not None and s != S:
            raise ValueError(f"attend takes one token per row, got {s}")

    def store(self, layer, qkv):
        """Copy the K and V thirds of the packed projection qkv [B, S, 3*H*D] to positions lens[b] + s of `layer`
        (positions >= capacity are dropped; lens is unchanged)."""
        self._check(layer, qkv)
        B, S, _ = qkv.shape
        self.empty = False
        if on_gpu(qkv):
            q = qkv if qkv.dtype == BF16 else qkv.to(BF16)
            q = q.contiguous()
            call("dtf_kv_store", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.lens), B, S, self.heads,
                 self.capacity, stream(qkv.device))
            return
        pos = self.lens[:, None] + torch.arange(S)[None, :]
        bi, si = torch.nonzero(pos < self.capacity, as_tuple=True)
        pi = pos[bi, si]
        x = qkv.float().reshape(B, S, 3, self.heads, self.head_dim)
        self.k[layer][bi, :, pi] = x[bi, si, 1]
        self.v[layer][bi, :, pi] = x[bi, si, 2]

    def attend(self, layer, qkv, scale=None):
        """One query row per (b, h) from qkv [B, 1, 3*H*D] over positions 0 .. min(lens[b], capacity-1) of `layer`
        (store first: the token's own key is position lens[b]) -> [B, 1, H*D]."""
        self._check(layer, qkv, 1)
        B = self.batch
        HD = self.heads * self.head_dim
        scale = float(scale) if scale is not None else 1.0 / math.sqrt(self.head_dim)
        if on_gpu(qkv):
            q = qkv if qkv.dtype == BF16 else qkv.to(BF16)
            q = q.contiguous()
            out = torch.empty(B, 1, HD, dtype=BF16, device=qkv.device)
            call("dtf_attn_decode", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.lens), ptr(out),
                 ptr(self.scratch), B, self.heads, self.capacity, scale, stream(qkv.device))
            return out
        q = qkv[:, 0, :HD].float().reshape(B, self.heads, 1, self.head_dim)
        n = self.lens.clamp(0, self.capacity - 1) + 1
        s = torch.matmul(q, self.k[layer].transpose(-1, -2)) * scale          # [B, H, 1, Smax]
        dead = torch.arange(self.capacity)[None, :] >= n[:, None]
        p = torch.softmax(s.masked_fill(dead[:, None, None, :], float("-inf")), -1)
        o = torch.matmul(p, self.v[layer])                                     # [B, H, 1, D]
        return o.permute(0, 2, 1, 3).reshape(B, 1, HD).to(qkv.dtype)

    def attend_chunk(self, layer, qkv, scale=None):
        """S query rows per (b, h) from qkv [B, S, 3*H*D] over a filled cache (store first: query s's own key is
        position lens[b] + s): query s attends positions 0 .. min(lens[b] + s, capacity-1), `attend`'s rule per query
        -> [B, S, H*D]. S == 1 is `attend` itself (same kernel, same bits). S > 1: the explicit f32 path for CPU tensors;
        on the GPU one launch of the append kernel when the cache was built with chunked=True (lens is read on the
        device only: capturable), and NotImplementedError on a default cache, never an eager fallback — feed such a
        cache one token at a time (GPT2.extend(chunk=1), generate(prefill_chunk=1))."""
        self._check(layer, qkv)
        B, S, _ = qkv.shape
        if S == 1:
            return self.attend(layer, qkv, scale)
        HD = self.heads * self.head_dim
        scale = float(scale) if scale is not None else 1.0 / math.sqrt(self.head_dim)
        if on_gpu(qkv):
            if not self.chunked:
                raise NotImplementedError(f"attend_chunk: no GPU kernel for a chunk of {S} > 1 queries over a filled "
                                          "KV cache built without chunked=True; feed one token at a time (chunk=1 / "
                                          "prefill_chunk=1)")
            q = qkv if qkv.dtype == BF16 else qkv.to(BF16)
            q = q.contiguous()
            out = torch.empty(B, S, HD, dtype=BF16, device=qkv.device)
            call("dtf_attn_append", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.lens), ptr(out), B, S,
                 self.heads, self.capacity, scale, stream(qkv.device))
            return out
        q = qkv[:, :, :HD].float().reshape(B, S, self.heads, self.head_dim).transpose(1, 2)   # [B, H, S, D]
        lim = (self.lens.clamp(min=0)[:, None] + torch.arange(S)[None, :]).clamp(max=self.capacity - 1)  # [B, S]
        s = torch.matmul(q, self.k[layer].transpose(-1, -2)) * scale                           # [B, H, S, Smax]
        dead = torch.arange(self.capacity)[None, None, :] > lim[:, :, None]                    # [B, S, Smax]
        p = torch.softmax(s.masked_fill(dead[:, None], float("-inf")), -1)
        o = torch.matmul(p, self.v[layer])                                                     # [B, H, S, D]
        return o.transpose(1, 2).reshape(B, S, HD).to(qkv.dtype)

    def advance(self, n=1):
        self.lens.add_(n)

    def set_lens(self, lens):
        self.lens.copy_(lens)

    def reset(self):
        self.lens.zero_()
        self.empty = True


def dense_skinny(x, w, bias=None, act=None):
    """act(x @ w^T + bias) for at most 16 rows of x (all leading axes together): the weight-streaming kernel of a
    decode step. w: [N, K] bf16, or an f32 master variable (its bf16 shadow is read); bias f32; K % 8 == N % 8 == 0."""
    a = act_code(act)
    if not on_gpu(x):
        y = torch.nn.functional.linear(x.to(w.dtype), w, bias)
        return _act_ref(y, a)
    w16 = w if w.dtype == BF16 else bf16_shadow(w)
    w16 = w16.contiguous()
    x2 = x.reshape(-1, x.shape[-1])
    x2 = (x2 if x2.dtype == BF16 else x2.to(BF16)).contiguous()
    if bias is not None and (bias.dtype != F32 or not bias.is_contiguous()):
        bias = bias.float().contiguous()
    M, Kd = x2.shape
    N = w16.shape[0]
    if w16.shape[1] != Kd:
        raise ValueError(f"dense_skinny: x [..., {Kd}] against w {tuple(w16.shape)}")
    out = torch.empty(M, N, dtype=BF16, device=x.device)
    call("dtf_dense_skinny", ptr(x2), ptr(w16), ptr(bias), ptr(out), M, N, Kd, a, stream(x.device))
    return out.reshape(*x.shape[:-1], N)


# (N, K) of projections that the decode step keeps on ops.dense because dense_skinny measured slower there
# (tools/bench_generate.py, profiles/generate_decode.txt)
SKINNY_EXCLUDE = frozenset()


def step_dense(x, w, bias=None, act=None):
    """A projection of the one-token decode step: dense_skinny from the bf16 shadow of w wherever it applies."""
    if on_gpu(x):
        M = x.numel() // x.shape[-1]
        N, Kd = w.shape
        if M <= 16 and N % 8 == 0 and Kd % 8 == 0 and (N, Kd) not in SKINNY_EXCLUDE:
            return dense_skinny(x, w, bias, act)
    return dense(x, w, bias, act=act)
