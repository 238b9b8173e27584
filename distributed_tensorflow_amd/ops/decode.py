"""KV-cached decoding: the cache, single-token attention and the M <= 16 dense layer (csrc/kernels/attn_decode.hip,
attn_decode_fused.hip).

A decode step computes one token per sequence: its attention reads the keys and values of every earlier position
(a memory-bound stream over the cache) and its projections read every weight once for at most 16 rows of activations
(a weight stream). ``KVCache`` owns K and V of all layers as ``[layers, B, H, Smax, 64]`` bf16 (or fp8 codes, below), one ``lens[B]`` int64
tensor shared by the layers (valid positions per batch row; also the position ids of the step's embedding) and the
split-KV scratch. Per layer a step calls ``store`` (append at ``lens``), then ``attend``; the caller ``advance``s
``lens`` once per token. Nothing reads a device value on the host, so a step is hipGraph-capturable.
``attend_chunk`` is the same rule for S queries per row (query s sees positions 0 .. min(lens + s, capacity-1)): the
CPU reference of appending a multi-token chunk to a filled cache. On the GPU S == 1 is ``attend``; S > 1 runs the
multi-token append kernel (``dtf_attn_append``, csrc/kernels/attention.hip) on a cache built with ``chunked=True`` and
raises on a default cache (the route is opt-in per cache for now).

``KVCache(kv_dtype="fp8")`` stores every cached row (64 values of one layer, batch row, head and position) as 64 OCP
e4m3 codes and one power-of-two f32 scale, 68 bytes instead of 128 (csrc/kernels/attn_decode_fp8.hip; the format is
``kv_quantize_reference``). ``store``, ``attend`` and ``attend_chunk`` route by the cache's dtype; the fused step's
launches (``attend(fused=True)``, ``dense_skinny_fused(store=)``) have no fp8 variant and raise ValueError. On the CPU
an fp8 cache holds the dequantized values in f32: ``store`` rounds through the format, everything else is unchanged.

``KVCache.fork(G)`` serves G continuations of one prompt (``GPT2.generate(num_return_sequences=G)``): the fork has
batch B0 * G and K/V of its own for the new tokens only, and keeps the filled parent as a read-only prefix. Its
``attend`` (csrc/kernels/attn_decode_shared.hip) reads the prompt's keys and values once per group, the G queries
against a key tile on the MFMA, and each row's own positions with the split-KV pass; both write partials that one merge
sums in a fixed order. bf16 caches and groups of 2 to 16 only; ``attend(fused=True)`` and multi-token chunks raise.
``fork(G, beams=True)`` is the cache of beam search (``GPT2.generate(num_beams=G)``): a uint8 slot table names, per row
and own position, the physical row of the group that holds it, the split-KV pass resolves every key through it
(``dtf_attn_decode_beam``), and ``reorder(parent)`` lets row j continue row parent[j] by rewriting table columns in place
(``dtf_beam_reorder``, csrc/kernels/beam.hip): no K/V is ever copied.

``dense_skinny`` is an explicit route: ``ops.dense`` / ``ops.gemm`` dispatch as before and never reach it.
``dense_skinny_fused`` and ``KVCache.attend(fused=True)`` are the launches of the fused one-token step
(``GPT2.generate(step="fused")``): the same kernels with LayerNorm, the residual add, the cache append and the split-KV
merge inside them. ``dense_wide`` (csrc/kernels/dense_wide.hip) is the weight stream for up to 64 rows, the projections
of the opt-in wide step (``GPT2.generate(step="wide")``) at 17 to 64 sequences. ``dense_tall``
(csrc/kernels/dense_tall.hip) carries the weight stream to 256 rows, x shared through LDS and K split across blocks:
the projections of the tall step (``GPT2.generate(step="tall")``) at 65 to 256 rows, which below that is the wide step.
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


def kv_quantize_reference(x):
    """The fp8 KV-cache format in plain torch on the CPU: x [..., 64] -> (codes uint8 [..., 64], scale f32 [...]).
    scale = 2^e with a = the row's largest finite |v| = m * 2^x (1 <= m < 2): e = x - 8 if m <= 1.75 else x - 7 (the
    smallest e with a * 2^-e <= 448), at least -64, and 0 for a == 0. code = e4m3fn(clamp(v * 2^-e, +-448)), rounded
    to nearest even; NaN stays a NaN code, +-inf saturates."""
    x = x.detach().float().cpu()
    a = torch.where(torch.isfinite(x), x.abs(), torch.zeros_like(x)).amax(-1)
    mant, exp = torch.frexp(a)                      # a = mant * 2^exp, 0.5 <= mant < 1: m = 2 mant, x = exp - 1
    e = exp - 9 + (mant > 0.875).to(exp.dtype)
    e = torch.where(a == 0, torch.zeros_like(e), e.clamp(min=-64))
    y = torch.ldexp(x, -e[..., None]).clamp(-448.0, 448.0)   # exact; torch.clamp keeps NaN
    return y.to(torch.float8_e4m3fn).view(torch.uint8), torch.ldexp(torch.ones_like(a), e)


def _kv_dequantize(codes, scale):
    return codes.view(torch.float8_e4m3fn).float() * scale[..., None]


class KVCache:
    def __init__(self, layers, batch, heads, capacity, device, head_dim=HEAD_DIM, chunked=False, kv_dtype=None):
        if kv_dtype not in (None, "bf16", "fp8"):
            raise ValueError(f"KVCache: kv_dtype {kv_dtype!r} (None, 'bf16' or 'fp8')")
        self.kv_dtype = kv_dtype or "bf16"
        self.fp8 = self.kv_dtype == "fp8"
        self.device = torch.device(device)
        gpu = self.device.type == "cuda"
        if gpu and head_dim != HEAD_DIM:
            raise ValueError(f"KVCache on the GPU supports head dim {HEAD_DIM} only (got {head_dim})")
        self.layers, self.batch, self.heads, self.head_dim = int(layers), int(batch), int(heads), int(head_dim)
        self.capacity = (int(capacity) + 63) // 64 * 64
        shape = (self.layers, self.batch, self.heads, self.capacity, self.head_dim)
        # GPU: uninitialised (the kernels never let a position past lens reach the arithmetic); CPU reference: zeros
        self.k_scale = self.v_scale = None
        if gpu and self.fp8:  # e4m3 codes and one f32 power-of-two scale per cached row
            self.k, self.v = (torch.empty(shape, dtype=torch.uint8, device=self.device) for _ in range(2))
            self.k_scale, self.v_scale = (torch.empty(shape[:-1], dtype=F32, device=self.device) for _ in range(2))
        else:
            self.k = torch.empty(shape, dtype=BF16, device=self.device) if gpu else torch.zeros(shape, dtype=F32)
            self.v = torch.empty(shape, dtype=BF16, device=self.device) if gpu else torch.zeros(shape, dtype=F32)
        self.lens = torch.zeros(self.batch, dtype=torch.int64, device=self.device)
        self.empty = True  # host-side: nothing stored since the last reset
        # GPU: attend_chunk with S > 1 runs the append kernel (False: it raises); the CPU path takes any S either way
        self.chunked = bool(chunked)
        self.scratch = self.counters = None
        if gpu:
            self.nchunks = -(-self.capacity // decode_chunk())
            self.scratch = torch.empty(self.batch * self.heads * self.nchunks * PART, dtype=F32, device=self.device)
            # attend(fused=True): one ticket counter per (b, h); zero here, and every call leaves them zero
            self.counters = torch.zeros(self.batch * self.heads, dtype=torch.int32, device=self.device)
        # set by fork(): group > 1 marks a forked cache; on the GPU prefix is the parent and plens its lengths
        self.group, self.prefix, self.plens = 1, None, None
        # fork(beams=True): rows may continue each other's history (reorder); on the GPU through the slot table
        self.beams, self.slots = False, None

    def fork(self, group, beams=False):
        """A cache of batch B0 * group for `group` continuations of every row of this (filled, bf16) cache: row
        b0 * group + j continues row b0. Same capacity, layers and heads. On the GPU nothing is copied: the new cache
        has uninitialised K/V of its own for positions from plens = lens.clone() on and keeps this cache by reference
        as its read-only `prefix`; `attend` reads positions below plens[b0] once per group from the prefix
        (dtf_attn_decode_shared). Do not write to the parent while a fork is in use. On the CPU the parent's rows are
        repeated into a plain f32 cache: the reference semantics. ValueError for an empty, fp8 or already forked cache
        and for a group outside 2..16.

        beams=True (beam search, GPT2.generate(num_beams=)): the rows of a group may continue each other's history
        (`reorder`). On the GPU the fork also owns `slots`, uint8 [B0 * group, capacity]: row b's key and value at an
        own position p (plens <= p < lens[b]) live in physical row (b // group) * group + slots[b, p] of the fork's
        K/V; position lens[b], the token `store` has just put there, is always row b's own. Every entry of row b
        starts as b % group, and `attend` resolves each key through the table (dtf_attn_decode_beam)."""
        G = int(group)
        if not 2 <= G <= 16:
            raise ValueError(f"KVCache.fork: group {group} (2..16)")
        if self.fp8:
            raise ValueError("KVCache.fork: the shared-prefix attention has no fp8-cache variant")
        if self.empty:
            raise ValueError("KVCache.fork: the cache is empty (prefill it first)")
        if self.group > 1:
            raise ValueError("KVCache.fork: this cache is a fork already")
        c = KVCache(self.layers, self.batch * G, self.heads, self.capacity, self.device, head_dim=self.head_dim)
        c.group, c.plens, c.empty = G, self.lens.clone(), False
        c.lens = c.plens.repeat_interleave(G)
        if self.device.type == "cuda":
            c.prefix = self
            c.scratch = torch.empty(2 * c.scratch.numel(), dtype=F32, device=self.device)  # a prefix and a suffix half
        else:
            c.k, c.v = self.k.repeat_interleave(G, 1), self.v.repeat_interleave(G, 1)
        c.beams = bool(beams)
        if c.beams and c.prefix is not None:
            own = torch.arange(c.batch, device=self.device) % G
            c.slots = own.to(torch.uint8)[:, None].repeat(1, c.capacity)
        return c

    def reorder(self, parent, history=None, token=None):
        """Row g * G + j of a fork(beams=True) continues row g * G + parent[g * G + j] (parent [batch] int32, values
        0 .. G-1; the rows of a group hold the same length). Call it after the step that stored position lens - 1 and
        before the next `store`. On the GPU no K/V moves: one launch (dtf_beam_reorder) gathers the slot table by
        parent column by column, in place, and makes the column just closed (lens - 1) parent itself. history
        [batch, width] int64 (each row's tokens so far) is gathered the same way in the same launch, and its column
        lens[b] receives token [batch] int64 when given. CPU tensors: an index_select of K/V and of the history."""
        if not self.beams:
            raise ValueError("KVCache.reorder: not a fork(beams=True)")
        G = self.group
        if tuple(parent.shape) != (self.batch,) or parent.dtype != torch.int32 or not parent.is_contiguous():
            raise ValueError(f"KVCache.reorder: parent is a contiguous int32 [{self.batch}]")
        if history is not None and (history.dim() != 2 or history.shape[0] != self.batch
                                    or history.dtype != torch.int64 or not history.is_contiguous()):
            raise ValueError(f"KVCache.reorder: history is a contiguous int64 [{self.batch}, width]")
        if token is not None and (history is None or tuple(token.shape) != (self.batch,)
                                  or token.dtype != torch.int64 or not token.is_contiguous()):
            raise ValueError(f"KVCache.reorder: token is a contiguous int64 [{self.batch}] and goes with a history")
        if self.slots is not None:
            call("dtf_beam_reorder", ptr(self.slots), ptr(history), ptr(parent), ptr(self.lens), ptr(token),
                 self.batch // G, G, self.capacity, 0 if history is None else history.shape[1],
                 stream(self.device))
            return
        rows = torch.arange(self.batch) // G * G + parent.long().clamp(0, G - 1)
        self.k, self.v = self.k.index_select(1, rows), self.v.index_select(1, rows)
        if history is not None:
            history.copy_(history.index_select(0, rows))
            if token is not None:
                at = self.lens < history.shape[1]
                history[torch.nonzero(at)[:, 0], self.lens[at]] = token[at]

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
            if self.fp8:
                call("dtf_kv_store_fp8", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.k_scale[layer]),
                     ptr(self.v_scale[layer]), ptr(self.lens), B, S, self.heads, self.capacity, stream(qkv.device))
                return
            call("dtf_kv_store", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.lens), B, S, self.heads,
                 self.capacity, stream(qkv.device))
            return
        pos = self.lens[:, None] + torch.arange(S)[None, :]
        bi, si = torch.nonzero(pos < self.capacity, as_tuple=True)
        pi = pos[bi, si]
        x = qkv.float().reshape(B, S, 3, self.heads, self.head_dim)
        if self.fp8:  # the reference of the fp8 store: the values the format keeps
            x = _kv_dequantize(*kv_quantize_reference(x))
        self.k[layer][bi, :, pi] = x[bi, si, 1]
        self.v[layer][bi, :, pi] = x[bi, si, 2]

    def attend(self, layer, qkv, scale=None, fused=False):
        """One query row per (b, h) from qkv [B, 1, 3*H*D] over positions 0 .. min(lens[b], capacity-1) of `layer`
        (store first: the token's own key is position lens[b]) -> [B, 1, H*D]. fused=True (GPU): one launch, the
        split-KV merge done by the last block of each head; the same bits as the two-launch default."""
        self._check(layer, qkv, 1)
        if fused and self.fp8:
            raise ValueError("attend(fused=True): the one-launch decode attention has no fp8-cache variant")
        if fused and self.group > 1:
            raise ValueError("attend(fused=True): the one-launch decode attention has no forked-cache variant")
        B = self.batch
        HD = self.heads * self.head_dim
        scale = float(scale) if scale is not None else 1.0 / math.sqrt(self.head_dim)
        if on_gpu(qkv):
            q = qkv if qkv.dtype == BF16 else qkv.to(BF16)
            q = q.contiguous()
            out = torch.empty(B, 1, HD, dtype=BF16, device=qkv.device)
            if self.prefix is not None:  # a fork: positions below plens come from the parent, once per group
                pre = self.prefix
                if self.slots is not None:  # beams: the own positions through the slot table
                    call("dtf_attn_decode_beam", ptr(q), ptr(pre.k[layer]), ptr(pre.v[layer]), ptr(self.k[layer]),
                         ptr(self.v[layer]), ptr(self.plens), ptr(self.lens), ptr(self.slots), ptr(out),
                         ptr(self.scratch), pre.batch, self.group, self.heads, pre.capacity, self.capacity, scale,
                         stream(qkv.device))
                    return out
                call("dtf_attn_decode_shared", ptr(q), ptr(pre.k[layer]), ptr(pre.v[layer]), ptr(self.k[layer]),
                     ptr(self.v[layer]), ptr(self.plens), ptr(self.lens), ptr(out), ptr(self.scratch), pre.batch,
                     self.group, self.heads, pre.capacity, self.capacity, scale, stream(qkv.device))
                return out
            if fused:
                call("dtf_attn_decode_fused", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.lens), ptr(out),
                     ptr(self.scratch), ptr(self.counters), B, self.heads, self.capacity, scale, stream(qkv.device))
                return out
            if self.fp8:
                call("dtf_attn_decode_fp8", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.k_scale[layer]),
                     ptr(self.v_scale[layer]), ptr(self.lens), ptr(out), ptr(self.scratch), B, self.heads,
                     self.capacity, scale, stream(qkv.device))
                return out
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
        if self.group > 1:
            raise ValueError(f"attend_chunk: a forked cache takes one token per row, got {S}")
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
            if self.fp8:
                call("dtf_attn_append_fp8", ptr(q), ptr(self.k[layer]), ptr(self.v[layer]), ptr(self.k_scale[layer]),
                     ptr(self.v_scale[layer]), ptr(self.lens), ptr(out), B, S, self.heads, self.capacity, scale,
                     stream(qkv.device))
                return out
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

    def dequantized(self, layer):
        """(K, V) of `layer` in f32, [B, H, capacity, D]: code * scale for an fp8 cache on the GPU, else the plain
        values (uninitialised rows of a GPU cache included, whatever they hold)."""
        if self.fp8 and self.k_scale is not None:
            return (_kv_dequantize(self.k[layer], self.k_scale[layer]),
                    _kv_dequantize(self.v[layer], self.v_scale[layer]))
        return self.k[layer].float(), self.v[layer].float()

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


WIDE_MAX_ROWS = 64
WIDE_VARIANTS = ((8, 1), (16, 1), (16, 2), (16, 4))  # (R, T) of dense_wide_kernel, in the order of `variant`


def dense_wide(x, w, bias=None, act=None, *, variant=None):
    """act(x @ w^T + bias) for at most 64 rows of x (all leading axes together): the weight-streaming kernel of a
    batched decode step past dense_skinny's 16 rows (csrc/kernels/dense_wide.hip). Arguments as dense_skinny's.
    variant: index into WIDE_VARIANTS to run that (rows per group, groups per block) instead of the measured choice
    (tools/bench_generate.py times them all)."""
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
        raise ValueError(f"dense_wide: x [..., {Kd}] against w {tuple(w16.shape)}")
    out = torch.empty(M, N, dtype=BF16, device=x.device)
    if variant is None:
        call("dtf_dense_wide", ptr(x2), ptr(w16), ptr(bias), ptr(out), M, N, Kd, a, stream(x.device))
    else:
        call("dtf_dense_wide_variant", ptr(x2), ptr(w16), ptr(bias), ptr(out), M, N, Kd, a, int(variant),
             stream(x.device))
    return out.reshape(*x.shape[:-1], N)


TALL_MAX_ROWS = 256
# (weight rows, x rows, slab budget) of dense_tall_kernel's blocks and split rule, in the order of `variant`
TALL_VARIANTS = tuple((128, bm, b) for b in (1, 2, 4) for bm in (128, 256, 64))


def dense_tall(x, w, bias=None, act=None, *, variant=None):
    """act(x @ w^T + bias) for at most 256 rows of x (all leading axes together): the weight-streaming kernel of a
    batched decode step past dense_wide's 64 rows (csrc/kernels/dense_tall.hip). Arguments as dense_skinny's.
    variant: index into TALL_VARIANTS to run that block shape and split budget instead of the measured choice
    (tools/bench_generate.py times them all). The split-K scratch is a fresh allocation per call: inside a captured
    step it lives in the graph's pool, and no later, larger request can free it under a replay."""
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
        raise ValueError(f"dense_tall: x [..., {Kd}] against w {tuple(w16.shape)}")
    elems = int(K().dtf_dense_tall_slab_elems(M, N, Kd))
    if elems < 0:
        raise RuntimeError(f"dense_tall cannot run x [{M}, {Kd}] against w [{N}, {Kd}] (1 to {TALL_MAX_ROWS} rows, "
                           "N and K multiples of 8)")
    slabs = torch.empty(max(elems, 4), dtype=F32, device=x.device)
    out = torch.empty(M, N, dtype=BF16, device=x.device)
    if variant is None:
        call("dtf_dense_tall", ptr(x2), ptr(w16), ptr(bias), ptr(out), ptr(slabs), slabs.numel(), M, N, Kd, a,
             stream(x.device))
    else:
        call("dtf_dense_tall_variant", ptr(x2), ptr(w16), ptr(bias), ptr(out), ptr(slabs), slabs.numel(), M, N, Kd, a,
             int(variant), stream(x.device))
    return out.reshape(*x.shape[:-1], N)


def ln_max_k():
    """Largest K of dense_skinny_fused's LayerNorm prologue (the kernel's constant: its LDS tile)."""
    return int(K().dtf_dense_skinny_ln_max_k())


def dense_skinny_fused(x, w, bias=None, act=None, *, ln=None, residual=None, store=None):
    """dense_skinny with the small neighbours of a decode step inside the same launch, each optional:
    ln=(gamma, beta, eps): the projection reads LayerNorm(x) (x is the bf16 residual stream; K <= ln_max_k());
    residual: out = residual + act(x w^T + bias), the projection rounded to bf16 first (the bits of ops.add after
    dense_skinny); store=(cache, layer): w is the packed QKV projection and x holds one token per cache row; the K and
    V thirds of the result are also written to row cache.lens[b] of `layer` (KVCache.store's rule; lens is unchanged).
    CPU tensors take the explicit f32 composition of the same steps."""
    a = act_code(act)
    cache, layer = store if store is not None else (None, None)
    if cache is not None and getattr(cache, "fp8", False):
        raise ValueError("dense_skinny_fused(store=): the cache-store epilogue has no fp8-cache variant")
    if not on_gpu(x):
        h = x
        if ln is not None:
            h = torch.nn.functional.layer_norm(x.float(), (x.shape[-1],), ln[0], ln[1], ln[2]).to(x.dtype)
        y = _act_ref(torch.nn.functional.linear(h.to(w.dtype), w, bias), a)
        if residual is not None:
            y = residual + y
        if cache is not None:
            cache.store(layer, y.reshape(cache.batch, 1, -1))
        return y
    w16 = w if w.dtype == BF16 else bf16_shadow(w)
    w16 = w16.contiguous()
    x2 = x.reshape(-1, x.shape[-1])
    x2 = (x2 if x2.dtype == BF16 else x2.to(BF16)).contiguous()
    if bias is not None and (bias.dtype != F32 or not bias.is_contiguous()):
        bias = bias.float().contiguous()
    M, Kd = x2.shape
    N = w16.shape[0]
    if w16.shape[1] != Kd:
        raise ValueError(f"dense_skinny_fused: x [..., {Kd}] against w {tuple(w16.shape)}")
    gamma = beta = None
    eps = 0.0
    if ln is not None:
        gamma, beta = (t.detach().float().contiguous() for t in ln[:2])
        eps = float(ln[2])
        if gamma.numel() != Kd or beta.numel() != Kd or Kd > ln_max_k():
            raise ValueError(f"dense_skinny_fused: LayerNorm of width {Kd} (gamma {gamma.numel()}, beta {beta.numel()}, "
                             f"at most {ln_max_k()})")
    if residual is not None:
        if residual.numel() != M * N:
            raise ValueError(f"dense_skinny_fused: residual {tuple(residual.shape)} against an output [{M}, {N}]")
        residual = (residual if residual.dtype == BF16 else residual.to(BF16)).contiguous()
    kc = vc = lens = None
    H = Smax = 0
    if cache is not None:
        if (not on_gpu(cache.k) or cache.batch != M or N != 3 * cache.heads * HEAD_DIM or cache.head_dim != HEAD_DIM
                or not 0 <= layer < cache.layers):
            raise ValueError(f"dense_skinny_fused: an output [{M}, {N}] / layer {layer} does not fit the cache (batch "
                             f"{cache.batch}, heads {cache.heads}, head dim {cache.head_dim}, layers {cache.layers})")
        kc, vc, lens, H, Smax = cache.k[layer], cache.v[layer], cache.lens, cache.heads, cache.capacity
        cache.empty = False
    out = torch.empty(M, N, dtype=BF16, device=x.device)
    call("dtf_dense_skinny_fused", ptr(x2), ptr(w16), ptr(bias), ptr(out), M, N, Kd, a, ptr(gamma), ptr(beta), eps,
         ptr(residual), ptr(kc), ptr(vc), ptr(lens), H, Smax, stream(x.device))
    return out.reshape(*x.shape[:-1], N)


# (N, K) of projections that the decode step keeps on ops.dense because dense_skinny measured slower there
# (tools/bench_generate.py, profiles/generate_decode.txt)
SKINNY_EXCLUDE = frozenset()
# the same for dense_wide inside the wide step (generate(step="wide")) at 17 to 64 rows. The GPT-2 LM head
# 1024 -> 50304: 1.08x faster than ops.dense at M = 17, but 0.9x / 0.8x / 0.7x at M = 32 / 48 / 64 (section 7)
WIDE_EXCLUDE = frozenset({(50304, 1024)})
# the same for dense_tall inside the tall step (generate(step="tall")) at 65 to 256 rows. The four layer projections
# are 1.27x to 4.46x faster than ops.dense at M = 65, 128, 192 and 256; the LM head 1024 -> 50304 takes 50 / 56 / 73 /
# 88 us against 37 to 41 us (0.74x to 0.46x; the best variant 48 / 56 / 64 / 75 us), section 10
TALL_EXCLUDE = frozenset({(50304, 1024)})


def step_dense(x, w, bias=None, act=None, wide=False, tall=False):
    """A projection of the one-token decode step: dense_skinny from the bf16 shadow of w wherever it applies.
    wide=True (the opt-in wide step): with 17 to 64 rows dense_wide instead of ops.dense; up to 16 rows unchanged.
    tall=True (the opt-in tall step): the wide route up to 64 rows, and with 65 to 256 rows dense_tall."""
    if on_gpu(x):
        M = x.numel() // x.shape[-1]
        N, Kd = w.shape
        if M <= 16 and N % 8 == 0 and Kd % 8 == 0 and (N, Kd) not in SKINNY_EXCLUDE:
            return dense_skinny(x, w, bias, act)
        if ((wide or tall) and 16 < M <= WIDE_MAX_ROWS and N % 8 == 0 and Kd % 8 == 0
                and (N, Kd) not in WIDE_EXCLUDE):
            return dense_wide(x, w, bias, act)
        if (tall and WIDE_MAX_ROWS < M <= TALL_MAX_ROWS and N % 8 == 0 and Kd % 8 == 0
                and (N, Kd) not in TALL_EXCLUDE):
            return dense_tall(x, w, bias, act)
    return dense(x, w, bias, act=act)
