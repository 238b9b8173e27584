"""The token sampler of ``GPT2.generate``: repetition penalty, temperature, top-k, nucleus (top-p) and the draw, with
the row bookkeeping of the generation loop, as one kernel launch per token (csrc/kernels/sample.hip).

The rule is written so that a host replica reproduces the kernel bit for bit: the only floating-point operations are
single IEEE f32 multiplies and subtractions, probabilities are integer masses, and the draw is a counter hash. The same
logits therefore give the same tokens on the CPU and on the GPU, eagerly and inside a replayed hipGraph, and for a row
sampled alone or among others at the same row index.

Per row b, with logits x[0..n):

1. z_i = f32(x_i). Repetition penalty r (1 = off) on every token id in out[b, 0:pos[b]] (ids outside [0, n) ignored):
   z_i * f32(1/r) if z_i > 0 else z_i * f32(r). Temperature: z_i * f32(1/T). NaN counts as -inf.
2. T == 0 is greedy: the lowest index attaining max z after the penalty; top_k and top_p are ignored.
3. top_k (None, 0 or >= n: off): keep z_i >= the k-th largest value (ties kept).
4. Masses, with m = max z: t_i = (m - z_i) * f32(log2 e); q_i = 0 unless 0 <= t_i < 40; else F = floor(t_i * 65536),
   e = F >> 16, idx = (F >> 8) & 255, rem = F & 255, v = TAB[idx] - (((TAB[idx] - TAB[idx + 1]) * rem) >> 8),
   q_i = v >> e, where TAB[j] = round(2^31 * 2^(-j/256)), j = 0..256 (``mass_table``: built once here, handed to the
   kernel as a device tensor).
5. top_p (None or >= 1: off) over the top-k survivors: W = sum q, P = round(p * 65536), need = (P*W + 65535) >> 16; the
   threshold is the largest value v with sum{q_i : z_i >= v} >= need; keep z_i >= v (ties kept, the maximum always
   kept). A p so close to 1 that P reaches 65536 keeps every element that has mass, which draws the same token as no
   filter, so it is treated as off.
6. Draw: U = mix64(mix64(seed + G*(b+1)) + G*(pos[b]+1)) >> 32 (mix64 and G of the dropout kernels, u64 wrap-around),
   or uniform[b] when given; target = floor(U * W' / 2^32) with W' the kept mass; the token is the smallest kept index
   whose inclusive prefix sum of q in index order exceeds target; 0 when W' == 0.
7. Bookkeeping: done[b] -> the token is pad; done[b] |= (tok == eos) when eos >= 0; out[b, pos[b]] = tok when
   pos[b] < out.shape[1]; pos[b] += 1.
"""
from __future__ import annotations

import numpy as np
import torch

from ._util import BF16, F32, call, on_gpu, ptr, stream

MAX_N = 65536
_M64 = (1 << 64) - 1
_G = 0x9E3779B97F4A7C15
_LOG2E = np.float32(1.4426950408889634)
_TABLES = {}


def mass_table(device=None):
    """TAB[j] = round(2^31 * 2^(-j/256)), j = 0..256, int64 (numpy on the host, a cached tensor on `device`)."""
    t = _TABLES.get("host")
    if t is None:
        t = np.array([int(round(2.0 ** 31 * 2.0 ** (-j / 256.0))) for j in range(257)], dtype=np.int64)
        _TABLES["host"] = t
    if device is None:
        return t
    key = (device.type, device.index)
    d = _TABLES.get(key)
    if d is None:
        d = _TABLES[key] = torch.from_numpy(t).to(device)
    return d


def _mix64(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def hash_uniform(seed, row, pos):
    """The 32-bit draw of row `row` at position `pos`."""
    return _mix64(_mix64(seed + _G * (row + 1)) + _G * (pos + 1)) >> 32


def masses(z, keep=None):
    """Integer masses q (int64) of the f32 vector z against its maximum (clause 4); 0 where `keep` is False."""
    z = np.asarray(z, dtype=np.float32)
    tab = mass_table()
    with np.errstate(invalid="ignore", over="ignore"):
        t = (z.max() - z) * _LOG2E
        ok = (t >= np.float32(0)) & (t < np.float32(40))
        F = np.floor(np.where(ok, t, np.float32(0)) * np.float32(65536)).astype(np.int64)
    e, idx, rem = F >> 16, (F >> 8) & 255, F & 255
    v = tab[idx] - (((tab[idx] - tab[idx + 1]) * rem) >> 8)
    q = np.where(ok, v >> e, 0).astype(np.int64)
    return q if keep is None else np.where(keep, q, 0)


def _settings(n, temperature, top_k, top_p, repetition_penalty, seed):
    n = int(n)
    if not 1 <= n <= MAX_N:
        raise ValueError(f"sample_logits: n = {n} outside [1, {MAX_N}]")
    T = 0.0 if temperature is None else float(temperature)
    if T < 0 or T != T:
        raise ValueError(f"sample_logits: temperature {temperature}")
    r = 1.0 if repetition_penalty is None else float(repetition_penalty)
    if not r > 0:
        raise ValueError(f"sample_logits: repetition_penalty {repetition_penalty}")
    k = 0 if top_k is None else int(top_k)
    if k < 0:
        raise ValueError(f"sample_logits: top_k {top_k}")
    if k >= n:
        k = 0
    P = -1
    if top_p is not None:
        p = float(top_p)
        if not p >= 0:
            raise ValueError(f"sample_logits: top_p {top_p}")
        if p < 1:
            P = int(round(p * 65536))
            if P >= 65536:
                P = -1
    return dict(n=n, greedy=T == 0, inv_t=np.float32(1.0 / T) if T else np.float32(1), k=k, P=P, r=np.float32(r),
                inv_r=np.float32(1.0 / r), seed=(0 if seed is None else int(seed)) & _M64)


def _pick_row(x, s, hist, U):
    """Clauses 1-6 for one row: x f32 [n], hist the row's earlier token ids, U the 32-bit draw or None (greedy)."""
    n = s["n"]
    z = x.astype(np.float32, copy=True)
    with np.errstate(invalid="ignore", over="ignore"):
        if s["r"] != np.float32(1):
            ids = hist[(hist >= 0) & (hist < n)]
            hit = np.zeros(n, dtype=bool)
            hit[ids] = True
            z = np.where(hit, np.where(z > 0, z * s["inv_r"], z * s["r"]), z).astype(np.float32)
        if not s["greedy"]:
            z = (z * s["inv_t"]).astype(np.float32)
    z[np.isnan(z)] = -np.inf
    if s["greedy"]:
        return int(np.argmax(z))
    keep = np.ones(n, dtype=bool)
    if s["k"]:
        keep = z >= np.partition(z, n - s["k"])[n - s["k"]]
    q = masses(z, keep)
    if s["P"] >= 0:
        W = int(q.sum())
        if W:
            need = max((s["P"] * W + 65535) >> 16, 1)
            order = np.argsort(-z, kind="stable")
            cs = np.cumsum(q[order])
            v = z[order[int(np.searchsorted(cs, need, side="left"))]]
            keep &= z >= v
            q = np.where(keep, q, 0)
    cs = np.cumsum(q)
    Wk = int(cs[-1])
    if Wk == 0:
        return 0
    target = (int(U) * Wk) >> 32
    return int(np.searchsorted(cs, target, side="right"))


def sample_reference(logits, *, n, temperature=0.0, top_k=None, top_p=None, repetition_penalty=None, seed=None, out,
                     pos, done, eos=None, pad=0, uniform=None):
    """The rule of this module in numpy integers and float32, on CPU tensors: the host replica of the kernel and the
    CPU path of `sample_logits`. Updates out, pos and done in place like the kernel -> tok [B] int64."""
    s = _settings(n, temperature, top_k, top_p, repetition_penalty, seed)
    x = logits.detach().float().numpy()
    B = x.shape[0]
    o, ps, dn = out.numpy(), pos.numpy(), done.numpy()  # views: written in place
    width = o.shape[1]
    eos = -1 if eos is None else int(eos)
    toks = np.zeros(B, dtype=np.int64)
    for b in range(B):
        p0 = int(ps[b])
        U = None
        if not s["greedy"]:
            U = (int(uniform[b]) & 0xFFFFFFFF) if uniform is not None else hash_uniform(s["seed"], b, p0)
        tok = _pick_row(x[b, :s["n"]], s, o[b, :min(max(p0, 0), width)], U)
        if dn[b]:
            tok = int(pad)
        if eos >= 0 and tok == eos:
            dn[b] = True
        if 0 <= p0 < width:
            o[b, p0] = tok
        ps[b] = p0 + 1
        toks[b] = tok
    return torch.from_numpy(toks)


def _check(logits, n, out, pos, done, uniform):
    if logits.dim() != 2 or logits.stride(1) != 1:
        raise ValueError(f"sample_logits: logits must be [B, ld] with unit inner stride, got {tuple(logits.shape)}")
    B = logits.shape[0]
    ld = logits.stride(0) if B > 1 else logits.shape[1]
    if n > logits.shape[1] or n > ld:
        raise ValueError(f"sample_logits: n = {n} exceeds the row ({logits.shape[1]} entries, stride {ld})")
    if ld % 8:
        raise ValueError(f"sample_logits: row stride {ld} is not a multiple of 8")
    if logits.dtype not in (BF16, F32):
        raise ValueError(f"sample_logits: logits {logits.dtype} (bf16 or f32)")
    if out.dim() != 2 or out.shape[0] != B or tuple(pos.shape) != (B,) or tuple(done.shape) != (B,):
        raise ValueError(f"sample_logits: out {tuple(out.shape)}, pos {tuple(pos.shape)}, done {tuple(done.shape)} "
                         f"against {B} rows")
    if out.dtype != torch.int64 or pos.dtype != torch.int64 or done.dtype != torch.bool:
        raise ValueError("sample_logits: out and pos are int64, done is bool")
    if not (out.is_contiguous() and pos.is_contiguous() and done.is_contiguous()):
        raise ValueError("sample_logits: out, pos and done must be contiguous (they are updated in place)")
    same = {t.device for t in (logits, out, pos, done)}
    if uniform is not None:
        if tuple(uniform.shape) != (B,) or uniform.dtype != torch.int64 or not uniform.is_contiguous():
            raise ValueError("sample_logits: uniform is a contiguous int64 [B] of values in [0, 2^32)")
        same.add(uniform.device)
    if len(same) != 1:
        raise ValueError(f"sample_logits: tensors on different devices {sorted(map(str, same))}")
    return B, ld


def sample_logits(logits, *, n, temperature=0.0, top_k=None, top_p=None, repetition_penalty=None, seed=None, out, pos,
                  done, eos=None, pad=0, uniform=None):
    """One token per row of logits [B, ld] (bf16 or f32; the first n entries of a row count, n <= 65536, ld % 8 == 0) by
    the rule of this module -> tok [B] int64. out [B, width] int64 holds each row's tokens so far (pos[b] of them: the
    penalty set) and receives the new one at pos[b]; pos [B] int64 and done [B] bool are updated in place. `uniform`
    (int64 [B], values in [0, 2^32)) replaces the hash draw. GPU tensors take one launch of the fused kernel, which
    reads no device value on the host (hipGraph-capturable); CPU tensors take `sample_reference`."""
    s = _settings(n, temperature, top_k, top_p, repetition_penalty, seed)
    B, ld = _check(logits, s["n"], out, pos, done, uniform)
    if not on_gpu(logits):
        return sample_reference(logits, n=n, temperature=temperature, top_k=top_k, top_p=top_p,
                                repetition_penalty=repetition_penalty, seed=seed, out=out, pos=pos, done=done, eos=eos,
                                pad=pad, uniform=uniform)
    if logits.data_ptr() % 16:
        raise ValueError("sample_logits: logits must be 16-byte aligned")
    dev = logits.device
    tok = torch.empty(B, dtype=torch.int64, device=dev)
    call("dtf_sample_logits", ptr(logits), int(logits.dtype == F32), ld, B, s["n"], float(s["inv_t"]), int(s["greedy"]),
         s["k"], s["P"], float(s["r"]), float(s["inv_r"]), s["seed"], ptr(uniform), ptr(mass_table(dev)), ptr(out),
         out.shape[1], ptr(pos), ptr(done), -1 if eos is None else int(eos), int(pad), ptr(tok), stream(dev))
    return tok
