"""Beam selection: the G best continuations of a group of G beams (csrc/kernels/beam.hip), the choice of
``GPT2.generate(num_beams=G)``.

The rule. Rows g * G .. g * G + G - 1 of logits are the beams of group g. A live beam j offers every token v < n with
value ``scores[j] + (logits[j, v] - lse_j)``, lse_j the log-sum-exp of the row's n entries; a done beam offers the
single pair (j, pad) with value ``scores[j]``. Everything is f32; NaN counts as -inf, and -inf is a legal value that
loses to anything finite. The G largest values win, ties to the smaller j * n + v, in descending order: the new
``scores``, ``parent`` (which beam of the group the winner continues), ``token``, and ``done`` (the parent's, or token
== eos). Scores ``[0, -inf, ...]`` per group over G copies of the prompt's logits therefore give the G best first
tokens. The sibling step is ``KVCache.reorder(parent, ...)`` (ops/decode.py).
"""
from __future__ import annotations

import torch

from ._util import BF16, F32, call, on_gpu, ptr, stream

MAX_N = 65536
MAX_GROUP = 16


def beam_select_reference(logits, *, n, scores, done, group, eos=None, pad=0):
    """The rule above in plain torch on CPU tensors (log_softmax, then a stable sort on (-value, index)): the CPU path
    of `beam_select`. Updates scores and done in place -> (parent int32, token int64)."""
    G, n = int(group), int(n)
    B = logits.shape[0]
    val = scores.float()[:, None] + torch.log_softmax(logits.detach().float()[:, :n], -1)
    val = torch.nan_to_num(val, nan=float("-inf"), posinf=float("inf"), neginf=float("-inf"))
    tok_of = torch.arange(n).repeat(G)
    beam_of = torch.arange(G).repeat_interleave(n)
    parent = torch.empty(B, dtype=torch.int32)
    token = torch.empty(B, dtype=torch.int64)
    new_scores, new_done = scores.clone(), done.clone()
    for g in range(B // G):
        rows = slice(g * G, g * G + G)
        live = ~done[rows]
        # candidates in index order: a live beam's n tokens, a done beam's one pair at index j * n + pad
        keep = live.repeat_interleave(n)
        v, bj, tk = val[rows].reshape(-1)[keep], beam_of[keep], tok_of[keep]
        dj = torch.nonzero(~live)[:, 0]
        v = torch.cat([v, scores[rows][dj].float()])
        bj = torch.cat([bj, dj])
        tk = torch.cat([tk, torch.full_like(dj, int(pad))])
        order = torch.argsort(bj * n + tk, stable=True)
        v, bj, tk = v[order], bj[order], tk[order]
        top = torch.sort(-torch.nan_to_num(v, nan=float("-inf")), stable=True).indices[:G]
        parent[rows], token[rows], new_scores[rows] = bj[top].int(), tk[top], v[top]
        d = done[rows][bj[top]]
        new_done[rows] = d | (tk[top] == int(eos)) if eos is not None else d
    scores.copy_(new_scores)
    done.copy_(new_done)
    return parent, token


def beam_select(logits, *, n, scores, done, group, eos=None, pad=0):
    """The G = group best continuations of every group of G rows of logits [B0 * G, ld] (bf16 or f32; the first n
    entries of a row count, G <= n <= 65536, ld % 8 == 0) by the rule of this module -> (parent [B0 * G] int32 in
    0 .. G-1, token [B0 * G] int64). scores [B0 * G] f32 and done [B0 * G] bool are updated in place, descending within
    a group. 0 <= pad < 65536. GPU tensors take two launches (one block per row, one wave per group) that read no device
    value on the host (hipGraph-capturable) and give the same bits on every call; CPU tensors take
    `beam_select_reference`."""
    G, n = int(group), int(n)
    if not 2 <= G <= MAX_GROUP:
        raise ValueError(f"beam_select: group {group} (2..{MAX_GROUP})")
    if not G <= n <= MAX_N:
        raise ValueError(f"beam_select: n = {n} outside [{G}, {MAX_N}]")
    if not 0 <= int(pad) < MAX_N:
        raise ValueError(f"beam_select: pad {pad} outside [0, {MAX_N})")
    if logits.dim() != 2 or logits.stride(1) != 1 or logits.shape[0] % G or logits.shape[0] < G:
        raise ValueError(f"beam_select: logits must be [B0 * {G}, ld] with unit inner stride, got {tuple(logits.shape)}")
    B = logits.shape[0]
    ld = logits.stride(0)
    if n > logits.shape[1] or n > ld:
        raise ValueError(f"beam_select: n = {n} exceeds the row ({logits.shape[1]} entries, stride {ld})")
    if logits.dtype not in (BF16, F32):
        raise ValueError(f"beam_select: logits {logits.dtype} (bf16 or f32)")
    if tuple(scores.shape) != (B,) or tuple(done.shape) != (B,) or scores.dtype != F32 or done.dtype != torch.bool:
        raise ValueError(f"beam_select: scores f32 [{B}] and done bool [{B}], got {tuple(scores.shape)} {scores.dtype}, "
                         f"{tuple(done.shape)} {done.dtype}")
    if not (scores.is_contiguous() and done.is_contiguous()):
        raise ValueError("beam_select: scores and done must be contiguous (they are updated in place)")
    if len({t.device for t in (logits, scores, done)}) != 1:
        raise ValueError("beam_select: tensors on different devices")
    if not on_gpu(logits):
        return beam_select_reference(logits, n=n, scores=scores, done=done, group=G, eos=eos, pad=pad)
    if ld % 8 or logits.data_ptr() % 16:
        raise ValueError(f"beam_select: row stride {ld} must be a multiple of 8 and logits 16-byte aligned")
    dev = logits.device
    parent = torch.empty(B, dtype=torch.int32, device=dev)
    token = torch.empty(B, dtype=torch.int64, device=dev)
    scratch = torch.empty(B * G * 2, dtype=torch.int32, device=dev)
    call("dtf_beam_select", ptr(logits), int(logits.dtype == F32), ld, B // G, G, n, ptr(scores), ptr(done),
         -1 if eos is None else int(eos), int(pad), ptr(parent), ptr(token), ptr(scratch), stream(dev))
    return parent, token
