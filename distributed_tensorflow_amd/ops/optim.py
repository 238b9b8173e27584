"""Fused optimizer apply (csrc/kernels/optim.hip, optim_layerwise.hip) over flat f32 arenas."""
from __future__ import annotations

import torch

from ._util import K, call, ptr, step_abort_ptr, stream

KINDS = {"sgd": 0, "adam": 1, "adagrad": 2, "adadelta": 3, "ftrl": 4, "rmsprop": 5, "lamb": 6, "lars": 7}

# layer-wise rules (optim_layerwise.hip)
LW_TILE = 4096                 # elements per tile at most (the kernels' compile-time LW_TILE)
LW_DECAY, LW_ADAPT = 1, 2      # per-variable flag bits
LW_SUM, LW_SCALE = 1, 2        # finalize modes


def optim_apply(kind, p, g, s1, s2, p16, hp, *, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, mom=0.0, l1=0.0, l2=0.0,
                nesterov=False, zero_grad=False, sumsq=None):
    """One streaming launch: update p (and slots s1/s2), write the bf16 copy p16, optionally zero g. Inside a
    per-stream hipGraph capture the kernel also reads the capture's error flag and applies nothing once a
    cross-stream wait of the step timed out (graph_sync.hip)."""
    k = KINDS[kind] if isinstance(kind, str) else int(kind)
    call("dtf_optim_apply", k, ptr(p), ptr(g), ptr(s1), ptr(s2), ptr(p16), p.numel(), float(b1), float(b2),
         float(eps), float(wd), float(mom), float(l1), float(l2), int(nesterov), int(zero_grad), ptr(hp), ptr(sumsq),
         step_abort_ptr(), stream())


def sumsq(x, out, zero=True):
    call("dtf_sumsq", ptr(x), x.numel(), ptr(out), int(zero), stream())


def layerwise_tiles(pieces, tile=LW_TILE):
    """Tile table rows (param offset, grad offset, length, variable index) for ``pieces`` = [(param offset, grad
    offset, length, variable index)] in arena order: every piece is cut into tiles of at most ``tile`` elements, so
    no tile crosses a piece (a variable) and a variable's tiles are consecutive. Offsets and lengths must be
    multiples of 16 (every access of the kernels is a 16-byte vector access)."""
    rows = []
    for po, go, n, var in pieces:
        if (po | go | n) % 16:
            raise ValueError(f"layer-wise piece {(po, go, n, var)} is not 16-element aligned")
        for o in range(0, n, tile):
            rows.append((po + o, go + o, min(tile, n - o), var))
    return rows


class LayerwisePlan:
    """The static state of the layer-wise kernels for one (arena, gradient buffer) pair: the tile table on the host
    (validated by every entry point before it launches) and on the device, per-variable flags, the per-tile
    partial sums, the per-variable sums and the per-variable scale. Built once, outside any capture."""

    def __init__(self, rows, flags, n_param, n_grad, device):
        self.nvars = len(flags)
        self.ntiles = len(rows)
        self.n_param, self.n_grad = int(n_param), int(n_grad)
        self.host = torch.tensor(rows, dtype=torch.int64).reshape(-1, 4).contiguous()
        self.flags_host = list(flags)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            if K().dtf_lw_tile_elems() != LW_TILE:
                raise RuntimeError("optim_layerwise.hip was built with another LW_TILE than ops.optim.LW_TILE")
            self.dev = self.host.to(self.device)
            self.flags = torch.tensor(self.flags_host, dtype=torch.int32, device=self.device)
            self.partials = torch.zeros(max(1, self.ntiles), 2, dtype=torch.float32, device=self.device)
            self.sums = torch.zeros(self.nvars, 2, dtype=torch.float32, device=self.device)
            self.scale = torch.ones(self.nvars, dtype=torch.float32, device=self.device)

    def _table(self):
        return (self.host.data_ptr(), ptr(self.dev), self.ntiles, self.nvars, self.n_param, self.n_grad)


def _gptr(g):
    """The gradient buffer the table's gradient offsets count from: a tensor, or the raw device address of the
    compact shard buffer (ZeRO-1: the segments' gradients are views of it)."""
    return g if isinstance(g, int) else ptr(g)


def layerwise_pass1(kind, plan, p, g, s1, s2, hp, *, b1=0.9, b2=0.999, eps=1e-6, wd=0.0, sumsq=None):
    """Pass 1 over the plan's tiles. LAMB: update m (s1) and v (s2), write the un-scaled step u into g, store the
    per-tile partial sums of w^2 and u^2. LARS: store the partial sums of w^2 and (scaled g)^2."""
    call("dtf_lw_pass1", KINDS[kind], *plan._table(), ptr(p), _gptr(g), ptr(s1), ptr(s2), ptr(plan.flags),
         ptr(plan.partials), float(b1), float(b2), 1.0 - float(b1), 1.0 - float(b2), float(eps), float(wd), ptr(hp),
         ptr(sumsq), step_abort_ptr(), stream())


def layerwise_finalize(kind, plan, *, mode=LW_SUM | LW_SCALE, wd=0.0, eeta=0.001, eps=0.0):
    """One wave per variable: LW_SUM adds the variable's tile partials in table order (into plan.sums), LW_SCALE
    turns the sums (its own, or plan.sums after a reduction over replicas) into plan.scale."""
    call("dtf_lw_finalize", KINDS[kind], int(mode), *plan._table(), ptr(plan.partials), ptr(plan.sums),
         ptr(plan.flags), ptr(plan.scale), float(wd), float(eeta), float(eps), step_abort_ptr(), stream())


def layerwise_pass2(kind, plan, p, g, s1, p16, hp, *, wd=0.0, mom=0.0, nesterov=False, zero_grad=True, sumsq=None):
    """Pass 2 over the plan's tiles: the weight update with lr*scale[var], the bf16 copy, the zeroed gradient."""
    call("dtf_lw_pass2", KINDS[kind], *plan._table(), ptr(p), _gptr(g), ptr(s1), ptr(p16), ptr(plan.scale),
         ptr(plan.flags), float(wd), float(mom), int(nesterov), int(zero_grad), ptr(hp), ptr(sumsq),
         step_abort_ptr(), stream())
