"""NHWC Conv2D (+ fused FusedBatchNorm / residual / ReLU) on the gfx950 implicit-GEMM kernel.

Activations are channels-last ``[N, H, W, C]`` bf16; filters are stored KRSC
(``[out, kh, kw, in]``) as f32 master variables with a bf16 compute shadow.
The training-mode BatchNorm statistics are produced by the conv epilogue
(per-M-tile partial sum / sum^2 rows, reduced deterministically by bn_finalize)
so the forward BN costs one apply pass
instead of three (SURVEY §2.4.b K4/K5, §7.4 hard part 1).
"""
from __future__ import annotations

import os

import torch

from ._util import (BF16, F32, SIDE_STREAM_ON, IntOut, K as K_, before_overwrite, bf16_shadow, call, contig,
                    crsk_shadow, direct_grad, fork_side, mark_parked, on_gpu, ptr, stream, workspace)


def out_size(h, k, s, p, d=1):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


def same_pads(h, k, s, d=1):
    """TF 'SAME' padding (pad_top, pad_total) for one spatial dim."""
    out = (h + s - 1) // s
    total = max((out - 1) * s + (k - 1) * d + 1 - h, 0)
    return total // 2, total


def _geom(x, w, stride, pad, dil):
    N, H, W, C = x.shape
    K, R, S, C2 = w.shape
    assert C == C2, f"channel mismatch {C} vs {C2}"
    sh, sw = stride
    ph, pw = pad
    dh, dw = dil
    P = out_size(H, R, sh, ph, dh)
    Q = out_size(W, S, sw, pw, dw)
    return N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw


def _partial_rows(want, cap, width, device):
    """Up to `cap` BatchNorm partial-sum rows ([2 * width] f32) for a kernel epilogue to write: the buffer, the row
    counter the launch fills in and the (pointer, counter address) pair to launch with; Nones when not wanted."""
    if not want:
        return None, None, (None, None)
    part, rows = torch.empty(cap * 2 * width, dtype=F32, device=device), IntOut()
    return part, rows, (ptr(part), rows.addr)


def _bn_ptrs(bn):
    """Pointers of a _BNSource's BN input (materialised first if it was not stored), ReLU bits and batch mean."""
    return (ptr(bn.materialize()), ptr(bn.mbits), ptr(bn.mean)) if bn is not None else (None, None, None)


def conv_fwd_raw(x, w16, g, stats=False, bias=None, act=0):
    """Returns y, or (y, partials, rows) when stats: BN partial sums, one [2K] row per M-tile."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw = g
    y = torch.empty((N, P, Q, K), dtype=BF16, device=x.device)
    part, rows, row_args = _partial_rows(stats, (N * P * Q + 63) // 64, K, x.device)
    call("dtf_conv_fwd", ptr(x), ptr(w16), ptr(y), ptr(bias), *row_args, N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh,
         dw, int(act), 0, -1, stream())
    return (y, part, rows.value) if stats else y


def conv_fwd_bn_raw(x, w16, g, gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean, invstd):
    """Training ConvBN forward: y plus the output BatchNorm's scale/shift/mean/invstd and running-statistics update,
    finalized inside the conv launch's tail (gemm_core.h BnFin) — or by the separate reduction + finalize launches
    when the launch cannot (the native side falls back by itself)."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw = g
    y = torch.empty((N, P, Q, K), dtype=BF16, device=x.device)
    part = torch.empty(((N * P * Q + 63) // 64) * 2 * K, dtype=F32, device=x.device)
    call("dtf_conv_fwd_bn", ptr(x), ptr(w16), ptr(y), ptr(part), N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw,
         -1, ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), float(momentum), float(eps), ptr(scale), ptr(shift),
         ptr(mean), ptr(invstd), None, stream())
    return y


def conv_dgrad_raw(dy, w_master, g, acc=None, bn=None, acc_mask=None, acc_sub2=None):
    """dX (bf16); with `acc` (a bf16 [N,H,W,C] gradient already holding another contribution) the epilogue
    adds into it (beta = 1) and returns it; `acc_mask` (1 bit per element) first zeroes the acc values whose
    bit is clear (a residual gradient whose ReLU mask was deferred). With `bn` (the _BNSource of the
    BatchNorm whose output this conv consumed) the epilogue also produces that BatchNorm's backward
    reduction of the final dX values and stores it on `bn` (see _BNSource)."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw = g
    wc = crsk_shadow(w_master, K, R * S, C)
    dx = torch.empty((N, H, W, C), dtype=BF16, device=dy.device) if acc is None else acc
    ws = workspace(dy.device)  # strided convs: per-phase compact filters (bf16) live here
    # one partial row per M-tile (>= 64 rows) of every launch: a strided dgrad runs sh*sw phase launches, each of
    # which may end in a partial tile
    part, rows, row_args = _partial_rows(bn is not None, (N * H * W + 63) // 64 + sh * sw, C, dy.device)
    if acc_sub2 is not None:  # + the compact gradient of a stride-2 1x1 shortcut at the even pixels
        assert acc is None and (R, S, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0)
    args = (ptr(dy), ptr(wc), ptr(dx), N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw,
            1.0 if (acc is not None or acc_sub2 is not None) else 0.0, ptr(ws), 2 * ws.numel())
    tail = (*row_args, ptr(acc_mask) if acc is not None else None, ptr(acc_sub2))
    recomputed = False
    if bn is not None and bn.yc is None:
        # the BN input was not stored: the launch recomputes it per tile from the producer's input and filter, or
        # answers -12 without launching when the shape's route cannot (only the persistent pointwise route can)
        rc = K_().dtf_conv_dgrad_x(*args, None, ptr(bn.mbits), ptr(bn.mean), *tail, ptr(bn.rx),
                                   ptr(bf16_shadow(bn.rw)), stream())
        if rc not in (0, -12):
            raise RuntimeError(f"dtf_conv_dgrad_x failed with status {rc}")
        recomputed = rc == 0
    if not recomputed:
        call("dtf_conv_dgrad_x", *args, *_bn_ptrs(bn), *tail, None, None, stream())
    if bn is not None:
        bn.provide(dx, part, rows.value)
    return dx


def _recompute_y(x, w, g):
    """bf16(x w^T) of a stage-1 channel-expanding 1x1 conv whose output was not stored, with the pointwise forward
    kernel the two-pass forward used (the same MFMA sequence: bitwise its values)."""
    N, H, W, C, K = g[:5]
    M = N * H * W
    y = torch.empty((N, H, W, K), dtype=BF16, device=x.device)
    stats, _, row_args = _partial_rows(True, (M + 63) // 64, K, x.device)  # (always written; not used here)
    call("dtf_pwconv_fwd", ptr(x), ptr(bf16_shadow(w)), ptr(y), *row_args, M, C, K, stream())
    return y


def pw_bwd_ok(g, M_min=64 * 256):
    """Shapes of the fused 1x1 data + weight gradient (pwbwd.hip): stride-1 unpadded 1x1, K_out 256 from C_in 64
    (ResNet-50 stage-1 c3 and stride-1 projection), >= 256 pixel tiles, tensors < 2 GiB."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw = g[:13]
    M = N * P * Q
    return ((R, S, sh, sw, ph, pw) == (1, 1, 1, 1, 0, 0) and K == 256 and C == 64 and M >= M_min
            and M * K * 2 < (1 << 31))


def pw_bwd_bn_ok(g):
    """Shapes of the BatchNorm-folded form (dtf_pw_conv_bwd_bn): stage 1 (K_out 256 from 64, >= 256 64-pixel tiles)
    or stage 2 (K_out 512 from 128, >= 128 32-pixel tiles)."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw = g[:13]
    M = N * P * Q
    if (R, S, sh, sw, ph, pw) != (1, 1, 1, 1, 0, 0) or M * K * 2 >= (1 << 31):
        return False
    return (K, C) == (256, 64) and M >= 64 * 256 or (K, C) == (512, 128) and M >= 32 * 128


def conv_bwd_fused_raw(dy, x, w_master, g, dw_out, bn=None):
    """dX (bf16) and dW += (into the f32 arena gradient dw_out) of a pw_bwd_ok conv in ONE pass over dy
    (pwbwd.hip); with `bn` (the _BNSource of the BatchNorm that produced x, see conv_dgrad_raw) the BN-backward
    partial rows of dX go to it."""
    N, H, W, C, K = g[:5]
    M = N * H * W
    wc = crsk_shadow(w_master, K, 1, C)
    dx = torch.empty((N, H, W, C), dtype=BF16, device=dy.device)
    ws = workspace(dy.device)
    part, rows, row_args = _partial_rows(bn is not None, 256, C, dy.device)  # (<= 256 pixel slots)
    call("dtf_pw_conv_bwd", ptr(dy), ptr(x), ptr(wc), ptr(dx), ptr(dw_out), 1, *_bn_ptrs(bn), *row_args, ptr(ws),
         ws.numel(), M, K, C, stream())
    if bn is not None:
        bn.provide(dx, part, rows.value)
    return dx


def conv_bwd_bn_fused_raw(dout, y, ymask, coef, x, w_master, g, dw_out, bn=None, sc=None, wy=None):
    """conv_bwd_fused_raw with dy = a*dz + b*y + c (the BatchNorm(+ReLU) backward of y = conv output, coefficients
    coef [3K] from dtf_bn_bwd_coef, dz = dout under the ReLU bits ymask) computed inside the kernel. With `sc` (the
    _BNSource of a deferred projection-shortcut BN added as this layer's residual) the kernel also takes that BN's
    backward reduction of dz and provides it to the source for `dout`, together with ymask: the shortcut's backward then
    receives the raw dout and applies the ReLU bits itself (no dz is materialised). With `wy` (the layer's bf16 forward
    filter) and y None, y is recomputed per tile from x (it was not stored)."""
    N, H, W, C, K = g[:5]
    M = N * H * W
    wc = crsk_shadow(w_master, K, 1, C)
    dx = torch.empty((N, H, W, C), dtype=BF16, device=dout.device)
    ws = workspace(dout.device)
    part, rows, row_args = _partial_rows(bn is not None, 256, C, dout.device)  # (<= 256 pixel slots)
    psc, rsc, sc_args = _partial_rows(sc is not None, 256, K, dout.device)
    sc_ptrs = (ptr(sc.yc), ptr(sc.mean)) if sc is not None else (None, None)
    call("dtf_pw_conv_bwd_bn", ptr(dout), ptr(y), ptr(ymask), ptr(coef), ptr(x), ptr(wc), ptr(dx), ptr(dw_out), 1,
         *_bn_ptrs(bn), *row_args, ptr(ws), ws.numel(), M, K, C, *sc_ptrs, *sc_args, ptr(wy), stream())
    if bn is not None:
        bn.provide(dx, part, rows.value)
    if sc is not None:
        sc.provide(dout, psc, rsc.value, mask=ymask)
    return dx


def conv_wgrad_raw(x, dy, g, out=None):
    """dW [K,R,S,C] f32; with `out` (an arena gradient view) the result is accumulated into it."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw = g
    dw_ = torch.empty((K, R, S, C), dtype=F32, device=x.device) if out is None else out
    ws = workspace(x.device)
    call("dtf_conv_wgrad", ptr(x), ptr(dy), ptr(dw_), N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw,
         int(out is not None), 0, -1, ptr(ws), ws.numel(), stream())
    return dw_


_STEM_WGRAD = os.environ.get("DTF_STEM_WGRAD", "1") != "0"  # A/B switch: 0 keeps the general wgrad tiles
# 1: the s2d stem's BN + ReLU + MaxPool backward is applied inside the stem wgrad kernel (dtf_stem_wgrad_fused)
_STEM_WGRAD_FUSED = _STEM_WGRAD and os.environ.get("DTF_STEM_WGRAD_FUSED", "1") != "0"


def stem_wgrad_raw(x, dy, g):
    """dW [64, 4, 4, 16] f32 of the space-to-depth stem conv (valid 4x4/1 over the s2d image x [N, Hs, Ws, 16]): the
    persistent stem kernel (csrc/kernels/stemwgrad.hip: the filter gradient resident in the accumulators, one dY row
    image and a ring of s2d rows in LDS, taps as pixel shifts), or the general tiles when it does not take the shape."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw = g
    if (_STEM_WGRAD and on_gpu(x) and (C, K, R, S, sh, sw, ph, pw, dh, dw) == (16, 64, 4, 4, 1, 1, 0, 0, 1, 1)
            and x.is_contiguous() and dy.is_contiguous()):
        dw_ = torch.empty((K, R, S, C), dtype=F32, device=x.device)
        ws = workspace(x.device)
        if K_().dtf_stem_wgrad(ptr(x), ptr(dy), ptr(dw_), N, H, W, 0, ptr(ws), ws.numel(), stream()) == 0:
            return dw_
    return conv_wgrad_raw(x, dy, g)


class _ConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, stride, pad, dil, act):
        x = x.contiguous()
        g = _geom(x, w, stride, pad, dil)
        y = conv_fwd_raw(x, bf16_shadow(w), g, bias=b, act=act)
        ctx.save_for_backward(x, w, y if act else None)
        ctx.g = g
        ctx.act = act
        ctx.has_b = b is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        dy = dy.to(BF16).contiguous()
        if ctx.act == 1:
            dz = torch.empty_like(dy)
            call("dtf_act", ptr(y), ptr(dy), ptr(dz), dz.numel(), 1, 1, stream())  # relu'(y) == relu'(pre)
            dy = dz
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = conv_dgrad_raw(dy, w, ctx.g)
        if ctx.needs_input_grad[1]:
            dw = conv_wgrad_raw(x, dy, ctx.g)
        if ctx.has_b and ctx.needs_input_grad[2]:
            db = torch.empty(dy.shape[-1], dtype=F32, device=dy.device)
            call("dtf_colsum", ptr(dy), dy.numel() // dy.shape[-1], dy.shape[-1], ptr(db), 0, stream())
        return dx, dw, db, None, None, None, None


def _ref_conv(x, w, b, stride, pad, dil):
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).to(w.dtype), w.permute(0, 3, 1, 2), b, stride=stride,
                                   padding=pad, dilation=dil)
    return y.permute(0, 2, 3, 1)


def conv2d(x, w, b=None, stride=(1, 1), pad=(0, 0), dil=(1, 1), act=0):
    """NHWC conv; w is KRSC. Explicit symmetric padding (use same_pads for TF SAME)."""
    stride, pad, dil = tuple(stride), tuple(pad), tuple(dil)
    if on_gpu(x):
        return _ConvFn.apply(x.to(BF16), w, b, stride, pad, dil, act)
    y = _ref_conv(x, w, b, stride, pad, dil)
    return torch.relu(y) if act == 1 else y


class ResidualGradLink:
    """Joins the two gradient contributions of a residual block's input without an extra add pass.

    The block input x feeds the first conv (role "acc") and the shortcut: either directly as the residual of
    the last conv (role "res") or through a projection conv (role "proj"). The shortcut's backward parks its
    gradient of x here instead of returning it, and the first conv's dgrad epilogue adds into that buffer
    (beta = 1) and returns the sum — autograd sees one gradient for x and runs no add kernel. If the first
    conv's backward happens to run before the projection's (autograd schedules by creation order; the block
    creates the projection after the first conv so that it runs first), the link closes and both return their
    gradients normally, so the result is the same either way.

    An identity shortcut may park LAZILY: the last conv's BatchNorm(+ReLU) backward then parks its incoming
    gradient together with the ReLU mask instead of writing the masked residual gradient, and the first conv's
    epilogue applies the mask while adding (one activation-sized write saved per identity block; the parked
    tensor is overwritten in place, it has no other reader).

    A stride-2 1x1 projection may park its data gradient COMPACT ([N, H/2, W/2, C], the only pixels it reaches):
    the first conv's dgrad epilogue then adds it at the even pixels of its own full-size output, so the
    projection's full-size gradient (3/4 zeros) is never cleared, written or read.
    """
    __slots__ = ("buf", "mask", "closed", "compact")

    def __init__(self):
        self.buf = None
        self.mask = None
        self.closed = False
        self.compact = False

    def park(self, g, mask=None, compact=False):
        """Shortcut side: returns what to hand autograd (None when parked)."""
        if self.closed or g is None:
            assert not compact, "a compact gradient can only be parked on an open link"
            return g
        self.buf, self.mask, self.compact = g, mask, compact
        mark_parked(g)
        return None

    def take(self):
        """First-conv side: (parked gradient to accumulate into, its deferred ReLU mask or None, compact flag), or
        (None, None, False); then the link closes."""
        buf, mask, compact = self.buf, self.mask, self.compact
        self.buf = self.mask = None
        self.compact = False
        if buf is None:
            self.closed = True
        else:
            before_overwrite(buf)  # side-stream readers of the parked gradient finish first
        return buf, mask, compact


class _BNSource:
    """What the consumer of a training-mode ConvBN output needs to fuse that BatchNorm's backward reduction
    into its own data-gradient GEMM: the BN input (conv output) yc, the 1-bit ReLU mask and the batch mean.

    Attached to the ConvBN output tensor. A consuming ConvBN whose dgrad produces the COMPLETE gradient of
    that output (its only consumer, or the residual-link "acc" conv that also adds the shortcut's parked
    gradient) lets the GEMM epilogue write sum(dz), sum(dz*(x-mean)) partial rows; the producing ConvBN's
    backward then skips its reduction pass (bn_bwd_reduce), provided the gradient it receives is exactly the
    tensor that dgrad wrote (same storage: autograd added nothing else to it)."""
    __slots__ = ("yc", "mbits", "mean", "invstd", "gamma", "gamma_p", "beta_p", "consumers", "part", "rows", "dx",
                 "ver", "mask", "rx", "rw", "g", "__weakref__")

    def __init__(self, yc, mbits, mean, invstd=None, gamma=None, params=(None, None), recompute=None):
        self.yc, self.mbits, self.mean = yc, mbits, mean
        self.invstd, self.gamma = invstd, gamma
        self.gamma_p, self.beta_p = params
        self.consumers = 0
        self.part = self.rows = self.dx = self.ver = self.mask = None
        # yc not stored: it is bf16(rx rw^T), the producing 1x1 conv's output (input rx, filter parameter rw, geometry
        # g), recomputed by the consumers that can (pwconv.hip RX, pwbwd.hip YR) or materialised on demand
        self.rx, self.rw, self.g = recompute if recompute is not None else (None, None, None)

    def materialize(self):
        """The BN input yc, recomputed once (bitwise the forward's values) if it was not stored."""
        if self.yc is None:
            self.yc = _recompute_y(self.rx, self.rw, self.g)
        return self.yc

    def provide(self, dx, part, rows, mask=None):
        """The producer of this BN's output gradient `dx` records the reduction rows it took of it, and `mask`, the
        ReLU bits still to apply to dx when it hands over a raw (unmasked) gradient."""
        # dx itself is held (not its address), with its version: see nn.same_unmodified
        self.part, self.rows, self.dx, self.ver, self.mask = part, rows, dx, dx._version, mask

    def take(self, dout):
        """For the gradient `dout` this BN's backward received: ((part, rows) or None (then the regular reduction
        runs), the ReLU bits still to apply to dout or None). Rows recorded for another tensor are dropped; a mask
        recorded for another tensor is an error (dout would be taken for an already masked gradient)."""
        from .nn import same_unmodified
        part, rows, dx, ver, mask = self.part, self.rows, self.dx, self.ver, self.mask
        self.part = self.rows = self.dx = self.ver = self.mask = None
        if not same_unmodified(dout, dx, ver):
            if mask is not None:
                raise RuntimeError(
                    "the projection shortcut's gradient was replaced or modified between the block's last conv and "
                    "the projection (a tensor hook that returns a new gradient, or a second consumer of the shortcut "
                    "whose gradient autograd added): the last conv handed over its raw gradient and the ReLU mask")
            return None, None
        return (part, rows) if part is not None and rows >= 1 else None, mask


# Fused BatchNorm backward reduction in the consumer's data-gradient GEMM (see _BNSource), lazy residual gradient
# (parked with its ReLU mask on the link), deferred projection-shortcut BN and the compact stride-2 shortcut
# gradient: module switches for tests (tests/test_resnet_gpu.py flips them to compare against the plain path).
_FUSE_BN_BWD = True
_LAZY_RES = True
_DEFER_PROJ_BN = True
_COMPACT_PROJ = True
# Two-pass forward of the channel-expanding 1x1 ConvBN (statistics pass + recomputed product with the BN apply in its
# epilogue, pwconv.hip dtf_conv_bn_apply_fwd) instead of conv(+stats) -> finalize -> standalone apply pass.
_TWO_PASS_PW = os.environ.get("DTF_PW2", "1") != "0"
# Fused data + weight gradient of the stage-1 channel-reducing 1x1 convs (pwbwd.hip): one read of dY for both,
# the weight gradient on the main stream instead of the side stream. Level 2 also folds the conv output's
# BatchNorm(+ReLU) backward into that pass when its reduction is already done (dY = a dz + b y + c computed per tile,
# never stored: the standalone apply pass disappears; see bwd_route). Levels 3 and 4 (default) stop storing stage-1 c3
# outputs at all: their consumers recompute them per tile, bitwise the forward's values (see _keep_y).
_FUSED_PW_BWD = int(os.environ.get("DTF_PW_BWD", "4"))


def _two_pass_ok(g):
    """Shapes the two-pass pointwise forward handles (pwconv.hip pw_plan): stride-1 unpadded 1x1, C_in 64/128/256,
    K_out = 256 x {1, 2, 4, 8}, tensors < 2 GiB, >= 8 row tiles."""
    N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw, dh, dw = g
    if (R, S, sh, sw, ph, pw) != (1, 1, 1, 1, 0, 0) or C not in (64, 128, 256) or K % 256 or K // 256 not in (1, 2, 4, 8):
        return False
    M = N * P * Q
    return M * K * 2 < (1 << 31) and M * C * 2 < (1 << 31) and M >= 8 * (128 if C == 64 else 64)
# (Measured and removed: "lazy" BatchNorm outputs applied by the consuming conv's operand loaders, r3 —
# profiles/r3_lazy_bn_modes.txt; the BN finalize inside the producing GEMM launch and a BN apply that recomputes the
# expanding 1x1 product, r4 — profiles/r4_negative_results.txt.)


def _keep_y(g, relu, has_res, res_deferred, link_given, role, needs_grad, level=None):
    """Whether the two-pass forward stores the conv output y. Level 3 does not store a stage-1 identity block's c3
    output: its consumers (the layer's BatchNorm-folded backward, the next block's c1 data gradient) recompute it
    from x and w; level 4 neither the projection block's (`res_deferred`: the residual is a deferred projection BN)."""
    level = _FUSED_PW_BWD if level is None else level
    N, H, W, C, K, R, S, P, Q = g[:9]
    return not (level >= 3 and (C, K) == (64, 256) and relu and has_res and N * P * Q >= 64 * 256 and needs_grad
                and ((not res_deferred and link_given and role == "res") or (level >= 4 and res_deferred)))


def _lazy_res(has_res, relu, role, link_open, relu_bits):
    """Identity shortcut with ReLU: dout is parked on the link with the ReLU mask, no masked gradient is written."""
    return bool(has_res and relu and role == "res" and link_open and _LAZY_RES and relu_bits)


def _bn_complete(consumers, role, acc_taken=False):
    """Whether a conv's dX is the COMPLETE gradient of its input BatchNorm's output (see _BNSource): it is the only
    consumer, or the "acc" conv that took the second consumer's parked gradient to add into. Never a projection,
    whose dX is joined with the first conv's. (Only the general route takes an acc; fold_identity has role "res".)"""
    return role != "proj" and (consumers == 1 or (role == "acc" and acc_taken and consumers == 2))


def bwd_route(g, role, relu, has_res, training, *, link_open, relu_bits, rows_taken, shortcut_src, yc_stored,
              mask_given, need_dx, need_dw, direct_w, x_bf16, level=None):
    """The route _ConvBNFn.backward takes, from facts alone (no tensors, no launches; level: _FUSED_PW_BWD unless
    given). rows_taken: the consumer's BN-backward partial rows were taken for this gradient; shortcut_src: a deferred
    projection-shortcut BN rides on this layer; mask_given: the gradient came with ReLU bits still to apply; direct_w:
    a direct weight-gradient view exists; x_bf16: x is contiguous bf16.

    fold_* (level >= 2, the BN reduction already taken): only the BN-backward coefficients are finalized, then ONE
    pass forms dY per tile and computes dX and dW from it (dtf_pw_conv_bwd_bn) — an identity block's c3, the stage-1
    projection block's c3 (taking the shortcut BN's reduction too), that block's stride-1 projection. Otherwise the
    standalone BN backward runs, then pw_fused (level >= 1: dX, dW in one pass over dY, dtf_pw_conv_bwd) or general."""
    level = _FUSED_PW_BWD if level is None else level
    if not training:
        return "frozen"
    stage1 = (g[4], g[3]) == (256, 64)
    if level >= 2 and rows_taken and need_dx and need_dw and x_bf16 and direct_w and pw_bwd_bn_ok(g):
        if _lazy_res(has_res, relu, role, link_open, relu_bits) and not shortcut_src and (yc_stored or stage1):
            return "fold_identity"
        if shortcut_src and relu and stage1:
            return "fold_proj_block"
        if yc_stored and mask_given and role == "proj" and not shortcut_src and stage1:
            return "fold_shortcut"
    if level >= 1 and need_dw and direct_w and need_dx and role != "acc" and pw_bwd_ok(g) and x_bf16:
        return "pw_fused"
    return "general"


def _bn_grad_targets(bn_params, K, device):
    """(dgamma, dbeta, direct) for a backward to write: the parameters' arena gradient views when both exist (then
    accumulated in place, direct), else fresh [K] buffers."""
    tg, tb = (direct_grad(p) for p in bn_params)
    if tg is not None and tb is not None:
        return tg, tb, True
    return torch.empty(K, dtype=F32, device=device), torch.empty(K, dtype=F32, device=device), False


def _grads(dx, dw, dgamma, dbeta, dres=None, direct_bn=False):
    """What _ConvBNFn / _ConvBNPoolFn.backward return: a slot per forward argument, (x, w, gamma, beta[, residual])
    first, no gradient for the rest; dgamma / dbeta accumulated in place (direct_bn) are not handed to autograd."""
    if direct_bn:
        dgamma = dbeta = None
    return (dx, dw, dgamma, dbeta, dres) + (None,) * (_FWD_ARGS - 5)


class _ConvBNFn(torch.autograd.Function):
    """y = [relu]( BN_train(conv(x, w)) [+ residual] ) with batch statistics from the conv epilogue."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, res, rmean, rvar, stride, pad, dil, relu, momentum, eps, training,
                link=None, role=None):
        in_src = getattr(x, "_dtf_bnsrc", None)
        if in_src is not None:
            in_src.consumers += 1
        if res is not None and getattr(res, "_dtf_bnsrc", None) is not None:
            res._dtf_bnsrc.consumers += 1
        x = x.contiguous()
        g = _geom(x, w, stride, pad, dil)
        N, H, W, C, K, R, S, P, Q = g[:9]
        M = N * P * Q
        dev = x.device
        work = torch.empty(4 * K, dtype=F32, device=dev)  # scale shift mean invstd
        scale, shift, mean, invstd = work[:K], work[K:2 * K], work[2 * K:3 * K], work[3 * K:]
        raff = getattr(res, "_dtf_affine", None) if res is not None else None
        raff_ptrs = (ptr(raff[0]), ptr(raff[1])) if raff else (None, None)
        # the deferred projection BN (its input + mean): its backward reduction is taken in our apply pass
        res_src = getattr(res, "_dtf_bnsrc", None) if raff is not None else None
        res = contig(res)
        deferred = role == "proj" and not relu and _DEFER_PROJ_BN
        mbits = torch.empty(M * K // 8, dtype=torch.uint8, device=dev) if relu else None
        if training and not deferred and _TWO_PASS_PW and _two_pass_ok(g):
            # (bottleneck c3; BatchNorm / residual / ReLU applied in the epilogue: pwconv.hip MODE 1 / 2)
            keep_y = _keep_y(g, relu, res is not None, raff is not None, link is not None, role,
                             any(ctx.needs_input_grad))
            yc = torch.empty((N, P, Q, K), dtype=BF16, device=dev) if keep_y else None
            out = torch.empty((N, P, Q, K), dtype=BF16, device=dev)
            part = torch.empty(((M + 63) // 64) * 2 * K, dtype=F32, device=dev)
            call("dtf_conv_bn_apply_fwd", ptr(x), ptr(bf16_shadow(w)), ptr(yc), ptr(out), ptr(mbits), ptr(res),
                 *raff_ptrs, M, C, K, int(relu), ptr(part), ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar),
                 float(momentum), float(eps), ptr(scale), ptr(shift), ptr(mean), ptr(invstd), stream())
        else:
            if training:
                yc = conv_fwd_bn_raw(x, bf16_shadow(w), g, gamma, beta, rmean, rvar, momentum, eps, scale, shift,
                                     mean, invstd)
            else:
                yc = conv_fwd_raw(x, bf16_shadow(w), g)
                call("dtf_bn_infer_coeff", ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), K, float(eps), ptr(scale),
                     ptr(shift), stream())
                if any(ctx.needs_input_grad):  # frozen BN: the backward normalises with the running statistics
                    mean.copy_(rmean)
                    torch.rsqrt(rvar + eps, out=invstd)
            if deferred:
                # projection shortcut: its BN output is consumed only as the residual of the block's last ConvBN,
                # whose apply pass normalises the conv output on the fly (res * scale + shift) — hand autograd the
                # conv output tagged with the affine instead of materialising the BN output
                out = yc
                out._dtf_affine = (scale, shift)
            else:
                out = torch.empty_like(yc)
                call("dtf_bn_apply", ptr(yc), ptr(scale), ptr(shift), ptr(res), ptr(out), M, K, int(relu),
                     ptr(mbits), *raff_ptrs, stream())
        # backward needs the conv output and a 1-bit ReLU mask, not the bf16 BN output
        ctx.save_for_backward(x, w, gamma, yc, mbits, mean, invstd)
        ctx.bn_params = (gamma, beta)
        ctx.g = g
        ctx.relu = relu
        ctx.has_res = res is not None
        ctx.training = training
        ctx.link, ctx.role = link, role
        ctx.in_src = in_src if (ctx.needs_input_grad[0] and _FUSE_BN_BWD) else None
        ctx.res_src = res_src if (training and _FUSE_BN_BWD) else None
        ctx.src = None
        if training and _FUSE_BN_BWD and any(ctx.needs_input_grad):
            ctx.src = out._dtf_bnsrc = _BNSource(yc, mbits, mean, invstd, gamma, (gamma, beta),
                                                 recompute=(x, w, g) if yc is None else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w, gamma, yc, mbits, mean, invstd = ctx.saved_tensors
        g = ctx.g
        N, H, W, C, K, R, S, P, Q, sh, sw, ph, pw = g[:13]
        M = N * P * Q
        yshape, dev = (N, P, Q, K), x.device
        dout = dout.to(BF16).contiguous()
        taken, dmask = ctx.src.take(dout) if ctx.src is not None else (None, None)
        if dmask is not None:
            # a deferred projection BN whose consumer folded (fold_proj_block): dout is raw, dz = dout under its mask
            assert mbits is None and not ctx.relu
            mbits = dmask
        link, role = ctx.link, ctx.role
        need_dx, need_dw = ctx.needs_input_grad[:2]
        link_open = link is not None and not link.closed
        lazy_res = _lazy_res(ctx.has_res, ctx.relu, role, link_open, mbits is not None)
        want_dres = ctx.has_res and ctx.relu and not lazy_res  # (the masked residual gradient is written out)
        rsrc = ctx.res_src if want_dres else None  # projection shortcut BN: its backward reduction rides on ours
        tw = direct_grad(w) if need_dw else None
        src = ctx.in_src

        def complete_src(acc_taken=False):  # the input BN's source if our dX may take its backward reduction
            return src if src is not None and _bn_complete(src.consumers, role, acc_taken) else None
        route = bwd_route(g, role, ctx.relu, ctx.has_res, ctx.training, link_open=link_open,
                          relu_bits=mbits is not None, rows_taken=taken is not None, shortcut_src=rsrc is not None,
                          yc_stored=yc is not None, mask_given=dmask is not None, need_dx=need_dx, need_dw=need_dw,
                          direct_w=tw is not None, x_bf16=x.is_contiguous() and x.dtype == BF16)
        if route == "frozen":
            return _ConvBNFn._backward_frozen(ctx, dout, x, w, gamma, yc, mbits, mean, invstd)
        dgamma, dbeta, direct_bn = _bn_grad_targets(ctx.bn_params, K, dev)
        if route.startswith("fold_"):
            # dY is formed per tile from dout, the ReLU bits and yc (recomputed from x when not stored), never stored
            coef = torch.empty(3 * K, dtype=F32, device=dev)
            call("dtf_bn_bwd_coef", ptr(taken[0]), taken[1], ptr(mean), ptr(invstd), ptr(gamma), M, K, ptr(dgamma),
                 ptr(dbeta), int(direct_bn), ptr(coef), stream())
            dx = conv_bwd_bn_fused_raw(dout, yc, mbits, coef, x, w, g, tw, bn=complete_src(), sc=rsrc,
                                       wy=bf16_shadow(w) if yc is None else None)
            ctx.in_src = ctx.src = ctx.res_src = None
            if route == "fold_identity":
                # the identity shortcut's gradient: dout parked with the ReLU mask (read above, in stream order, before
                # the first conv's dgrad overwrites it)
                link.park(dout, mask=mbits)
            elif route == "fold_shortcut" and link is not None:
                dx = link.park(dx)
            # fold_proj_block: the shortcut receives the raw dout; its ReLU bits went to rsrc with the reduction rows
            return _grads(dx, None, dgamma, dbeta, dout if route == "fold_proj_block" else None, direct_bn)
        if yc is None:  # (not stored by the forward and not recomputed inside a fused pass above)
            yc = _recompute_y(x, w, g)
        dyc = torch.empty(yshape, dtype=BF16, device=dev)
        dres = torch.empty(yshape, dtype=BF16, device=dev) if want_dres else None
        part2, rows2, sc_rows = _partial_rows(rsrc is not None, 2048, K, dev)
        sc = ((ptr(rsrc.yc), ptr(rsrc.mean)) if rsrc is not None else (None, None)) + sc_rows
        args = (ptr(mbits), ptr(yc), ptr(mean), ptr(invstd), ptr(gamma), M, K, ptr(dyc), ptr(dres), ptr(dgamma),
                ptr(dbeta), int(direct_bn))
        if taken is not None:  # the consumer's dgrad epilogue already reduced this gradient
            coef = torch.empty(3 * K, dtype=F32, device=dev)
            call("dtf_bn_bwd_partials", ptr(dout), *args, ptr(taken[0]), taken[1], ptr(coef), *sc, stream())
        else:
            work = torch.empty((2 * 1024 + 3) * K, dtype=F32, device=dev)
            call("dtf_bn_bwd", ptr(dout), None, *args, ptr(work), *sc, stream())
        if rsrc is not None and rows2.value > 0:
            rsrc.provide(dres, part2, rows2.value)
        ctx.res_src = ctx.src = None
        if ctx.has_res and not ctx.relu:
            dres = dout
        if lazy_res:
            dres = link.park(dout, mask=mbits)  # (None: parked; dout is overwritten by the first conv's dgrad)
        elif link is not None and role == "res":
            dres = link.park(dres)
        if route == "pw_fused":
            dx = conv_bwd_fused_raw(dyc, x, w, g, tw, bn=complete_src())
            if link is not None and role == "proj":
                dx = link.park(dx)
            ctx.in_src = None
            return _grads(dx, None, dgamma, dbeta, dres, direct_bn)
        dx = dw = None
        if need_dw:
            if tw is not None and SIDE_STREAM_ON:
                with fork_side(x.device, x, dyc):  # off the critical path: overlaps the dgrad chain
                    conv_wgrad_raw(x, dyc, g, out=tw)
            else:
                dw = conv_wgrad_raw(x, dyc, g, out=tw)
            if tw is not None:
                dw = None  # (autograd still runs the parameter's AccumulateGrad node with an undefined
                #            gradient, so its post-accumulate hooks — gradient bucketing — fire as usual)
        if need_dx:
            acc, acc_mask, compact = link.take() if (link is not None and role == "acc") else (None, None, False)
            bn = complete_src(acc_taken=acc is not None)
            if (role == "proj" and link_open and _COMPACT_PROJ
                    and (R, S, sh, sw, ph, pw) == (1, 1, 2, 2, 0, 0) and H == 2 * P and W == 2 * Q):
                # stride-2 1x1 shortcut: its gradient only reaches the even pixels — a plain GEMM over dY rows
                gc = (N, P, Q, C, K, 1, 1, P, Q, 1, 1, 0, 0, 1, 1)
                dx = link.park(conv_dgrad_raw(dyc, w, gc), compact=True)
            elif compact:
                dx = conv_dgrad_raw(dyc, w, g, bn=bn, acc_sub2=acc)
            else:
                dx = conv_dgrad_raw(dyc, w, g, acc=acc, bn=bn, acc_mask=acc_mask)
                if link is not None and role == "proj":
                    dx = link.park(dx)
            ctx.in_src = None
        return _grads(dx, dw, dgamma, dbeta, dres, direct_bn)

    @staticmethod
    def _backward_frozen(ctx, dout, x, w, gamma, yc, mbits, mean, invstd):
        """Backward of an inference-mode (frozen) BatchNorm — Keras' BatchNormalization(training=False) under a
        GradientTape, e.g. fine-tuning with frozen statistics: the BN is the fixed affine gamma*invstd*(z - mean) +
        beta of the running statistics, so dz = dy * relu' * gamma*invstd, dgamma = sum(dy relu' xhat),
        dbeta = sum(dy relu'). Rare path: torch ops on the GPU, f32 math."""
        K = yc.shape[-1]
        dz = dout.float()
        if mbits is not None:
            bits = (mbits.view(-1, 1) >> torch.arange(8, device=mbits.device, dtype=torch.uint8)) & 1
            dz = dz * bits.view(dz.shape).to(dz.dtype)
        dzr = dz.reshape(-1, K)
        xhat = (yc.float().reshape(-1, K) - mean) * invstd
        dgamma, dbeta = (dzr * xhat).sum(0), dzr.sum(0)
        gm = gamma if gamma is not None else torch.ones_like(invstd)
        dyc = (dz * (gm * invstd)).to(BF16).contiguous()
        dres = None
        if ctx.has_res:
            dres = dz.to(BF16) if ctx.relu else dout
        dx = dw = None
        if ctx.needs_input_grad[1]:
            dw = conv_wgrad_raw(x, dyc, ctx.g)
        if ctx.needs_input_grad[0]:
            dx = conv_dgrad_raw(dyc, w, ctx.g)
        ctx.in_src = ctx.src = ctx.res_src = None
        return _grads(dx, dw, dgamma if ctx.needs_input_grad[2] else None,
                      dbeta if ctx.needs_input_grad[3] else None, dres=dres)


def conv_bn(x, w, gamma, beta, rmean, rvar, stride=(1, 1), pad=(0, 0), dil=(1, 1), relu=True, residual=None,
            momentum=0.9, eps=1e-5, training=True, link=None, role=None):
    """Fused Conv2D -> FusedBatchNorm -> (+residual) -> ReLU, NHWC. `link`/`role`: see ResidualGradLink."""
    stride, pad, dil = tuple(stride), tuple(pad), tuple(dil)
    if on_gpu(x):
        return _ConvBNFn.apply(x.to(BF16), w, gamma, beta, residual, rmean, rvar, stride, pad, dil, bool(relu),
                               float(momentum), float(eps), bool(training), link, role)
    y = _ref_conv(x, w, None, stride, pad, dil)
    from .norm import batch_norm_ref
    y = batch_norm_ref(y, gamma, beta, rmean, rvar, momentum, eps, training)
    if residual is not None:
        y = y + residual.to(y.dtype)
    return torch.relu(y) if relu else y


class _ConvBNPoolFn(torch.autograd.Function):
    """y = MaxPool( relu( BN_train(conv(x, w)) ) ) — the ResNet stem as one autograd node.

    The BN+ReLU output is never materialised: one pass over the conv output produces the pooled output and an
    argmax byte per pooled element whose bit 7 is the ReLU mask (norm.hip bn_relu_maxpool_fwd_kernel). The
    backward gathers the pooled gradient per conv-output pixel on the fly in the BN backward's reduce and
    apply passes, instead of writing the pool gradient and re-reading it twice."""

    @staticmethod
    def forward(ctx, x, w, gamma, beta, rmean, rvar, stride, pad, dil, momentum, eps, training, pk, ps, pp,
                s2d=False):
        x = x.contiguous()
        w16 = bf16_shadow(w)
        if s2d:  # x: image_to_s2d_bf16 output; w: the 7x7 filter, run as its 4x4 space-to-depth form
            w16 = stem_s2d_filter(w16)
            g = _geom(x, w16, (1, 1), (0, 0), (1, 1))
        else:
            g = _geom(x, w, stride, pad, dil)
        N, H, W, C, K, R, S, P, Q = g[:9]
        M = N * P * Q
        dev = x.device
        work = torch.empty(4 * K, dtype=F32, device=dev)  # scale shift mean invstd
        scale, shift, mean, invstd = work[:K], work[K:2 * K], work[2 * K:3 * K], work[3 * K:]
        if training:
            yc = conv_fwd_bn_raw(x, w16, g, gamma, beta, rmean, rvar, momentum, eps, scale, shift, mean, invstd)
        else:
            yc = conv_fwd_raw(x, w16, g)
            call("dtf_bn_infer_coeff", ptr(gamma), ptr(beta), ptr(rmean), ptr(rvar), K, float(eps), ptr(scale),
                 ptr(shift), stream())
        P2, Q2 = out_size(P, pk[0], ps[0], pp[0]), out_size(Q, pk[1], ps[1], pp[1])
        y = torch.empty((N, P2, Q2, K), dtype=BF16, device=dev)
        arg = torch.empty((N, P2, Q2, K), dtype=torch.uint8, device=dev)
        call("dtf_bn_relu_maxpool_fwd", ptr(yc), ptr(scale), ptr(shift), ptr(y), ptr(arg), N, P, Q, K, P2, Q2,
             pk[0], pk[1], ps[0], ps[1], pp[0], pp[1], stream())
        ctx.save_for_backward(x, w, gamma, yc, arg, mean, invstd)
        ctx.bn_params = (gamma, beta)
        ctx.g = g
        ctx.pool = (P2, Q2, pk, ps, pp)
        ctx.s2d = s2d
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, gamma, yc, arg, mean, invstd = ctx.saved_tensors
        g = ctx.g
        N, H, W, C, K, R, S, P, Q = g[:9]
        P2, Q2, pk, ps, pp = ctx.pool
        dy = dy.to(BF16).contiguous()
        dgamma, dbeta, direct_bn = _bn_grad_targets(ctx.bn_params, K, yc.device)
        work = torch.empty((2 * 1024 + 3) * K, dtype=F32, device=yc.device)
        # s2d stem, filter gradient only: the BN + ReLU + pool backward is applied inside the stem wgrad kernel
        # (dtf_stem_wgrad_fused) from the coefficients the reduce pass leaves in work[:3K]; dyc is never formed
        fused = (ctx.s2d and _STEM_WGRAD_FUSED and ctx.needs_input_grad[1] and (K, pk, ps, pp) == (
            64, (3, 3), (2, 2), (1, 1)) and P == 2 * P2 and Q == 2 * Q2 and W <= 128 and C == 16 and R == 4)
        dyc = None if fused else torch.empty_like(yc)
        call("dtf_maxpool_bn_bwd", ptr(dy), ptr(arg), ptr(yc), ptr(mean), ptr(invstd), ptr(gamma), N, P, Q, K, P2,
             Q2, pk[0], pk[1], ps[0], ps[1], pp[0], pp[1], None if fused else ptr(dyc), ptr(dgamma),
             ptr(dbeta), int(direct_bn), ptr(work), stream())
        dx = dw = None
        if fused:
            dw2 = torch.empty((K, R, S, C), dtype=F32, device=x.device)
            ws = workspace(x.device)
            call("dtf_stem_wgrad_fused", ptr(x), ptr(yc), ptr(dy), ptr(arg), ptr(work), ptr(dw2), N, H, W, 0, ptr(ws),
                 ws.numel(), stream())
            dw = stem_s2d_filter_grad(dw2, w.shape)
            tw = direct_grad(w)
            if tw is not None:
                tw.add_(dw)
                dw = None
            return _grads(None, dw, dgamma, dbeta, direct_bn=direct_bn)
        if ctx.needs_input_grad[0]:
            if ctx.s2d:
                raise NotImplementedError("no input gradient through the space-to-depth stem (image input)")
            dx = conv_dgrad_raw(dyc, w, g)
        if ctx.needs_input_grad[1]:
            tw = direct_grad(w)
            if ctx.s2d:
                dw = stem_s2d_filter_grad(stem_wgrad_raw(x, dyc, g), w.shape)
                if tw is not None:
                    tw.add_(dw)
            else:
                dw = conv_wgrad_raw(x, dyc, g, out=tw)
            if tw is not None:
                dw = None
        return _grads(dx, dw, dgamma, dbeta, direct_bn=direct_bn)


_FWD_ARGS = _ConvBNFn.forward.__code__.co_argcount - 1  # (without ctx)
assert _ConvBNPoolFn.forward.__code__.co_argcount - 1 == _FWD_ARGS


_S2D_IDX = {}


def _s2d_index(Cp, device):
    """Column maps between a 7x7 stem filter [K, 7, 7, Cp] (flattened per output channel, plus one trailing
    zero column) and its space-to-depth form [K, 4, 4, 16]: s2d tap (a, b), channel (dh*2 + dw)*4 + c holds
    filter tap (2a + dh - 1, 2b + dw - 1), channel c (zero outside the 7x7 window or for c >= Cp)."""
    key = (Cp, str(device))
    if key not in _S2D_IDX:
        zero = 49 * Cp
        fwd = torch.full((4 * 4 * 16,), zero, dtype=torch.long)
        back = torch.full((49 * Cp,), 4 * 4 * 16, dtype=torch.long)
        for a in range(4):
            for b in range(4):
                for k in range(16):
                    dh, dw, c = k >> 3, (k >> 2) & 1, k & 3
                    kh, kw = 2 * a + dh - 1, 2 * b + dw - 1
                    if 0 <= kh < 7 and 0 <= kw < 7 and c < Cp:
                        fwd[(a * 4 + b) * 16 + k] = (kh * 7 + kw) * Cp + c
                        back[(kh * 7 + kw) * Cp + c] = (a * 4 + b) * 16 + k
        _S2D_IDX[key] = (fwd.to(device), back.to(device))
    return _S2D_IDX[key]


def _gather_cols(m, idx, ncols):
    """out[:, j] = m[:, idx[j]] of a row-major 2-D matrix, 0 where idx[j] == m.shape[1] (sort.hip dtf_gather_cols on
    the GPU: one launch, no zero-column concatenation)."""
    rows, cols = m.shape
    if on_gpu(m) and m.element_size() in (2, 4):
        m = m.contiguous()
        out = torch.empty((rows, ncols), dtype=m.dtype, device=m.device)
        call("dtf_gather_cols", ptr(m), m.element_size(), rows, cols, ptr(idx), ncols, ptr(out), stream())
        return out
    return torch.cat([m, m.new_zeros(rows, 1)], 1).index_select(1, idx)


class _S2DFilterFn(torch.autograd.Function):
    """stem_s2d_filter as an autograd node (the native column gather has no autograd of its own): the backward is the
    inverse gather stem_s2d_filter_grad. Used where the s2d filter feeds an autograd conv (the frozen-BN stem path)."""

    @staticmethod
    def forward(ctx, w):
        ctx.shape = tuple(w.shape)
        return _s2d_filter_raw(w)

    @staticmethod
    def backward(ctx, g):
        return stem_s2d_filter_grad(g.contiguous(), ctx.shape)


def _s2d_filter_raw(w):
    K, R, S, Cp = w.shape
    assert (R, S) == (7, 7)
    fwd, _ = _s2d_index(Cp, w.device)
    return _gather_cols(w.reshape(K, -1), fwd, fwd.numel()).reshape(K, 4, 4, 16)


def stem_s2d_filter(w):
    """[K, 7, 7, Cp] -> [K, 4, 4, 16]: the 7x7/2 pad-3 filter as a 4x4/1 filter over image_to_s2d_bf16 output
    (differentiable: gradients flow back to the 7x7 filter)."""
    if torch.is_grad_enabled() and w.requires_grad:
        return _S2DFilterFn.apply(w)
    return _s2d_filter_raw(w)


def stem_s2d_filter_grad(dw2, shape):
    """Gradient of stem_s2d_filter: [K, 4, 4, 16] -> [K, 7, 7, Cp] (every filter entry appears once; the padded
    colour channels c >= 4 get zero)."""
    K, R, S, Cp = shape
    _, back = _s2d_index(Cp, dw2.device)
    return _gather_cols(dw2.reshape(K, -1), back, back.numel()).reshape(K, R, S, Cp)


def image_to_s2d_bf16(x_nchw):
    """f32 NCHW images (<= 4 channels, even H, W) -> bf16 2x2 space-to-depth [N, H/2+3, W/2+3, 16] (zero padding
    baked in) for the space-to-depth stem (conv_bn_maxpool(..., s2d=True))."""
    N, C, H, W = x_nchw.shape
    if on_gpu(x_nchw):
        y = torch.empty((N, H // 2 + 3, W // 2 + 3, 16), dtype=BF16, device=x_nchw.device)
        call("dtf_nchw_to_s2d", ptr(x_nchw.float().contiguous()), ptr(y), N, C, H, W, stream())
        return y
    xp = torch.zeros((N, 4, H + 6, W + 6), dtype=x_nchw.dtype)
    xp[:, :C, 4:H + 4, 4:W + 4] = x_nchw
    # [N, 4, Hs, 2, Ws, 2] -> [N, Hs, Ws, dh, dw, c]
    t = xp.reshape(N, 4, (H + 6) // 2, 2, (W + 6) // 2, 2).permute(0, 2, 4, 3, 5, 1)
    return t.reshape(N, (H + 6) // 2, (W + 6) // 2, 16)


def conv_bn_maxpool(x, w, gamma, beta, rmean, rvar, stride=(1, 1), pad=(0, 0), dil=(1, 1), momentum=0.9, eps=1e-5,
                    training=True, pool_size=(3, 3), pool_strides=(2, 2), pool_pad=(1, 1), s2d=False):
    """MaxPool(ReLU(FusedBatchNorm(Conv2D(x)))), NHWC — the ResNet stem fused (see _ConvBNPoolFn).
    s2d=True: x is image_to_s2d_bf16(images) and w the [K, 7, 7, Cp] filter of a 7x7/2 pad-3 conv (run as the
    equivalent 4x4/1 conv over the space-to-depth image: 256 instead of 392 MACs per output, no padded taps)."""
    stride, pad, dil = tuple(stride), tuple(pad), tuple(dil)
    pk, ps, pp = tuple(pool_size), tuple(pool_strides), tuple(pool_pad)
    if s2d:
        assert tuple(w.shape[1:3]) == (7, 7) and stride == (2, 2) and pad == (3, 3) and dil == (1, 1)
    frozen_grad = not training and torch.is_grad_enabled() and any(
        getattr(t, "requires_grad", False) for t in (x, w, gamma, beta))
    if on_gpu(x) and w.shape[0] % 8 == 0 and pk[0] * pk[1] <= 127 and not frozen_grad:
        # (inference-mode BN under a tape takes the unfused pair below: conv_bn's frozen-BN backward + max_pool2d)
        return _ConvBNPoolFn.apply(x.to(BF16), w, gamma, beta, rmean, rvar, stride, pad, dil, float(momentum),
                                   float(eps), bool(training), pk, ps, pp, bool(s2d))
    if s2d:
        w = stem_s2d_filter(w)
        stride, pad = (1, 1), (0, 0)
    from .nn import max_pool2d
    y = conv_bn(x, w, gamma, beta, rmean, rvar, stride, pad, dil, relu=True, momentum=momentum, eps=eps,
                training=training)
    return max_pool2d(y, pk, ps, pp)


def image_to_nhwc_bf16(x_nchw, cpad=8):
    """Device-side input pipeline step: f32 NCHW images -> bf16 NHWC, channels padded to `cpad`."""
    N, C, H, W = x_nchw.shape
    if on_gpu(x_nchw):
        y = torch.empty((N, H, W, cpad), dtype=BF16, device=x_nchw.device)
        call("dtf_nchw_to_nhwc_pad", ptr(x_nchw.contiguous()), ptr(y), N, C, H * W, cpad, stream())
        return y
    y = torch.zeros((N, H, W, cpad), dtype=x_nchw.dtype)
    y[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return y
