"""The references of test_norm_edges_gpu.py and test_pool_edges_gpu.py (tests/_rowcmp.py: maxpool_first,
maxpool_scatter, bn_f64) pinned against PyTorch on the CPU, so a wrong reference cannot hide a wrong kernel; and the
CPU fallbacks of ops.batch_norm / ops.layer_norm / ops.max_pool2d (channel counts that are no multiple of 8) and
ops.norm.batch_norm_ref against float64.

Bounds: the float64 references agree with float64 PyTorch to 1e-12 per channel (summation order only); the f32
fallbacks to 1e-5 per channel (f32 epsilon 6e-8 times the ~100-term reductions, with margin).
"""
import pytest
import torch
import torch.nn.functional as F

from distributed_tensorflow_amd import ops
from distributed_tensorflow_amd.ops.norm import batch_norm_ref

from _rowcmp import POOL_GEOS, _pair, bn_f64, check_chans, check_rows, check_sums, maxpool_first, maxpool_scatter

F64 = torch.float64


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("geo", POOL_GEOS, ids=str)
@pytest.mark.parametrize("kind", ["randn", "negative", "ties"])
def test_maxpool_first_values_match_torch(geo, kind):
    H, W, k, s, p = geo
    g = torch.Generator().manual_seed(H * 100 + W)
    x = torch.randn(2, H, W, 5, generator=g, dtype=F64)
    if kind == "negative":
        x = -3.0 - x.abs()
    elif kind == "ties":
        x = torch.randint(-2, 3, x.shape, generator=g).double()
    v, idx = maxpool_first(x, k, s, p)
    ref = _nhwc(F.max_pool2d(_nchw(x), _pair(k), _pair(s), _pair(p)))
    assert torch.equal(v, ref)
    R, S = _pair(k)
    assert idx.min() >= 0 and idx.max() < R * S
    # the tap named by idx holds the maximum, and no earlier tap does (first-maximal rule), checked by gathering
    sh, sw = _pair(s)
    ph, pw = _pair(p)
    xp = F.pad(_nchw(x), (pw, pw, ph, ph), value=float("-inf"))
    N, P, Q, C = v.shape
    for r in range(R):
        for c in range(S):
            tap = _nhwc(xp[:, :, r:r + (P - 1) * sh + 1:sh, c:c + (Q - 1) * sw + 1:sw])
            assert (tap[idx == r * S + c] == v[idx == r * S + c]).all()
            assert (tap[idx > r * S + c] < v[idx > r * S + c]).all(), "an earlier tap already held the maximum"


@pytest.mark.parametrize("geo", POOL_GEOS, ids=str)
def test_maxpool_scatter_matches_autograd_without_ties(geo):
    H, W, k, s, p = geo
    g = torch.Generator().manual_seed(H * 100 + W + 1)
    N, C = 2, 5
    x = torch.randperm(N * H * W * C, generator=g).double().reshape(N, H, W, C) - 100.0   # all values distinct
    xr = x.clone().requires_grad_(True)
    y = _nhwc(F.max_pool2d(_nchw(xr), _pair(k), _pair(s), _pair(p)))
    dy = torch.randn(y.shape, generator=g, dtype=F64)
    (dref,) = torch.autograd.grad(y, xr, dy)
    v, idx = maxpool_first(x, k, s, p)
    dx = maxpool_scatter(dy, idx, H, W, k, s, p)
    assert torch.equal(v, y.detach())
    assert (dx - dref).abs().max().item() <= 1e-12 * dref.abs().max().item()


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("with_res", [False, True])
def test_bn_f64_matches_torch(relu, with_res):
    g = torch.Generator().manual_seed(11 + 2 * relu + with_res)
    N, H, W, C = 3, 5, 4, 6
    x = (torch.randn(N, H, W, C, generator=g, dtype=F64) * torch.tensor([0.1, 1, 5, 20, 1, 1]) +
         torch.tensor([0.0, 3, -40, 100, 0, -2])).requires_grad_(True)
    gamma = (torch.rand(C, generator=g, dtype=F64) + 0.5).requires_grad_(True)
    beta = torch.randn(C, generator=g, dtype=F64).requires_grad_(True)
    res = torch.randn(N, H, W, C, generator=g, dtype=F64).requires_grad_(True) if with_res else None
    dy = torch.randn(N, H, W, C, generator=g, dtype=F64)
    eps = 1e-3
    y = F.batch_norm(x.reshape(-1, C), None, None, gamma, beta, True, 0.1, eps).reshape(x.shape)
    if with_res:
        y = y + res
    if relu:
        y = torch.relu(y)
    grads = torch.autograd.grad(y, [x, gamma, beta] + ([res] if with_res else []), dy)
    r = bn_f64(x, gamma, beta, eps, res=res, relu=relu, dy=dy)
    check_chans("y", r.y, y.detach(), 1e-12)
    check_chans("dx", r.dx, grads[0], 1e-12)
    check_sums("dgamma", r.dgamma, grads[1], r.dgamma_scale, 1e-12)
    check_sums("dbeta", r.dbeta, grads[2], r.dbeta_scale, 1e-12)
    if with_res:
        check_chans("dres", r.dres, grads[3], 1e-12)
    else:
        assert r.dres is None
    x2 = x.detach().reshape(-1, C)
    assert torch.allclose(r.mean, x2.mean(0), rtol=1e-13, atol=0)
    assert torch.allclose(r.var, x2.var(0, unbiased=False), rtol=1e-12, atol=0)


def _bn_inputs(C, shape=(2, 7, 7)):
    g = torch.Generator().manual_seed(C)
    c = torch.arange(C)
    std = 2.0 ** ((c % 5) - 2).double()
    x = (torch.randn(*shape, C, generator=g, dtype=F64) + ((c % 3) - 1).double() * 2) * std
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return x.float(), gamma, beta, rm, rv


@pytest.mark.parametrize("shape", [(2, 7, 7), (1, 1, 1)], ids=["M98", "M1"])
def test_batch_norm_ref_and_cpu_fallback_match_f64(shape):
    """C = 20 is no multiple of 8: ops.batch_norm takes its PyTorch fallback (batch_norm_ref). M = 1: the unbiased
    factor is n / max(n - 1, 1) = 1."""
    C, eps, mom = 20, 1e-3, 0.9
    x, gamma, beta, rm0, rv0 = _bn_inputs(C, shape)
    res = torch.randn(*shape, C, generator=torch.Generator().manual_seed(3))
    n = x.numel() // C
    r = bn_f64(x, gamma, beta, eps)
    rm_ref = rm0.double() * mom + r.mean * (1 - mom)
    rv_ref = rv0.double() * mom + r.var * (n / max(n - 1, 1)) * (1 - mom)
    for fn in ("ref", "op"):
        rm, rv = rm0.clone(), rv0.clone()
        if fn == "ref":
            y = batch_norm_ref(x, gamma, beta, rm, rv, mom, eps, True)
            yref = r.y
        else:
            y = ops.batch_norm(x, gamma, beta, rm, rv, training=True, momentum=mom, eps=eps, relu=True, residual=res)
            yref = bn_f64(x, gamma, beta, eps, res=res, relu=True).y
        check_chans(f"{fn} y", y, yref, 1e-5)
        assert torch.allclose(rm.double(), rm_ref, rtol=1e-5, atol=1e-6)
        assert torch.allclose(rv.double(), rv_ref, rtol=1e-5, atol=1e-6)
    # inference: the running statistics are used and left alone
    rm, rv = rm0.clone(), rv0.clone()
    y = ops.batch_norm(x, gamma, beta, rm, rv, training=False, eps=eps)
    yref = (x.double() - rm0.double()) * torch.rsqrt(rv0.double() + eps) * gamma.double() + beta.double()
    check_chans("inference y", y, yref, 1e-5)
    assert torch.equal(rm, rm0) and torch.equal(rv, rv0)


def test_layer_norm_cpu_fallback_matches_f64():
    D = 20
    g = torch.Generator().manual_seed(5)
    x = torch.randn(7, D, generator=g) * 2.0 ** torch.arange(-3, 4).float()[:, None] + 3.0
    gamma, beta = torch.rand(D, generator=g) + 0.5, torch.randn(D, generator=g)
    y = ops.layer_norm(x, gamma, beta, eps=1e-5)
    ref = F.layer_norm(x.double(), (D,), gamma.double(), beta.double(), 1e-5)
    check_rows("layer_norm D=20", y, ref, 1e-5)


def test_max_pool_cpu_fallback_matches_first_tap_reference():
    g = torch.Generator().manual_seed(6)
    x = torch.randn(2, 9, 7, 20, generator=g)
    for H, W, k, s, p in POOL_GEOS:
        xs = x[:, :H, :W].contiguous()
        y = ops.max_pool2d(xs, _pair(k), _pair(s), _pair(p))
        v, _ = maxpool_first(xs, k, s, p)
        assert torch.equal(y.contiguous(), v)
