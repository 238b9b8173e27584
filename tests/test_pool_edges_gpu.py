"""Max pool and global average pool (csrc/kernels/pool.hip) against references that do not depend on PyTorch's tie
rule, at the geometries the ResNet never uses: odd maps, pad 0, overlapping stride-1 windows (an input pixel wins
several windows), stride == kernel, 1x1, a rectangular window; C = 8 (one chunk per pixel); inputs that are all
negative (zero padding instead of -inf would win every border window) or full of ties (the first maximal tap in (r, s)
order takes the gradient).

Bounds: the pooled values are exact (max of bf16 values); the gradients are sums of at most nine bf16 values in f32
rounded once, per-channel err <= 2^-8 (_rowcmp.ULP) against the float64 scatter rounded to bf16; the global average is
an f32 sum, |err| <= 1e-4 * mean |x| per (n, c) as f32 output and one bf16 rounding more (2^-8) as bf16 output.

Measured on MI355X, worst over all cases: max-pool values exact and dx error 0 for all three input kinds (every sum
of up to nine gradients rounds as the float64 one does); global average f32 output 8.0e-8 of its scale, bf16 output
3.86e-3 per channel, dx 0 from both an f32 and a bf16 dy.
"""
import pytest
import torch

from distributed_tensorflow_amd import ops
from distributed_tensorflow_amd.ops._util import call, ptr, stream

from _rowcmp import POOL_GEOS, ULP, _pair, bf16_round, check_chans, check_sums, maxpool_first, maxpool_scatter

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
_WORST = {}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("geo", POOL_GEOS, ids=str)
def test_max_pool_edges(cuda, geo, C, N):
    H, W, k, s, p = geo
    g = torch.Generator().manual_seed(H * 1000 + W * 10 + C + N)
    for kind in ("randn", "negative", "ties"):
        x = torch.randn(N, H, W, C, generator=g)
        if kind == "negative":
            x = -3.0 - x.abs()
        elif kind == "ties":
            x = torch.randint(-2, 3, (N, H, W, C), generator=g).float()
        x = x.to(BF)
        yref, idx = maxpool_first(x, k, s, p)
        dy = torch.randn(yref.shape, generator=g).to(BF)
        dxref = bf16_round(maxpool_scatter(dy, idx, H, W, k, s, p))
        xg = x.to(cuda).requires_grad_(True)
        y = ops.max_pool2d(xg, _pair(k), _pair(s), _pair(p))
        y.backward(dy.to(cuda))
        torch.cuda.synchronize()
        assert y.dtype == BF and torch.equal(y.cpu(), yref), f"{kind}: pooled values differ"
        if kind == "negative":
            assert (y <= -3).all()
        check_chans(f"maxpool {kind} dx", xg.grad.cpu(), dxref, ULP, _WORST)
        # every pooled gradient lands on exactly one input pixel
        assert (dxref != 0).any()


def _gap_inputs(N, HW, C):
    g = torch.Generator().manual_seed(N * 100000 + HW * 10 + C)
    c = torch.arange(C)
    std = 2.0 ** ((c % 13) - 6).double()
    x = ((torch.randn(N, HW, C, generator=g, dtype=torch.float64) + ((c % 5) - 2).double() * 4) * std).to(BF)
    dy = (torch.randn(N, C, generator=g, dtype=torch.float64) * std).float()
    return x, dy


@pytest.mark.parametrize("N,H,W,C", [(1, 1, 1, 8), (2, 7, 7, 2056), (3, 56, 56, 64)])
def test_global_avg_pool_edges(cuda, N, H, W, C):
    """HW = 1, a second block of channel chunks (C = 2056 > 8 * 256), and a long f32 sum (HW = 3136); bf16 output
    through ops.global_avg_pool, f32 output through dtf_gap_fwd(out_f32 = 1); the backward for an f32 and a bf16 dy."""
    HW = H * W
    x, dy = _gap_inputs(N, HW, C)
    xd = x.double()
    ref, scale = xd.mean(1), xd.abs().mean(1)
    xg = x.reshape(N, H, W, C).to(cuda).requires_grad_(True)
    y = ops.global_avg_pool(xg)
    dyb = dy.to(BF)
    y.backward(dyb.to(cuda))
    y32 = torch.full((N, C), float("nan"), dtype=F32, device=cuda)
    call("dtf_gap_fwd", ptr(xg), ptr(y32), N, HW, C, 1, stream())
    dx32 = torch.full((N, HW, C), float("nan"), dtype=BF, device=cuda)
    dyg = dy.to(cuda)
    call("dtf_gap_bwd", ptr(dyg), 1, ptr(dx32), N, HW, C, stream())
    torch.cuda.synchronize()
    tag = f"gap HW={HW} C={C}"
    assert y.dtype == BF and y.shape == (N, C)
    check_sums(f"{tag} y f32", y32.cpu(), ref, scale, 1e-4, _WORST)
    check_chans(f"{tag} y bf16", y.cpu(), ref, ULP, _WORST)
    for name, got, d in (("bf16", xg.grad.reshape(N, HW, C), dyb), ("f32", dx32, dy)):
        dref = bf16_round((d.double() / HW)[:, None, :].expand(N, HW, C))
        assert got.dtype == BF
        check_chans(f"{tag} dx from {name} dy", got.cpu(), dref, ULP, _WORST)
