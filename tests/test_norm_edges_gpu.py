"""Batch norm, the fused BN + ReLU + max-pool stem kernels and layer norm (csrc/kernels/norm.hip) against float64
references, PER CHANNEL (per row for layer norm), at the shapes where the kernels take another path: channel counts
whose column-reduction geometry leaves threads idle (C = 24, 40, 72), one thread per row (C = 8), a second channel trip
(C = 2056), row counts below one block / one trip / a ragged tail, reductions tall enough to launch the partial-row
grouping pass (narrow and generic variant), every relu x residual mode, inference, the ymask route and the fused
shortcut statistics of dtf_bn_bwd, the generic and the 2x2-block geometry of the stem kernels, and every
ln_fwd_kernel<NC> / ln_bwd_kernel<NC> boundary.

Batch-norm inputs: channel c has standard deviation 2^((c % 13) - 6) and mean ((c % 5) - 2) * 4 standard deviations
(channel scales span 2^12, means reach 8 sigma, 16 in one case), rounded to bf16 before the reference sees them. A
tensor-wide comparison would only see the largest channels.

Bounds (none taken from the kernels' output):
  bf16 outputs (y, dx, dres)    per-channel err <= 2^-8 (_rowcmp.ULP): one rounding of an f32 value whose statistics
                                are good to 1e-4 is half an ulp, 2^-9, of the channel's largest value
  f32 sums, statistics          |err_c| <= 1e-4 * (float64 sum of |terms| of channel c)       (_rowcmp.check_sums)
  bitwise claims                torch.equal
Two places where an error relative to the reference alone is undefined, with the reasoning at the assertion: dx of a
one-row batch (the reference is exactly 0) and layer norm's dgamma terms (the saved f32 mean at 50 sigma cannot hold
xhat closer than 6e-6, which is allowed on top of the summation bound).

Measured on MI355X, worst over all cases (the rounded baseline = the float64 result rounded to bf16, from the
reference alone, in brackets):
  batch norm    y 3.83e-3 [3.83e-3], dx 3.86e-3 [3.86e-3], dres 0, inference y 3.78e-3 [3.78e-3];
                dgamma 1.5e-6, dbeta 1.3e-8, running_mean 3.4e-7, running_var 1.3e-6 (of the 1e-4 bound's scale)
  dtf_bn_bwd    dx 3.27e-3 [3.27e-3], dgamma 8.1e-8, dbeta 4.4e-9, part2 1.7e-9 / 1.7e-8
  fused stem    y 0 (exact), dx 3.67e-3 [3.67e-3], dgamma 1.6e-7, dbeta 0
  layer norm    y 3.89e-3 [3.89e-3], dx 3.83e-3 [3.83e-3], dgamma 1.8e-5, dbeta 1.1e-8; D = 20 / 2056 (PyTorch path)
                y 2.70e-3, dx 3.52e-3
Every bf16 output sits at its rounded baseline (ratio 1.00): no case needed more than 2^-8.
Constant channels: all 0 and all 2.5 give y = beta to bf16 rounding and a variance of 0 into running_var (|.| < 4e-7,
the f32 rounding of 0.9 * running_var); the constant-100 channel at M = 33000 gives max |y - beta| = 1.05e-3 (the bf16
rounding of beta) and a batch variance of 0 to the same rounding, since bn_stats_kernel sums x - x[row 0].

What these tests found (fixed with them): the standalone statistics formed var = E[x^2] - mean^2 from unshifted f32
sums (M = 3 rows whose spread is small against their mean: invstd off by 1.5e-4, dgamma 1.5x over its bound), and the
apply pass folded the mean into shift = beta - mean * scale, which loses 2^-24 |mean * scale| (M = 1, x = -256,
variance 0: y off beta by 2.6e-2 of the channel). ops.layer_norm raised for D > 2048.
"""
import pytest
import torch

from distributed_tensorflow_amd import ops
from distributed_tensorflow_amd.ops._util import IntOut, call, ptr, stream

from _rowcmp import (ULP, bf16_round, bn_f64, chan_base, check_chans, check_rows, check_sums, maxpool_first,
                     maxpool_scatter, maxpool_unique, row_err)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
EPS, MOM = 1e-3, 0.9
_WORST = {}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


# ------------------------------------------------------------------ batch norm through ops.batch_norm
def _bn_inputs(shape, C, kmean=4, const=()):
    """CPU tensors: bf16 x / dy / res, f32 gamma / beta / running statistics. const: (channel, value) pairs."""
    g = torch.Generator().manual_seed(C * 1000 + shape[0] * shape[1] * shape[2] + kmean)
    c = torch.arange(C)
    std = 2.0 ** ((c % 13) - 6).double()
    mean = ((c % 5) - 2).double() * kmean * std
    x = torch.randn(*shape, C, generator=g, dtype=F64) * std + mean
    for ch, val in const:
        x[..., ch] = val
    dy = torch.randn(*shape, C, generator=g).to(BF)
    res = torch.randn(*shape, C, generator=g).to(BF)
    gamma = torch.rand(C, generator=g) + 0.5
    beta = torch.randn(C, generator=g) * 0.5
    rm = torch.randn(C, generator=g)
    rv = torch.rand(C, generator=g) + 0.5
    return x.to(BF), dy, res, gamma, beta, rm, rv


def _bn_train(cuda, shape, C, relu=False, with_res=False, kmean=4, const=(), skip=()):
    """One training step of ops.batch_norm and its backward against bn_f64; returns (outputs, reference) for extra
    assertions. skip: channels left out of the comparisons (still required to be finite)."""
    x, dy, res, gamma, beta, rm0, rv0 = _bn_inputs(shape, C, kmean, const)
    xg, gg, bg = (t.to(cuda).requires_grad_(True) for t in (x, gamma, beta))
    rg = res.to(cuda).requires_grad_(True) if with_res else None
    rm, rv = rm0.to(cuda), rv0.to(cuda)
    y = ops.batch_norm(xg, gg, bg, rm, rv, training=True, momentum=MOM, eps=EPS, relu=relu, residual=rg)
    y.backward(dy.to(cuda))
    torch.cuda.synchronize()
    assert y.dtype == BF and xg.grad.dtype == BF
    r = bn_f64(x, gamma, beta, EPS, res=res if with_res else None, relu=relu, dy=dy)
    M = x.numel() // C
    keep = torch.tensor([c not in skip for c in range(C)])
    for t in (y, xg.grad, gg.grad, bg.grad, rm, rv):
        assert torch.isfinite(t).all()
    tag = f"bn M={M} C={C}"
    check_chans(f"{tag} y", y.cpu()[..., keep], r.y[..., keep], ULP, _WORST, chan_base(r.y[..., keep]))
    if M == 1:
        # the reference gradient is exactly 0 (dz - mean(dz) with one row), so an error relative to it is undefined:
        # the kernel's a*dz + (b*x + c) cancels two f32 terms of size gamma * invstd * |dz|, bounded relative to them
        term = (gamma.double() * r.invstd * dy.double().abs()).reshape(xg.grad.shape)
        assert (r.dx == 0).all() and (xg.grad.double().cpu().abs() <= ULP * term).all()
    else:
        check_chans(f"{tag} dx", xg.grad.cpu()[..., keep], r.dx[..., keep], ULP, _WORST, chan_base(r.dx[..., keep]))
    if with_res:
        check_chans(f"{tag} dres", rg.grad.cpu(), r.dres, ULP, _WORST)
        if not relu:
            assert torch.equal(rg.grad.cpu(), dy)
    check_sums(f"{tag} dgamma", gg.grad.cpu()[keep], r.dgamma[keep], r.dgamma_scale[keep], 1e-4, _WORST)
    check_sums(f"{tag} dbeta", bg.grad.cpu()[keep], r.dbeta[keep], r.dbeta_scale[keep], 1e-4, _WORST)
    # running statistics: batch_norm_ref's rule in float64; the scale of each is the sum of its |terms| (the variance is
    # formed as E[x^2] - mean^2, so those two are its terms)
    f = M / max(M - 1, 1)
    x2 = x.double().reshape(-1, C)
    rm_ref = rm0.double() * MOM + r.mean * (1 - MOM)
    rv_ref = rv0.double() * MOM + r.var * f * (1 - MOM)
    rm_scale = rm0.double().abs() * MOM + x2.abs().mean(0) * (1 - MOM)
    rv_scale = rv0.double() * MOM + ((x2 * x2).mean(0) + r.mean ** 2) * f * (1 - MOM)
    check_sums(f"{tag} running_mean", rm.cpu()[keep], rm_ref[keep], rm_scale[keep], 1e-4, _WORST)
    check_sums(f"{tag} running_var", rv.cpu()[keep], rv_ref[keep], rv_scale[keep], 1e-4, _WORST)
    out = dict(y=y.cpu(), dx=xg.grad.cpu(), rm=rm.cpu(), rv=rv.cpu(), rm0=rm0, rv0=rv0, beta=beta, M=M)
    return out, r


@pytest.mark.parametrize("C", [8, 24, 40, 72, 264, 2056])
def test_bn_channel_geometry(cuda, C):
    """TPR = C/8 threads per row: 1 (256 rows per pass), 3 / 5 / 9 (255, 255, 252 active threads), 33, and 257 column
    chunks (bn_stats_kernel and bn_bwd_reduce_kernel take a second channel trip)."""
    _bn_train(cuda, (2, 7, 7), C)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 3, 1), (1, 1, 5), (1, 15, 17)], ids=["M1", "M3", "M5", "M255"])
def test_bn_short_and_ragged_rows(cuda, shape):
    """C = 64 (32 rows per pass): fewer rows than one pass, than one unrolled trip, and a ragged tail (M = 255: the
    unrolled loop and the tail loop both run). M = 1: the unbiased factor's M > 1 guard."""
    _bn_train(cuda, shape, 64)


@pytest.mark.parametrize("shape,C", [((33, 40, 25), 512), ((33, 20, 25), 1024)], ids=["narrow", "generic"])
def test_bn_partial_row_grouping(cuda, shape, C):
    """More than 256 reduction blocks (M > 8192 * RPB), so dtf_group_rows_once runs before both finalize kernels: its
    narrow variant for 2C <= 1024 floats per row, the generic one above."""
    _bn_train(cuda, shape, C)


@pytest.mark.parametrize("C", [24, 64])
@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("relu", [False, True], ids=["norelu", "relu"])
def test_bn_modes(cuda, C, relu, with_res):
    """relu without a residual has no dres; a residual without relu gets dy itself; with both, the masked dz."""
    _bn_train(cuda, (2, 7, 7), C, relu=relu, with_res=with_res)


def test_bn_mean_offset_16_sigma(cuda):
    """Channel means up to 16 standard deviations: var = E[x^2] - mean^2 cancels 257 : 1 in f32."""
    _bn_train(cuda, (8, 40, 25), 64, kmean=8)


def test_bn_constant_channels(cuda):
    """An all-0 and an all-2.5 channel: their f32 sums are exact, so y = beta, dx is finite (and right) and the batch
    variance that enters running_var is 0."""
    out, r = _bn_train(cuda, (4, 25, 25), 64, const=((3, 0.0), (10, 2.5)))
    for ch in (3, 10):
        # (y against the reference, which is beta in these channels, was compared per channel by _bn_train)
        assert r.var[ch] == 0 and (r.y[..., ch] == out["beta"][ch].double()).all()
        var_in = (out["rv"][ch].double() - out["rv0"][ch].double() * MOM) / (1 - MOM)
        assert abs(var_in.item()) <= 1e-5 * out["rv0"][ch].item(), var_in   # f32 rounding of 0.9 * rv0 only
        dev = (out["y"][..., ch].double() - out["beta"][ch].double()).abs().max().item()
        print(f"  constant channel {ch}: max |y - beta| = {dev:.3e}, variance into running_var = {var_in.item():.3e}")


def test_bn_constant_channel_100_tall(cuda):
    """A channel of constant 100 over M = 33000 rows: its plain sum of squares (3.3e8) is not exact in f32, and a
    variance formed from it is some small positive number where the true one is 0. Only finiteness is asserted for
    that channel; the other channels keep their bounds. Measured on MI355X with the row-0 pivot in bn_stats_kernel:
    max |y - beta| = 1.05e-3 (the bf16 rounding of beta), batch variance -4.8e-7 (the f32 rounding of the
    running_var update it is read back from; the kernel's value is 0)."""
    ch = 5
    out, r = _bn_train(cuda, (33, 40, 25), 64, const=((ch, 100.0),), skip=(ch,))
    assert torch.isfinite(out["y"][..., ch]).all() and torch.isfinite(out["dx"][..., ch]).all()
    M = out["M"]
    var_in = (out["rv"][ch].double() - out["rv0"][ch].double() * MOM) / (1 - MOM) * (M - 1) / M
    dev = (out["y"][..., ch].double() - out["beta"][ch].double()).abs().max().item()
    print(f"  constant 100, M={M}: max |y - beta| = {dev:.3e}, batch variance = {var_in.item():.3e} (true 0)")


@pytest.mark.parametrize("C", [8, 264, 2056])
def test_bn_inference(cuda, C):
    """training=False (bn_infer_coeff_kernel): y from the running statistics, which stay bitwise unchanged."""
    shape = (2, 7, 7)
    x, dy, res, gamma, beta, _, _ = _bn_inputs(shape, C)
    g = torch.Generator().manual_seed(C)
    c = torch.arange(C)
    std = 2.0 ** ((c % 13) - 6).float()
    rm0 = ((c % 5) - 2).float() * 4 * std + 0.5 * std * torch.randn(C, generator=g)
    rv0 = 10.0 ** (torch.rand(C, generator=g) * 6 - 3)            # log-uniform in [1e-3, 1e3]
    rm, rv = rm0.to(cuda), rv0.to(cuda)
    y = ops.batch_norm(x.to(cuda), gamma.to(cuda), beta.to(cuda), rm, rv, training=False, momentum=MOM, eps=EPS)
    torch.cuda.synchronize()
    ref = (x.double() - rm0.double()) * torch.rsqrt(rv0.double() + EPS) * gamma.double() + beta.double()
    check_chans(f"bn inference C={C} y", y.cpu(), ref, ULP, _WORST, chan_base(ref))
    assert torch.equal(rm.cpu(), rm0) and torch.equal(rv.cpu(), rv0)


# ------------------------------------------------------------------ raw dtf_bn_bwd
def _raw_bn_fwd(cuda, x, gamma, beta, res):
    """dtf_bn_stats + dtf_bn_finalize_pivot + dtf_bn_apply with ReLU and mask bits on [M, C] tensors."""
    M, C = x.shape
    part = torch.empty(1024 * 2 * C, dtype=F32, device=cuda)
    rows = IntOut()
    call("dtf_bn_stats", ptr(x), M, C, ptr(part), rows.addr, stream())
    scale, shift, mean, invstd = (torch.empty(C, dtype=F32, device=cuda) for _ in range(4))
    call("dtf_bn_finalize_pivot", ptr(part), rows.value, ptr(x), ptr(gamma), ptr(beta), None, None, M, C, MOM, EPS,
         ptr(scale), ptr(shift), ptr(mean), ptr(invstd), stream())
    y = torch.empty_like(x)
    mbits = torch.empty(M * C // 8, dtype=torch.uint8, device=cuda)
    call("dtf_bn_apply", ptr(x), ptr(scale), ptr(shift), ptr(res), ptr(y), M, C, 1, ptr(mbits), None, None, stream())
    return y, mbits, mean, invstd


def _raw_bn_bwd(cuda, dy, ymask, mbits, x, mean, invstd, gamma, sc=None):
    M, C = x.shape
    dx, dz = (torch.full_like(x, float("nan")) for _ in range(2))
    dg, db = (torch.full((C,), float("nan"), dtype=F32, device=cuda) for _ in range(2))
    work = torch.empty((2 * 1024 + 3) * C, dtype=F32, device=cuda)
    rows2 = IntOut()
    x2, mean2, part2 = sc if sc is not None else (None, None, None)
    call("dtf_bn_bwd", ptr(dy), ptr(ymask), ptr(mbits), ptr(x), ptr(mean), ptr(invstd), ptr(gamma), M, C, ptr(dx),
         ptr(dz), ptr(dg), ptr(db), 0, ptr(work), ptr(x2), ptr(mean2), ptr(part2), rows2.addr if sc else None,
         stream())
    torch.cuda.synchronize()
    return dx, dz, dg, db, rows2.value


@pytest.mark.parametrize("C", [24, 64])
def test_bn_bwd_ymask_route_and_shortcut_statistics(cuda, C):
    """The ReLU mask read from the forward's bf16 output (ymask) gives bitwise what the 1-bit mask gives. With x2 /
    mean2 / part2 the apply pass also leaves the shortcut BatchNorm's partial sums over the stored bf16 dz: at C = 64
    (TPR * RPB == 256) as rows2 > 0 partial rows; at C = 24 the fusion is declined (rows2 == 0) and dx is still right."""
    M = 1000
    x, dy, res, gamma, beta, _, _ = _bn_inputs((1, M, 1), C)
    x, dy, res = (t.reshape(M, C).to(cuda) for t in (x, dy, res))
    gg, bg = gamma.to(cuda), beta.to(cuda)
    y, mbits, mean, invstd = _raw_bn_fwd(cuda, x, gg, bg, res)
    a = _raw_bn_bwd(cuda, dy, None, mbits, x, mean, invstd, gg)
    b = _raw_bn_bwd(cuda, dy, y, None, x, mean, invstd, gg)
    for name, u, v in zip(("dx", "dz_out", "dgamma", "dbeta"), a, b):
        assert torch.equal(u, v), f"{name}: the ymask route differs from the mbits route"
    assert a[4] == 0 and b[4] == 0
    # reference from the kernel's own mask (y > 0), so that an element within rounding of 0 cannot flip it
    dz_ref = dy * (y > 0)
    assert torch.equal(a[1], dz_ref)
    r = bn_f64(x.cpu(), gamma, beta, EPS, dy=dz_ref.cpu())
    check_chans(f"bn_bwd C={C} dx", a[0].cpu(), r.dx, ULP, _WORST, chan_base(r.dx))
    check_sums(f"bn_bwd C={C} dgamma", a[2].cpu(), r.dgamma, r.dgamma_scale, 1e-4, _WORST)
    check_sums(f"bn_bwd C={C} dbeta", a[3].cpu(), r.dbeta, r.dbeta_scale, 1e-4, _WORST)
    # fused shortcut statistics
    g = torch.Generator().manual_seed(C)
    x2 = (torch.randn(M, C, generator=g) * 2 + 1).to(BF).to(cuda)
    mean2 = (torch.randn(C, generator=g) * 0.5 + 1).to(cuda)
    part2 = torch.full((2048 * 2 * C,), float("nan"), dtype=F32, device=cuda)
    s = _raw_bn_bwd(cuda, dy, None, mbits, x, mean, invstd, gg, sc=(x2, mean2, part2))
    assert torch.equal(s[0], a[0]) and torch.equal(s[1], a[1]) and torch.equal(s[2], a[2]) and torch.equal(s[3], a[3])
    if C == 64:
        T = s[4]
        assert 0 < T <= 2048
        assert torch.isnan(part2[T * 2 * C:]).all(), "wrote past its partial rows"
        sums = part2[:T * 2 * C].view(T, 2 * C).double().sum(0).cpu()
        dz = dz_ref.double().cpu()
        t2 = dz * (x2.double().cpu() - mean2.double().cpu())
        check_sums("bn_bwd part2 sum dz", sums[:C], dz.sum(0), dz.abs().sum(0), 1e-4, _WORST)
        check_sums("bn_bwd part2 sum dz*(x2-mean2)", sums[C:], t2.sum(0), t2.abs().sum(0), 1e-4, _WORST)
    else:
        assert s[4] == 0
        assert torch.isnan(part2).all()


# ------------------------------------------------------------------ fused BN + ReLU + max pool (the stem)
@pytest.mark.parametrize("N,H,W,C,k,s,p", [(2, 8, 12, 24, 3, 2, 1), (2, 7, 9, 24, 3, 2, 1), (1, 8, 8, 8, 2, 2, 0),
                                           (1, 6, 6, 64, 3, 1, 1)], ids=["B2", "odd", "2x2s2p0", "3x3s1"])
def test_bn_relu_maxpool_fused(cuda, N, H, W, C, k, s, p):
    """dtf_bn_relu_maxpool_fwd / dtf_maxpool_bn_bwd against BN apply -> ReLU -> bf16 round -> first-tap max pool and
    its float64 backward. 8x12 with 3x3/2/1 takes the 2x2-block kernels (<B2 = true>), the others the generic ones."""
    x, _, _, gamma, beta, _, _ = _bn_inputs((N, H, W), C)
    g = torch.Generator().manual_seed(N * H * W * C)
    st = bn_f64(x, gamma, beta, EPS)
    scale64 = gamma.double() * st.invstd
    scale, shift = scale64.float(), (beta.double() - st.mean * scale64).float()
    mean, invstd = st.mean.float(), st.invstd.float()
    v = bf16_round(torch.relu(x.double() * scale.double() + shift.double()))      # what the unfused apply stores
    yref, idx = maxpool_first(v, k, s, p)
    P, Q = yref.shape[1:3]
    xg, scg, shg, meang, invg = (t.to(cuda) for t in (x, scale, shift, mean, invstd))
    y = torch.empty(N, P, Q, C, dtype=BF, device=cuda)
    arg = torch.empty(N, P, Q, C, dtype=torch.uint8, device=cuda)
    geo = (N, H, W, C, P, Q, k, k, s, s, p, p)
    call("dtf_bn_relu_maxpool_fwd", ptr(xg), ptr(scg), ptr(shg), ptr(y), ptr(arg), *geo, stream())
    torch.cuda.synchronize()
    tag = f"stem {H}x{W} C={C}"
    check_chans(f"{tag} y", y.cpu(), yref, ULP, _WORST)
    a = arg.cpu().long()
    uniq = maxpool_unique(v, k, s, p)
    assert uniq.any() and torch.equal((a & 127)[uniq], idx[uniq]), "argmax tap differs where the maximum is unique"
    assert torch.equal((a & 128) != 0, yref > 0), "bit 7 is not y > 0"
    # backward
    dy = torch.randn(N, P, Q, C, generator=g).to(BF)
    dz = bf16_round(maxpool_scatter(dy.double() * (yref > 0), idx, H, W, k, s, p))
    r = bn_f64(x, gamma, beta, EPS, dy=dz)
    dyg, gg = dy.to(cuda), gamma.to(cuda)
    work = torch.empty((2 * 1024 + 3) * C, dtype=F32, device=cuda)
    outs = []
    for with_dx in (True, False):
        dx = torch.full((N, H, W, C), float("nan"), dtype=BF, device=cuda) if with_dx else None
        dg, db = (torch.full((C,), float("nan"), dtype=F32, device=cuda) for _ in range(2))
        call("dtf_maxpool_bn_bwd", ptr(dyg), ptr(arg), ptr(xg), ptr(meang), ptr(invg), ptr(gg), *geo, ptr(dx),
             ptr(dg), ptr(db), 0, ptr(work), stream())
        torch.cuda.synchronize()
        outs.append((dx, dg.cpu(), db.cpu()))
    dx, dg, db = outs[0]
    check_chans(f"{tag} dx", dx.cpu(), r.dx, ULP, _WORST, chan_base(r.dx))
    check_sums(f"{tag} dgamma", dg, r.dgamma, r.dgamma_scale, 1e-4, _WORST)
    check_sums(f"{tag} dbeta", db, r.dbeta, r.dbeta_scale, 1e-4, _WORST)
    assert torch.equal(outs[1][1], dg) and torch.equal(outs[1][2], db), "dx = None changes dgamma / dbeta"


# ------------------------------------------------------------------ layer norm
def _ln_inputs(M, D):
    g = torch.Generator().manual_seed(M * 10000 + D)
    std = 2.0 ** ((torch.arange(M) % 9) - 4).double()[:, None]
    x = ((torch.randn(M, D, generator=g, dtype=F64) + 50.0) * std).to(BF)
    dy = torch.randn(M, D, generator=g).to(BF)
    gamma = torch.rand(D, generator=g) + 0.5
    gamma[torch.randperm(D, generator=g)[:max(1, D // 8)]] = 0.0
    beta = torch.randn(D, generator=g) * 0.5
    return x, dy, gamma, beta


def _ln_f64(x, gamma, beta, eps, dy):
    xd = x.double().cpu().requires_grad_(True)
    gd, bd = (t.double().cpu().requires_grad_(True) for t in (gamma, beta))
    y = torch.nn.functional.layer_norm(xd, (x.shape[-1],), gd, bd, eps)
    dx, dg, db = torch.autograd.grad(y, [xd, gd, bd], dy.double().cpu())
    mu = xd.mean(-1, keepdim=True).detach()
    rstd = torch.rsqrt(xd.var(-1, unbiased=False, keepdim=True) + eps).detach()
    xhat = (xd.detach() - mu) * rstd
    dyd = dy.double().cpu()
    # dgamma's terms dy * xhat are not exact inputs of the sum: the backward forms xhat = (x - mean) * rstd from the
    # saved f32 mean, which cannot hold the mean closer than one f32 ulp (2^-23 |mean|); with the mean at 50 sigma that
    # is 6e-6 in xhat, more than 1e-4 of a term wherever |xhat| < 0.06 (and with one row the "sum" is that one term).
    # That representation error of each term is allowed on top of the 1e-4 summation bound (folded into the scale).
    term_err = (dyd.abs() * rstd * mu.abs() * 2.0 ** -23).sum(0)
    return y.detach(), dx, dg, db, (dyd * xhat).abs().sum(0) + term_err / 1e-4, dyd.abs().sum(0)


def _ln_check(cuda, M, D, eps, tag):
    x, dy, gamma, beta = _ln_inputs(M, D)
    xg, gg, bg = (t.to(cuda).requires_grad_(True) for t in (x, gamma, beta))
    y = ops.layer_norm(xg, gg, bg, eps=eps)
    y.backward(dy.to(cuda))
    torch.cuda.synchronize()
    assert y.dtype == BF and xg.grad.dtype == BF
    yr, dxr, dgr, dbr, gs, bs = _ln_f64(x, gamma, beta, eps, dy)
    check_rows(f"{tag} y", y.cpu(), yr, ULP, _WORST, row_err(bf16_round(yr), yr).max().item())
    check_rows(f"{tag} dx", xg.grad.cpu(), dxr, ULP, _WORST, row_err(bf16_round(dxr), dxr).max().item())
    check_sums(f"{tag} dgamma", gg.grad.cpu(), dgr, gs, 1e-4, _WORST)
    check_sums(f"{tag} dbeta", bg.grad.cpu(), dbr, bs, 1e-4, _WORST)


@pytest.mark.parametrize("eps", [1e-5, 1e-12])
@pytest.mark.parametrize("M", [1, 3, 4, 5, 130])
@pytest.mark.parametrize("D", [8, 264, 512, 520, 1024, 1032, 1536, 1544, 2048])
def test_layer_norm_edges(cuda, D, M, eps):
    """Both sides of every NC boundary (512 / 1024 / 1536 / 2048), one lane (D = 8), one row, a partial 4-row block.
    Row r has standard deviation 2^((r % 9) - 4) and mean 50 standard deviations (the kernel is two-pass); gamma has
    exact zeros."""
    _ln_check(cuda, M, D, eps, "ln")


@pytest.mark.parametrize("D", [20, 2056])
def test_layer_norm_widths_without_a_kernel(cuda, D):
    """D % 8 != 0 and D > 2048 have no kernel: ops.layer_norm computes them with PyTorch (D = 2056 used to raise
    'dtf_layernorm_fwd failed with status -1')."""
    _ln_check(cuda, 5, D, 1e-5, f"ln fallback D={D}")


def test_layer_norm_bwd2_raw(cuda):
    """dtf_layernorm_bwd2 at M = 100, D = 264: a workspace of 3 partial rows caps the launch at 3 blocks (and nothing
    is written behind them); res is joined as round(round(dx) + res); accumulate = 1 adds to dgamma | dbeta."""
    M, D, eps = 100, 264, 1e-5
    x, dy, gamma, beta = _ln_inputs(M, D)
    xg, dyg, gg, bg = (t.to(cuda) for t in (x, dy, gamma, beta))
    y = torch.empty_like(xg)
    mean, rstd = (torch.empty(M, dtype=F32, device=cuda) for _ in range(2))
    call("dtf_layernorm_fwd", ptr(xg), ptr(gg), ptr(bg), ptr(y), ptr(mean), ptr(rstd), M, D, eps, stream())
    yr, dxr, dgr, dbr, gs, bs = _ln_f64(x, gamma, beta, eps, dy)
    ref, scale = torch.cat([dgr, dbr]), torch.cat([gs, bs])

    def bwd(ws_rows, acc, res, dgb):
        ws = torch.full((8 * 2 * D,), float("nan"), dtype=F32, device=cuda)
        dx = torch.full_like(xg, float("nan"))
        call("dtf_layernorm_bwd2", ptr(dyg), ptr(xg), ptr(gg), ptr(mean), ptr(rstd), ptr(dx), ptr(dgb), ptr(ws),
             ws_rows * 2 * D, M, D, acc, ptr(res), stream())
        torch.cuda.synchronize()
        assert torch.isnan(ws[ws_rows * 2 * D:]).all(), "wrote past ws_elems"
        assert torch.isfinite(ws[:min(ws_rows, 25) * 2 * D]).all()
        return dx

    dgb = torch.full((2 * D,), float("nan"), dtype=F32, device=cuda)
    dx = bwd(3, 0, None, dgb)
    check_rows("ln_bwd2 dx", dx.cpu(), dxr, ULP, _WORST)
    check_sums("ln_bwd2 capped dgamma|dbeta", dgb.cpu(), ref, scale, 1e-4, _WORST)
    dgb8 = torch.full((2 * D,), float("nan"), dtype=F32, device=cuda)
    dx8 = bwd(8, 0, None, dgb8)
    assert torch.equal(dx8, dx)
    check_sums("ln_bwd2 dgamma|dbeta", dgb8.cpu(), ref, scale, 1e-4, _WORST)
    g = torch.Generator().manual_seed(9)
    res = torch.randn(M, D, generator=g).to(BF).to(cuda)
    g0 = torch.randn(2 * D, generator=g)
    acc = g0.to(cuda)
    dxres = bwd(3, 1, res, acc)
    assert torch.equal(dxres, (dx.float() + res.float()).to(BF)), "dx with res is not round(round(dx) + res)"
    check_sums("ln_bwd2 accumulate", acc.cpu(), g0.double() + ref, g0.double().abs() + scale, 1e-4, _WORST)
