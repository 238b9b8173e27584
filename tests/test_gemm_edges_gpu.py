"""Exact and per-element reference tests of the bf16 GEMM routes (gemm.hip + gemm_core.h, gemm_w4.hip, gemm256.hip,
the split-K slab reductions) against float64 references (tests/_gemmref.py).

Small-integer operands make every route reproduce the float64 result bit for bit (f32 outputs as they are, bf16 outputs
as its nearest-even image); every test asserts through the launch counters that it ran on the kernel it names, and
every strided output is a view of a sentinel-filled buffer that is checked for stores past row M / column N.

Shapes are the smallest at which each kernel can go wrong: M 8 (one partial tile), 264 (one full 256 tile + 8 rows), 257
(odd, K-contiguous A only), 1; N 8, 136 (one full 128 tile + 8), 264, 132 (N % 8 != 0: no staged bf16 store); K 64 (one
K-tile), 128 (the fewest the 8-wave kernel takes), 192 (odd count of K-tiles), 72 and 8 (partial K-tile, generic only).

Two properties of the kernels, read from their code, shape the bf16 `beta` cases: the staged bf16 epilogues (4-wave,
8-wave and the generic kernel's staged path) round alpha * A B^T to bf16 BEFORE adding beta * C (documented: "exactly
the unfused GEMM followed by an elementwise add"), so those cases use operands in [-1, 1], whose products (|.| <= 192)
are bf16 values and the single remaining rounding is the reference's.
"""
import pytest
import torch

from distributed_tensorflow_amd import ops
from distributed_tensorflow_amd.ops import linalg as LA
from distributed_tensorflow_amd.ops._util import call, launch_counts, launch_delta, ptr, stream, workspace

from _gemmref import (SENTINEL, abs_product, assert_exact, bf16_half_ulp, bf16_round, check_elems, gelu_f64, gemm_f64,
                      guarded_out, int_operand)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]
WORST = {}  # worst err / bound of the random-normal cases, printed per test


# ---------------------------------------------------------------- operands and references (computed once, shared)
_CACHE = {}


def operands(M, N, K, lo=-3, hi=3, seed=0, kind="int"):
    """Logical A [M, K], B [N, K] (bf16, CPU) and their float64 product, cached per shape."""
    key = (M, N, K, lo, hi, seed, kind)
    if key not in _CACHE:
        if kind == "int":
            A, B = int_operand((M, K), lo, hi, 11 + seed), int_operand((N, K), lo, hi, 23 + seed)
        elif kind == "eye":  # A = I, B asymmetric: a transposed or mis-tiled store shows (values < 251: bf16 integers)
            A = torch.eye(M, K).to(BF)
            B = torch.arange(N * K, dtype=torch.float32).reshape(N, K).remainder(251).to(BF)
        else:
            g = torch.Generator().manual_seed(5 + seed)
            A, B = torch.randn(M, K, generator=g).to(BF), torch.randn(N, K, generator=g).to(BF)
        _CACHE[key] = (A, B, gemm_f64(A, B)[1], abs_product(A, B))
    return _CACHE[key]


def stored(t, kouter, dev, ld_extra=0):
    """The operand as the kernel reads it: [rows, K] or, K-outer, [K, rows]; ld_extra > 0: a column-sliced view of a
    wider buffer (row stride = columns + 2 * ld_extra, 16-B aligned start)."""
    s = (t.t() if kouter else t).contiguous().to(dev)
    if not ld_extra:
        return s
    wide = torch.full((s.shape[0], s.shape[1] + 2 * ld_extra), 7.0, dtype=BF, device=dev)
    wide[:, ld_extra:ld_extra + s.shape[1]] = s
    return wide[:, ld_extra:ld_extra + s.shape[1]]


def dims(a, b, ak, bk):
    M, K = (a.shape[-1], a.shape[-2]) if ak else (a.shape[-2], a.shape[-1])
    return M, (b.shape[-1] if bk else b.shape[-2]), K


# ---------------------------------------------------------------- routes
# (name, kind, parameter). tile: ops.gemm(tile=t) -> gemm_core.h gemm_kernel; w4: dtf_gemm_w4 with tile width bn; auto:
# the default dispatch (the 4-wave kernel for these shapes, by pick_w4); g256 / g256bn: the 8-wave kernel.
GENERIC = [("tile%d" % t, "tile", t) for t in (0, 1, 2, 3, 4, 5, 6)]
GLDS = [("tile%d" % t, "tile", t) for t in (7, 8, 9, 10, 15, 16)]
W4 = [("w4_128", "w4", 128), ("w4_256", "w4", 256), ("auto", "auto", 0)]
G256 = [("g256", "g256", 1), ("g256_split3", "g256", 3), ("g256_bn128", "g256bn", 128)]
ROUTES = GENERIC + GLDS + W4 + G256
IDS = [r[0] for r in ROUTES]


def launch(route, a, b, ak, bk, out):
    """Run C = A B^T on `route` into `out` (2-D, any row stride) and assert the launch counters name that kernel."""
    _, kind, p = route
    M, N, K = dims(a, b, ak, bk)
    f32 = int(out.dtype == F32)
    before = launch_counts()
    if kind in ("tile", "auto"):
        ops.gemm(a, b, a_kouter=ak, b_kouter=bk, out=out, tile=p if kind == "tile" else -1)
    elif kind == "w4":
        call("dtf_gemm_w4", ptr(a), ptr(b), ptr(out), M, N, K, a.stride(0), b.stride(0), out.stride(0), int(ak), int(bk),
             f32, p, stream())
    elif kind == "g256":
        ws = workspace(a.device)
        call("dtf_gemm256", ptr(a), ptr(b), ptr(out), M, N, K, a.stride(0), b.stride(0), out.stride(0), int(ak), int(bk),
             f32, p, ptr(ws), ws.numel(), stream())
    else:
        call("dtf_gemm256_bn", ptr(a), ptr(b), ptr(out), M, N, K, a.stride(0), b.stride(0), out.stride(0), int(ak),
             int(bk), f32, p, stream())
    d = launch_delta(before)
    gemms = {k: d[k] for k in ("w4_256", "w4_128", "gemm256", "gemm_tile")}
    want = dict.fromkeys(gemms, 0)
    if kind == "tile":
        want["gemm_tile"] = 1
    elif kind == "w4":
        want["w4_%d" % p] = 1
    elif kind in ("g256", "g256bn"):
        want["gemm256"] = 1
    if kind == "auto":
        assert d["w4_256"] + d["w4_128"] == 1 and d["gemm256"] == 0 and d["gemm_tile"] == 0, (route[0], d)
    else:
        assert gemms == want, (route[0], d)
    assert d["splitk"] == 0 and d["gemm_dact"] == 0 and d["beta_bf16"] == 0, (route[0], d)


def route_shapes(route):
    """(M, N, K, layouts) per route, by the alignment rules of gemm_impl and of each kernel's host checks."""
    _, kind, p = route
    kc_a = [(False, False), (False, True)]  # odd M: K-contiguous A only (a K-outer A needs M % 8 == 0)
    if kind == "tile" and p <= 6:
        return [(264, 136, 192, LAYOUTS), (8, 8, 64, LAYOUTS), (257, 264, 72, kc_a), (1, 8, 8, kc_a),
                (264, 132, 64, [(False, False), (True, False)])]  # N % 8 != 0: K-contiguous B only
    if kind == "tile":
        # LDS-DMA tiles (gemm_core.h GldsLoader / GldsKOuter): every (tile, layout) pair is instantiated by
        # launch_modes (glds_mode holds for OP_KCONTIG and OP_KOUTER), so none is left out; the shapes keep
        # pick_glds_tile's conditions (K-outer row counts % 8 == 0, operands < 2 GiB) and whole K-tiles
        return [(264, 136, 192, LAYOUTS), (8, 8, 64, LAYOUTS), (257, 264, 64, kc_a)]
    if kind in ("w4", "auto"):
        return [(264, 136, 192, LAYOUTS), (8, 8, 64, LAYOUTS), (257, 264, 64, kc_a), (1, 8, 64, kc_a)]
    if kind == "g256" and p == 3:
        return [(264, 136, 384, LAYOUTS)]  # 3 splits of 128: gemm256_try takes no split shorter than 2 K-tiles
    return [(264, 136, 192, LAYOUTS), (8, 8, 128, LAYOUTS), (257, 264, 128, kc_a)]


def out_dtypes(route):
    return [F32] if route[1] == "g256" and route[2] > 1 else [F32, BF]  # split-K writes f32 slabs


def ldc_for(route, N):
    return N if route[1] == "g256" and route[2] > 1 else N + 16  # (the split entry point needs ldc == N)


# ---------------------------------------------------------------- a. routes, exact
@pytest.mark.parametrize("route", ROUTES, ids=IDS)
def test_route_exact(cuda, route):
    for M, N, K, layouts in route_shapes(route):
        A, B, ref, _ = operands(M, N, K)
        for ak, bk in layouts:
            a, b = stored(A, ak, cuda), stored(B, bk, cuda)
            for dt in out_dtypes(route):
                if dt == BF and N % 8 and route[1] != "tile":
                    continue
                out, check = guarded_out(M, N, ldc_for(route, N), dt, device=cuda)
                launch(route, a, b, ak, bk, out)
                name = f"{route[0]} {M}x{N}x{K} ak={int(ak)} bk={int(bk)} {dt}"
                assert_exact(name, out, ref)
                check(name)


@pytest.mark.parametrize("route", ROUTES, ids=IDS)
def test_route_identity_asymmetric(cuda, route):
    """A = I (264 x 320), B[n, k] = (n K + k) % 251: C[m, n] = B[n, m] on the partial tiles too."""
    M, N, K = 264, 136, 384 if route[0] == "g256_split3" else 320
    A, B, ref, _ = operands(M, N, K, kind="eye")
    assert torch.equal(ref, B.double().t()[:M])
    for ak, bk in LAYOUTS:
        a, b = stored(A, ak, cuda), stored(B, bk, cuda)
        for dt in out_dtypes(route):
            out, check = guarded_out(M, N, ldc_for(route, N), dt, device=cuda)
            launch(route, a, b, ak, bk, out)
            assert_exact(f"{route[0]} identity ak={int(ak)} bk={int(bk)} {dt}", out, ref)
            check()


def test_n_not_multiple_of_8_leaves_the_4wave_kernel(cuda):
    """N = 132: the 4-wave kernel refuses a bf16 output (gemm_w4_ok: N % 8), so the default dispatch falls through
    tile256_try: to the generic kernel at K = 64 (gemm256_try needs 2 K-tiles), to the 8-wave kernel at K = 192 (its
    unstaged epilogue stores 8-B pieces, N % 4). An f32 output stays on the 4-wave kernel."""
    for K, key in ((64, "gemm_tile"), (192, "gemm256")):
        A, B, ref, _ = operands(264, 132, K)
        a, b = stored(A, False, cuda), stored(B, False, cuda)
        out, check = guarded_out(264, 132, 148, BF, device=cuda)
        before = launch_counts()
        ops.gemm(a, b, out=out)
        d = launch_delta(before)
        assert d[key] == 1 and d["w4_128"] + d["w4_256"] == 0, d
        assert_exact(f"N=132 K={K} bf16", out, ref)
        check()
        out, check = guarded_out(264, 132, 148, F32, device=cuda)
        before = launch_counts()
        ops.gemm(a, b, out=out)
        d = launch_delta(before)
        assert d["w4_128"] + d["w4_256"] == 1 and d["gemm_tile"] + d["gemm256"] == 0, d
        assert_exact(f"N=132 K={K} f32", out, ref)
        check()


# ---------------------------------------------------------------- b. epilogue on the 4-wave and the generic route
EPI_SHAPES = [(264, 136, 192), (8, 8, 64)]
EPI_ROUTES = [("w4", -1), ("generic", 0)]  # default dispatch (4-wave), forced 128x128 tile of the generic kernel


def epi_gemm(cuda, which, tile, a, b, **kw):
    """ops.gemm on the 4-wave (default dispatch) or the generic route; asserts the route."""
    before = launch_counts()
    out = ops.gemm(a, b, tile=tile, **kw)
    d = launch_delta(before)
    if which == "w4":
        assert d["w4_128"] + d["w4_256"] == 1 and d["gemm_tile"] + d["gemm256"] == 0, d
    else:
        assert d["gemm_tile"] == 1 and d["w4_128"] + d["w4_256"] + d["gemm256"] == 0, d
    assert d["splitk"] == 0, d
    return out, d


@pytest.mark.parametrize("which,tile", EPI_ROUTES, ids=["w4", "generic"])
@pytest.mark.parametrize("alpha", [0.5, -2.0])
def test_epilogue_alpha(cuda, which, tile, alpha):
    for M, N, K in EPI_SHAPES:
        A, B, prod, _ = operands(M, N, K)
        a, b = stored(A, False, cuda), stored(B, False, cuda)
        for dt in (F32, BF):
            out, check = guarded_out(M, N, N + 16, dt, device=cuda)
            epi_gemm(cuda, which, tile, a, b, out=out, alpha=alpha)
            assert_exact(f"alpha={alpha} {M}x{N}x{K} {dt}", out, alpha * prod)
            check()


@pytest.mark.parametrize("which,tile", EPI_ROUTES, ids=["w4", "generic"])
@pytest.mark.parametrize("beta", [1.0, 0.5, -1.0])
def test_epilogue_beta(cuda, which, tile, beta):
    for M, N, K in EPI_SHAPES:
        C0 = int_operand((M, N), -3, 3, 31)
        for dt in (F32, BF):
            # bf16: the staged epilogues round the product to bf16 before adding beta * C (see the module docstring):
            # operands in [-1, 1] keep the product (<= 192) a bf16 value, so one rounding remains, the reference's
            A, B, prod, _ = operands(M, N, K) if dt == F32 else operands(M, N, K, -1, 1)
            a, b = stored(A, False, cuda), stored(B, False, cuda)
            out, check = guarded_out(M, N, N + 16, dt, device=cuda)
            out.copy_(C0.to(cuda))
            _, d = epi_gemm(cuda, which, tile, a, b, out=out, beta=beta)
            assert d["beta_bf16"] == (1 if dt == BF else 0), d
            if dt == BF:
                assert torch.equal(bf16_round(prod), prod), "TEST BUG: the product must be a bf16 value here"
            assert_exact(f"beta={beta} {M}x{N}x{K} {dt}", out, prod + beta * C0.double(), beta=beta, partial=[prod])
            check()


@pytest.mark.parametrize("which,tile", EPI_ROUTES, ids=["w4", "generic"])
def test_epilogue_beta0_ignores_nan_output(cuda, which, tile):
    """beta == 0 must not read the old C: an output buffer full of NaN gives the exact finite product."""
    for M, N, K in EPI_SHAPES:
        A, B, prod, _ = operands(M, N, K)
        a, b = stored(A, False, cuda), stored(B, False, cuda)
        for dt in (F32, BF):
            out = torch.full((M, N), float("nan"), dtype=dt, device=cuda)
            epi_gemm(cuda, which, tile, a, b, out=out)
            assert_exact(f"beta=0 over NaN {M}x{N}x{K} {dt}", out, prod)


@pytest.mark.parametrize("which,tile", EPI_ROUTES, ids=["w4", "generic"])
def test_epilogue_bias_relu_aux(cuda, which, tile):
    for M, N, K in EPI_SHAPES:
        A, B, prod, _ = operands(M, N, K)
        a, b = stored(A, False, cuda), stored(B, False, cuda)
        bias = int_operand((N,), -3, 3, 41).float()
        pre, relu = gemm_f64(A, B, bias=bias, act="relu")
        out, check = guarded_out(M, N, N + 16, BF, device=cuda)
        epi_gemm(cuda, which, tile, a, b, out=out, bias=bias.to(cuda))
        assert_exact(f"bias {M}x{N}x{K}", out, pre)
        check()
        out, check = guarded_out(M, N, N + 16, BF, device=cuda)
        epi_gemm(cuda, which, tile, a, b, out=out, act=1)
        assert_exact(f"relu {M}x{N}x{K}", out, torch.relu(prod))
        check()
        # bias + ReLU with the pre-activation side output (same row stride as the output)
        out, check = guarded_out(M, N, N + 16, BF, device=cuda)
        aux, check_aux = guarded_out(M, N, N + 16, BF, device=cuda)
        epi_gemm(cuda, which, tile, a, b, out=out, bias=bias.to(cuda), act=1, aux=aux)
        assert_exact(f"bias+relu {M}x{N}x{K}", out, relu)
        assert_exact(f"aux {M}x{N}x{K}", aux, pre)  # (assert_exact compares a bf16 tensor with bf16_round(pre))
        check()
        check_aux("aux guard")


@pytest.mark.parametrize("which,tile", EPI_ROUTES, ids=["w4", "generic"])
def test_epilogue_bias_gelu(cuda, which, tile):
    """bias + GELU against the float64 tanh-GELU of the exact pre-activation. Per element |out - ref| <= 2^-8 |ref| +
    2^-22 |pre|: one bf16 ulp of the result, and four f32 ulps of the cancelling 1 + tanh factor (the device evaluates
    x * rcp(1 + exp(-2u)) in f32 with the fast exponential and reciprocal)."""
    for M, N, K in EPI_SHAPES:
        # operands in [-1, 1]: pre-activations of a few units, where GELU is neither 0 nor the identity
        A, B, _, _ = operands(M, N, K, -1, 1)
        a, b = stored(A, False, cuda), stored(B, False, cuda)
        bias = int_operand((N,), -3, 3, 41).float()
        pre, ref = gemm_f64(A, B, bias=bias, act="gelu")
        out, check = guarded_out(M, N, N + 16, BF, device=cuda)
        aux, check_aux = guarded_out(M, N, N + 16, BF, device=cuda)
        epi_gemm(cuda, which, tile, a, b, out=out, bias=bias.to(cuda), act=2, aux=aux)
        assert_exact(f"gelu aux {M}x{N}x{K}", aux, pre)
        got = out.double().cpu()
        assert torch.isfinite(got).all()
        bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * pre.abs()
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
        print(f"  gelu {which} {M}x{N}x{K}: worst err / bound {ratio:.3f}")
        WORST[f"gelu {which} {M}x{N}x{K}"] = ratio
        assert ratio <= 1.0, f"gelu {which} {M}x{N}x{K}: worst err / bound {ratio:.3f}"
        check()
        check_aux()


@pytest.mark.parametrize("M", [8, 72, 264])
@pytest.mark.parametrize("fused", [False, True], ids=["plain", "bias_relu"])
def test_epilogue_stats_generic(cuda, M, fused):
    """Column sums and sums of squares of the STORED bf16 values, accumulated into a non-zero stats vector; one partial
    row per 64-row tile (1, 2 and 5 of them). Operands in [-1, 1] keep the sums of squares below 2^24."""
    N, K = 136, 64
    A, B, _, _ = operands(M, N, K, -1, 1)
    a, b = stored(A, False, cuda), stored(B, False, cuda)
    bias = int_operand((N,), -3, 3, 41).float() if fused else None
    _, ref = gemm_f64(A, B, bias=bias, act="relu" if fused else None)
    y = bf16_round(ref)
    s0 = int_operand((2 * N,), -3, 3, 43).float()
    stats = s0.clone().to(cuda)
    before = launch_counts()
    out = ops.gemm(a, b, bias=None if bias is None else bias.to(cuda), act=1 if fused else 0, stats=stats)
    d = launch_delta(before)
    assert d["gemm_tile"] == 1 and d["w4_128"] + d["w4_256"] + d["gemm256"] + d["splitk"] == 0, d
    assert_exact(f"stats out M={M}", out, ref)
    want = s0.double() + torch.cat([y.sum(0), (y * y).sum(0)])
    assert_exact(f"stats M={M}", stats, want, partial=[(y * y).sum(0), y.abs().sum(0)])


# ---------------------------------------------------------------- c. strided and batched operands
@pytest.mark.parametrize("route", [r for r in ROUTES if r[0] in ("tile0", "tile8", "tile15", "auto", "g256")],
                         ids=["tile0", "tile8", "tile15", "auto", "g256"])
def test_strided_operands(cuda, route):
    """lda > K and ldb > N-or-K: operands are column slices of wider buffers (row strides % 8 == 0)."""
    M, N, K = 264, 136, 192
    A, B, ref, _ = operands(M, N, K)
    for ak, bk in LAYOUTS:
        a, b = stored(A, ak, cuda, ld_extra=8), stored(B, bk, cuda, ld_extra=16)
        assert a.stride(0) == a.shape[1] + 16 and b.stride(0) == b.shape[1] + 32
        for dt in (F32, BF):
            out, check = guarded_out(M, N, N + 16, dt, device=cuda)
            launch(route, a, b, ak, bk, out)
            assert_exact(f"strided {route[0]} ak={int(ak)} bk={int(bk)} {dt}", out, ref)
            check()


def batch_operands(nb, M, N, K):
    """Batch i draws from [-(i + 1), i + 1]: a swapped batch / slab order shows."""
    A = torch.stack([int_operand((M, K), -(i + 1), i + 1, 50 + i) for i in range(nb)])
    B = torch.stack([int_operand((N, K), -(i + 1), i + 1, 60 + i) for i in range(nb)])
    return A, B


@pytest.mark.parametrize("K,key", [(64, "w4"), (72, "gemm_tile")])
def test_batched(cuda, K, key):
    M, N = 72, 136
    A, B = batch_operands(3, M, N, K)
    for ak, bk in LAYOUTS:
        a = (A.transpose(1, 2) if ak else A).contiguous().to(cuda)
        b = (B.transpose(1, 2) if bk else B).contiguous().to(cuda)
        ref = gemm_f64(a, b, ak, bk)[1]
        for dt in (F32, BF):
            before = launch_counts()
            out = ops.gemm(a, b, a_kouter=ak, b_kouter=bk, out_dtype=dt)
            d = launch_delta(before)
            if key == "w4":
                assert d["w4_128"] + d["w4_256"] == 1 and d["gemm_tile"] == 0, d
            else:
                assert d["gemm_tile"] == 1 and d["w4_128"] + d["w4_256"] == 0, d
            assert d["splitk"] == 0, d
            assert_exact(f"batched K={K} ak={int(ak)} bk={int(bk)} {dt}", out, ref)
    # batch stride 0: one B shared by every batch entry
    a = A.contiguous().to(cuda)
    b = B[1].contiguous().to(cuda).expand(3, N, K)
    assert b.stride(0) == 0
    out = ops.gemm(a, b)
    assert_exact(f"batch stride 0 K={K}", out, gemm_f64(a, B[1].expand(3, N, K))[1])


def test_batched_splitk_slab_order(cuda):
    """f32 output, forced splitk = 3 over a batch of 3: the slabs are [batch][split]."""
    M, N, K = 72, 136, 192
    A, B = batch_operands(3, M, N, K)
    a, b = A.to(cuda), B.to(cuda)
    ref = gemm_f64(a, b)[1]
    C0 = torch.stack([int_operand((M, N), -3, 3, 70 + i) for i in range(3)])
    for beta in (0.0, 1.0):
        out = C0.float().to(cuda)
        before = launch_counts()
        ops.gemm(a, b, out=out, beta=beta, splitk=3)
        d = launch_delta(before)
        assert d["splitk"] == 1 and d["gemm_tile"] == 1, d
        assert_exact(f"batched split beta={beta}", out, ref + beta * C0.double(), beta=beta, partial=[ref])


# ---------------------------------------------------------------- d. split-K
SPLITS = [
    (64, 8, 8, 320),      # kchunk 64: 5 splits hold K, 3 are empty; dtf_sum_rows narrow branch (W = 512)
    (64, 64, 40, 2560),   # W = 4096, 40 slabs: one grouping pass
    (128, 160, 12, 768),  # W = 20480 (80 column blocks), 12 slabs: cascade
    (256, 256, 5, 320),   # W = 65536: float4 wide rows
    (256, 256, 72, 4608),  # wide rows with more than 64 slabs: cascade
    (64, 64, 3, 320),     # 3 does not divide the 5 K-tiles: splits of 128, 128, 64
]


@pytest.mark.parametrize("M,N,s,K", SPLITS)
def test_splitk_exact(cuda, M, N, s, K):
    A, B, ref, _ = operands(M, N, K)
    a, b = stored(A, False, cuda), stored(B, False, cuda)
    C0 = int_operand((M, N), -3, 3, 33)
    for beta in (0.0, 1.0):
        out = C0.float().to(cuda)
        before = launch_counts()
        ops.gemm(a, b, out=out, beta=beta, splitk=s)
        d = launch_delta(before)
        # (a forced split count on shapes this small stays on the generic kernel: gemm_impl re-plans for the 256-row
        # kernels only when they would fill most of the chip)
        assert d["splitk"] == 1 and d["gemm_tile"] == 1 and d["w4_128"] + d["w4_256"] + d["gemm256"] == 0, d
        assert_exact(f"splitk {M}x{N} s={s} K={K} beta={beta}", out, ref + beta * C0.double(), beta=beta, partial=[ref])


_BIG = {}


def big_case(cuda):
    """(2048, 1024, 4160), both operands K-outer: the one large shape (weight-gradient layout). The float64 reference
    is a float64 matmul on the device, exact for these integers."""
    if not _BIG:
        T, M, N = 4160, 2048, 1024
        dz, x = int_operand((T, M), -3, 3, 81).to(cuda), int_operand((T, N), -3, 3, 82).to(cuda)
        _BIG.update(dz=dz, x=x, ref=(dz.double().t() @ x.double()).cpu(), db=dz.double().sum(0).cpu())
    return _BIG


def test_splitk_automatic_plan(cuda):
    """plan_w4_split for (2048, 1024, 4160): 256x128 tiles (64 of them) x 4 splits fill the 256 CUs (score 0.8 - 0.09
    against 0.5 - 0.09 for 256x256); kchunk = 1088, so the splits are 1088, 1088, 1088, 896: uneven."""
    c = big_case(cuda)
    before = launch_counts()
    out = ops.gemm(c["dz"], c["x"], a_kouter=True, b_kouter=True, out_dtype=F32)
    d = launch_delta(before)
    assert d["splitk"] == 1 and d["w4_128"] == 1 and d["w4_256"] + d["gemm256"] + d["gemm_tile"] == 0, d
    assert_exact("automatic split", out, c["ref"])


# ---------------------------------------------------------------- e. fused weight + bias gradient
@pytest.mark.parametrize("T,M,N", [(64, 8, 8), (192, 264, 136), (4160, 2048, 1024)])
def test_wgrad_bias_exact(cuda, T, M, N):
    """dW += dZ^T X and db += column sums of dZ (dtf_gemm_wgrad_bias) against float64, accumulated into integers."""
    if T == 4160:
        c = big_case(cuda)
        dz, x, ref, dbref = c["dz"], c["x"], c["ref"], c["db"]
    else:
        dz, x = int_operand((T, M), -3, 3, 83).to(cuda), int_operand((T, N), -3, 3, 84).to(cuda)
        ref, dbref = gemm_f64(dz, x, True, True)[1], dz.double().sum(0).cpu()
    w0, b0 = int_operand((M, N), -3, 3, 85).float(), int_operand((M,), -3, 3, 86).float()
    dw, db = w0.to(cuda), b0.to(cuda)
    before = launch_counts()
    assert LA.dense_wgrad_bias(dz, x, dw, db)
    d = launch_delta(before)
    assert d["w4_128"] + d["w4_256"] == 1 and d["gemm_tile"] + d["gemm256"] == 0, d
    assert d["splitk"] == (1 if T == 4160 else 0), d
    assert_exact(f"dW T={T}", dw, ref + w0.double(), beta=1.0, partial=[ref])
    assert_exact(f"db T={T}", db, dbref + b0.double(), beta=1.0, partial=[dz.double().abs().sum(0).cpu()])


@pytest.mark.parametrize("T,M", [(72, 8), (64, 12)])
def test_wgrad_bias_refuses_and_leaves_outputs(cuda, T, M):
    """T % 64 != 0 or M % 8 != 0: the fused kernel cannot run; it must say so and touch nothing."""
    N = 8
    dz, x = int_operand((T, M), -3, 3, 83).to(cuda), int_operand((T, N), -3, 3, 84).to(cuda)
    dw = torch.full((M, N), SENTINEL, device=cuda)
    db = torch.full((M,), SENTINEL, device=cuda)
    before = launch_counts()
    assert LA.dense_wgrad_bias(dz, x, dw, db) is False
    d = launch_delta(before)
    assert all(v == 0 for v in d.values()), d
    torch.cuda.synchronize()
    assert bool((dw == SENTINEL).all()) and bool((db == SENTINEL).all())


# ---------------------------------------------------------------- f. data gradient with the activation backward fused
@pytest.mark.parametrize("K,key", [(192, "w4"), (72, "gemm_tile")])
@pytest.mark.parametrize("act", [1, 2], ids=["relu", "gelu"])
def test_gemm_dact(cuda, K, key, act):
    M, N = 264, 136
    A, B, prod, _ = operands(M, N, K)
    a, b = stored(A, False, cuda), stored(B, True, cuda)  # dZ [M, K], W [K, N] K-outer, as a data gradient reads it
    pre = int_operand((M, N), -2, 2, 91)
    pre.view(-1)[::7] = 0.0
    pre.view(-1)[3::11] = -0.0  # zeros and negative zeros
    assert (pre.view(torch.int16) == -32768).any() and (pre.view(torch.int16) == 0).any()
    pre_d = pre.to(cuda)
    out = torch.empty((M, N), dtype=BF, device=cuda)
    before = launch_counts()
    call("dtf_gemm_dact", ptr(a), ptr(b), ptr(out), ptr(pre_d), act, M, N, K, a.stride(0), b.stride(0), N, 0, 1, stream())
    d = launch_delta(before)
    assert d["gemm_dact"] == 1, d
    if key == "w4":
        assert d["w4_128"] + d["w4_256"] == 1 and d["gemm_tile"] + d["gemm256"] == 0, d
    else:
        assert d["gemm_tile"] == 1 and d["w4_128"] + d["w4_256"] + d["gemm256"] == 0, d
    # the unfused pair: GEMM, then the activation backward kernel
    p16 = ops.gemm(a, b, b_kouter=True)
    assert_exact("dact product", p16, prod)
    pair = torch.empty_like(p16)
    call("dtf_act", ptr(pre_d), ptr(p16), ptr(pair), pair.numel(), act, 1, stream())
    assert torch.equal(out.view(torch.int16), pair.view(torch.int16)), "fused and unfused differ bitwise"
    if act == 1:
        want = bf16_round(prod) * (pre.double() > 0)
        nz = pre.double() != 0
        assert torch.equal(out.double().cpu()[nz], want[nz])
        assert bool((out.double().cpu()[~nz] == 0).all())


# ---------------------------------------------------------------- g. padded path, ops.dense, ops.colsum
@pytest.mark.parametrize("M,N,K", [(3, 10, 7), (13, 24, 5)])
def test_padded_gemm(cuda, M, N, K):
    A, B, prod, _ = operands(M, N, K)
    bias = int_operand((N,), -3, 3, 41).float()
    C0 = int_operand((M, N), -3, 3, 31)
    for ak, bk in LAYOUTS:
        a, b = stored(A, ak, cuda), stored(B, bk, cuda)
        kw = dict(a_kouter=ak, b_kouter=bk)
        name = f"padded {M}x{N}x{K} ak={int(ak)} bk={int(bk)}"
        before = launch_counts()
        assert_exact(name + " alpha", ops.gemm(a, b, alpha=-2.0, out_dtype=F32, **kw), -2.0 * prod)
        d = launch_delta(before)
        assert d["gemm_tile"] == 1 and d["w4_128"] + d["w4_256"] + d["gemm256"] == 0, d
        pre, relu = gemm_f64(A, B, bias=bias, act="relu")
        aux = torch.full((M, N), SENTINEL, dtype=BF, device=cuda)
        assert_exact(name + " bias+relu", ops.gemm(a, b, bias=bias.to(cuda), act=1, aux=aux, **kw), relu)
        assert_exact(name + " aux", aux, pre)
        for dt in (F32, BF):
            out = C0.to(dt).to(cuda)
            ops.gemm(a, b, out=out, beta=1.0, **kw)
            assert_exact(name + f" out= beta=1 {dt}", out, prod + C0.double(), beta=1.0, partial=[prod])
        s0 = int_operand((2 * N,), -3, 3, 43).float()
        stats = s0.to(cuda)
        y = ops.gemm(a, b, stats=stats, **kw)
        assert_exact(name + " stats out", y, prod)
        yr = bf16_round(prod)
        assert_exact(name + " stats", stats, s0.double() + torch.cat([yr.sum(0), (yr * yr).sum(0)]))
    A3, B3 = batch_operands(3, M, N, K)
    assert_exact(f"padded batch {M}x{N}x{K}", ops.gemm(A3.to(cuda), B3.to(cuda), out_dtype=F32), gemm_f64(A3, B3)[1])


@pytest.mark.parametrize("T,nin,nout", [(5, 20, 12), (7, 64, 10)])
@pytest.mark.parametrize("act", [None, "relu", "gelu"])
def test_dense_unaligned_end_to_end(cuda, T, nin, nout, act):
    """ops.dense forward and backward (dx, dW, db) with unaligned sizes and a 3-D x against float64 autograd. Integer
    data: without an activation and with ReLU everything is exact (|values| <= 9 * 64 + 3 needs bf16 rounding of y and
    dx: compared with the rounded image). GELU: y within the bound of test_epilogue_bias_gelu; the gradients within
    what rounding dz = dy * gelu'(pre) to bf16 costs: REL * sum |dz| |w| with REL = 2^-8 (half a bf16 ulp, relative,
    at worst) + 2^-18 (the f32 evaluation of gelu' with the fast exponential: tens of f32 ulps), plus half a bf16 ulp
    of a bf16 result."""
    lo = 1 if act == "gelu" else 3
    x = int_operand((2, T, nin), -lo, lo, 101)
    w = int_operand((nout, nin), -lo, lo, 102).float()
    b = int_operand((nout,), -3, 3, 103).float()
    dy = int_operand((2, T, nout), -3, 3, 104)
    xd = x.double().requires_grad_(True)
    wd, bd = w.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = xd @ wd.t() + bd
    yref = pre if act is None else torch.relu(pre) if act == "relu" else gelu_f64(pre)
    dxr, dwr, dbr = torch.autograd.grad(yref, [xd, wd, bd], dy.double())
    xg = x.to(cuda).requires_grad_(True)
    wg, bg = w.to(cuda).requires_grad_(True), b.to(cuda).requires_grad_(True)
    before = launch_counts()
    y = ops.dense(xg, wg, bg, act=act)
    d = launch_delta(before)
    assert d["gemm_tile"] == 1, d
    assert y.shape == (2, T, nout) and y.dtype == BF
    y.backward(dy.to(cuda))
    name = f"dense {T}x{nin}x{nout} {act}"
    if act != "gelu":
        assert_exact(name + " y", y, yref.detach())
        assert_exact(name + " dx", xg.grad, dxr)
        assert_exact(name + " dW", wg.grad, dwr)
        assert_exact(name + " db", bg.grad, dbr)
        return
    pre, yref = pre.detach(), yref.detach()

    def within(what, got, ref, bound):
        err = (got.double().cpu() - ref).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
        print(f"  {name} {what}: worst err / bound {r:.3f}")
        assert r <= 1.0, f"{name} {what}: worst err / bound {r:.3f}"

    within("y", y, yref, 2.0 ** -8 * yref.abs() + 2.0 ** -22 * pre.abs())
    k0 = 0.7978845608028654
    t = torch.tanh(k0 * (pre + 0.044715 * pre ** 3))
    dz = (dy.double() * (0.5 * (1 + t) + 0.5 * pre * (1 - t * t) * k0 * (1 + 3 * 0.044715 * pre ** 2))).abs()
    REL = 2.0 ** -8 + 2.0 ** -18
    sx = REL * (dz @ w.double().abs())
    within("dx", xg.grad, dxr, sx + bf16_half_ulp(dxr.abs() + sx))
    within("dW", wg.grad, dwr, REL * torch.einsum("bto,bti->oi", dz, x.double().abs()))
    within("db", bg.grad, dbr, REL * dz.sum((0, 1)))


@pytest.mark.parametrize("M", [1, 7, 300])
@pytest.mark.parametrize("N", [8, 264, 12])
def test_colsum_exact(cuda, M, N):
    """Column sums of a bf16 matrix into f32 (N = 12: the N % 8 fallback), with and without accumulate."""
    x = int_operand((M, N), -3, 3, 111)
    ref = x.double().sum(0)
    xd = x.to(cuda)
    assert_exact(f"colsum {M}x{N}", ops.colsum(xd), ref)
    o0 = int_operand((N,), -3, 3, 112).float()
    out = o0.to(cuda)
    ops.colsum(xd, out=out, accumulate=True)
    assert_exact(f"colsum accumulate {M}x{N}", out, ref + o0.double(), beta=1.0, partial=[x.double().abs().sum(0)])
    out = torch.full((N,), float("nan"), device=cuda)
    ops.colsum(xd, out=out)
    assert_exact(f"colsum overwrite {M}x{N}", out, ref)


# ---------------------------------------------------------------- h. random-normal data: what the routes cost
@pytest.mark.parametrize("route", ROUTES, ids=IDS)
def test_route_random_normal(cuda, route):
    M, N, K = 264, 136, 384 if route[0] == "g256_split3" else 192
    A, B, ref, S = operands(M, N, K, kind="randn")
    a, b = stored(A, False, cuda), stored(B, False, cuda)
    for dt in out_dtypes(route):
        out, check = guarded_out(M, N, ldc_for(route, N), dt, device=cuda)
        launch(route, a, b, False, False, out)
        check_elems(f"{route[0]} {'bf16' if dt == BF else 'f32'}", out, ref, S, K, bf16_out=dt == BF, worst=WORST)
        check()


@pytest.mark.parametrize("s", [8, 40])
def test_splitk_random_normal(cuda, s):
    M, N, K = 264, 136, 2560
    A, B, ref, S = operands(M, N, K, kind="randn")
    a, b = stored(A, False, cuda), stored(B, False, cuda)
    before = launch_counts()
    out = ops.gemm(a, b, out_dtype=F32, splitk=s)
    d = launch_delta(before)
    assert d["splitk"] == 1 and d["gemm_tile"] == 1, d
    check_elems(f"splitk s={s} f32", out, ref, S, K, worst=WORST)
