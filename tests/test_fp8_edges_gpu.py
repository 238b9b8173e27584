"""The fp8 quantizers (gemm_fp8.hip dtf_quant_fp8 / dtf_quant_fp8_exact / dtf_quant_fp8_t2, the q8 epilogues of
gemm256.hip and gemm_w4_fp8.hip) byte for byte against the references of tests/_fp8ref.py, and the scale bookkeeping
around them (amax slots, delayed and exact scales, the scale-update kernels, refusals, the non-finite policy).

Scales are powers of two, so 1 / scale is exact whatever the division does, and every byte must equal the reference's;
one case per producer uses 0.05, where the kernel's 1 / scale may differ from the reference's in the last bit: there a
byte may also be the adjacent code, and the count of those is printed.

Shapes are the smallest that reach each code path. dtf_quant_fp8 walks 8-element chunks, 4 per thread and trip, on a
grid capped at 2048 blocks of 256 threads: 1 chunk, 1024 (main loop only), 1024 + 259 (main loop + a partial tail trip)
and 2048 * 256 * 5 + 5 (capped grid, several trips, tail). The transposing quantizer works on 64-column x 256-row
strips of 64-row tiles: (64, 64), (320, 128) (one full strip + a 64-row one) and (512, 192).

Non-finite policy (asserted here for every producer): a NaN value is stored as a NaN code in q and at the transposed
position of qT and no other byte changes; +-inf saturates to +-FMAX; amax is the maximum over the non-NaN values (inf is
recorded as inf); the column-sum partial of a column holding a NaN is NaN.
"""
import pytest
import torch

from distributed_tensorflow_amd.ops import fp8
from distributed_tensorflow_amd.ops._util import K, launch_counts, launch_delta, ptr, stream, workspace

from _fp8ref import (BF16, FMAX, GELU_SHARE_CAP, TOP, assert_bytes, count_adjacent, decode, draw_ints, fp8_int_operand,
                     gelu_band, gelu_case, is_nan_code, quant_ref, sweep_fill, sweep_values)

pytestmark = pytest.mark.gpu

F32 = torch.float32
U8 = torch.uint8
FILL = 0xA5  # sentinel byte of output buffers (a finite code of both formats that the small sweeps also produce: the
#              checks compare whole buffers, never search for it)
POW2 = [2.0 ** -3, 1.0, 2.0 ** 5]
NONPOW2 = 0.05
ADJ = {}  # adjacent-code counts of the 0.05-scale and GELU cases, printed per test


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def f32(v, dev):
    return torch.tensor([v], dtype=F32, device=dev)


def same_bits(t, v):
    """The f32 tensor element t holds exactly the float v (bit for bit; inf included, -0 != 0)."""
    return t.detach().cpu().view(torch.int32).item() == torch.tensor([v], dtype=F32).view(torch.int32).item()


# ---------------------------------------------------------------- producers
def run_quant(x, scale, amax=None, zero_amax=0, guard=64):
    """dtf_quant_fp8 on a flat bf16 tensor into a sentinel-filled buffer with `guard` bytes after n."""
    n = x.numel()
    buf = torch.full((n + guard,), FILL, dtype=U8, device=x.device)
    rc = K().dtf_quant_fp8(ptr(x), ptr(buf), n, ptr(scale), ptr(amax), zero_amax, stream())
    torch.cuda.synchronize()
    return rc, buf[:n].cpu(), buf[n:].cpu()


def run_exact(x, guard=64):
    n = x.numel()
    buf = torch.full((n + guard,), FILL, dtype=U8, device=x.device)
    so = torch.full((1,), -1.0, dtype=F32, device=x.device)
    rc = K().dtf_quant_fp8_exact(ptr(x), ptr(buf), n, ptr(so), ptr(workspace(x.device)), stream())
    torch.cuda.synchronize()
    return rc, buf[:n].cpu(), buf[n:].cpu(), so


def run_t2(x, scale=None, *, fmt=0, pre=None, act=0, exact_out=None, amax=None, colsums=False, amax_prev=None,
           scale_used=None, scale_used2=None):
    q, qT, cp = fp8.quantize_t(x, scale, amax, fmt=fmt, pre=pre, act=act, colsums=colsums, exact_out=exact_out,
                               amax_prev=amax_prev, scale_used=scale_used, scale_used2=scale_used2)
    torch.cuda.synchronize()
    return q.cpu(), qT.cpu(), None if cp is None else cp.cpu()


def check_t2(name, q, qT, ref, fmt):
    assert_bytes(name + " q", q, ref, fmt)
    assert torch.equal(qT, q.t().contiguous()), name + ": qT != q.t()"


def check_ties(name, q, ti, tc):
    got = q.reshape(-1)[ti]
    bad = torch.nonzero(got != tc)
    assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} of {ti.numel()} midpoints off the even code; first: got "
                               f"0x{got[bad[0]].item():02X}, expected 0x{tc[bad[0]].item():02X}")


# ---------------------------------------------------------------- dtf_quant_fp8
QUANT_N8 = [1, 1024, 1024 + 259]


@pytest.mark.parametrize("scale", POW2)
@pytest.mark.parametrize("n8", QUANT_N8)
def test_quant_fp8_sweep(cuda, n8, scale):
    """Every code, every tie and its bf16 neighbours, +-0, saturation and +-inf through each loop of the kernel."""
    n = 8 * n8
    if n8 == 1:  # 8 values of the sweep: ties of both signs, FMAX, beyond it, -inf
        sv, ti, tc = sweep_values(0, scale)
        pick = torch.tensor([int(ti[0]), int(ti[1]), int(ti[-1]), int(ti[-2]), TOP[0], sv.numel() - 6, sv.numel() - 3,
                             sv.numel() - 1])
        x, ti, tc = sv[pick].contiguous(), torch.arange(4), tc[[0, 1, -1, -2]]
    else:
        x, ti, tc = sweep_fill((n,), 0, scale)
    amax = f32(0.0, cuda)
    rc, q, guard = run_quant(x.to(cuda), f32(scale, cuda), amax)
    assert rc == 0
    assert_bytes("quant_fp8", q, quant_ref(x, scale, 0), 0)
    check_ties("quant_fp8", q, ti, tc)
    assert (guard == FILL).all(), "stores past n"
    assert same_bits(amax, x.float().abs().max().item())  # (inf once the sweep's +-inf are inside)


def test_quant_fp8_capped_grid(cuda):
    """2048 * 256 * 5 + 5 chunks: the capped grid takes several main-loop trips and a tail."""
    n = 8 * (2048 * 256 * 4 + 2048 * 256 + 5)
    x, ti, tc = sweep_fill((n,), 0, 1.0, overflow=False)
    amax = f32(0.0, cuda)
    rc, q, guard = run_quant(x.to(cuda), f32(1.0, cuda), amax)
    assert rc == 0
    assert_bytes("quant_fp8 capped", q, quant_ref(x, 1.0, 0), 0)
    assert (guard == FILL).all(), "stores past n"
    assert same_bits(amax, 448.0)


def test_quant_fp8_refuses_partial_chunk(cuda):
    x = torch.ones(16, dtype=BF16, device=cuda)
    amax = f32(3.0, cuda)
    rc, q, guard = run_quant(x[:12], f32(1.0, cuda), amax, zero_amax=1)
    assert rc == -1
    assert (q == FILL).all() and (guard == FILL).all() and same_bits(amax, 3.0)
    rc, q, guard, so = run_exact(x[:12])
    assert rc == -1 and (q == FILL).all() and (guard == FILL).all() and same_bits(so, -1.0)


def test_quant_fp8_amax_slot(cuda):
    """amax == max |v| bit for bit; a larger value in the slot survives, a smaller one is raised, zero_amax clears."""
    x = (draw_ints((8 * 1283,), 3) * 0.375).to(BF16)  # max |x| = 3.0
    xd, s = x.to(cuda), f32(1.0, cuda)
    for start, zero, want in ((0.0, 0, 3.0), (5.5, 0, 5.5), (1.25, 0, 3.0), (5.5, 1, 3.0)):
        amax = f32(start, cuda)
        rc, q, _ = run_quant(xd, s, amax, zero_amax=zero)
        assert rc == 0 and same_bits(amax, want), (start, zero, amax.item())
    assert_bytes("quant_fp8 ints", q, quant_ref(x, 1.0, 0), 0)


def test_quant_fp8_scale_floor(cuda):
    """scale[0] = 0 quantizes with the 1e-30 floor: {0, +-1} -> {0, +-FMAX}, no NaN."""
    x = torch.tensor([0.0, 1.0, -1.0, 0.0, 1.0, -1.0, -1.0, 1.0] * 4, dtype=BF16)
    rc, q, _ = run_quant(x.to(cuda), f32(0.0, cuda))
    assert rc == 0
    assert torch.equal(decode(q, 0), x.double() * 448.0)
    assert_bytes("floor", q, quant_ref(x, 0.0, 0), 0)
    qt, qT, _ = run_t2(x.repeat(128).reshape(64, 64).to(cuda), f32(0.0, cuda), fmt=1)
    assert torch.equal(decode(qt, 1), x.repeat(128).reshape(64, 64).double() * 57344.0)


@pytest.mark.parametrize("producer", ["quant", "exact", "t2-e4m3", "t2-e5m2", "t2-exact"])
def test_nonpow2_scale_adjacent_codes(cuda, producer):
    """Scale 0.05 (exact producers: max |x| / FMAX of random data): 1 / scale is rounded, and the kernel's quotient
    may differ from the reference's in the last bit, so a value next to a rounding boundary may take the adjacent
    code. Nothing further off is accepted; the count is printed."""
    g = torch.Generator().manual_seed(17)
    fmt = 1 if producer == "t2-e5m2" else 0
    x = (torch.randn(320, 128, generator=g) * (0.3 * FMAX[fmt] * NONPOW2)).to(BF16)  # saturates a few per mille
    xd = x.to(cuda)
    if producer == "quant":
        rc, q, _ = run_quant(xd.view(-1), f32(NONPOW2, cuda))
        assert rc == 0
        ref = quant_ref(x.view(-1), NONPOW2, fmt)
    elif producer == "exact":
        rc, q, _, so = run_exact(xd.view(-1))
        assert rc == 0
        ref = quant_ref(x.view(-1), so.cpu(), fmt, floor=0.0)
    elif producer == "t2-exact":
        so = f32(-1.0, cuda)
        q, qT, _ = run_t2(xd, exact_out=so)
        assert torch.equal(qT, q.t().contiguous())
        ref = quant_ref(x, so.cpu(), fmt, floor=0.0)
    else:
        q, qT, _ = run_t2(xd, f32(NONPOW2, cuda), fmt=fmt)
        assert torch.equal(qT, q.t().contiguous())
        ref = quant_ref(x, NONPOW2, fmt)
    if "exact" in producer:  # the published scale is max |x| / FMAX to the last bit or the one next to it
        want = x.float().abs().max() / torch.tensor(FMAX[fmt], dtype=F32)
        assert abs(so.item() - want.item()) <= 2.0 ** -23 * want.item(), (so.item(), want.item())
    ADJ[producer] = count_adjacent(producer, q, ref, fmt)
    print(f"  {producer}: {ADJ[producer]} of {q.numel()} bytes on the adjacent code")
    # a last-bit difference of 1 / scale moves a value by 2^-23 of itself, a code step is 2^-4 of it or more: a share
    # of the order of 2^-19 of the values can change code
    assert ADJ[producer] <= 0.001 * q.numel()


# ---------------------------------------------------------------- dtf_quant_fp8_exact
@pytest.mark.parametrize("k", [-3, 0, 5])
def test_quant_fp8_exact_scale(cuda, k):
    """max |x| = FMAX * 2^k: scale_out == 2^k bit for bit and the bytes equal the reference, ties included."""
    x, ti, tc = sweep_fill((8 * 1283,), 0, 2.0 ** k, overflow=False)
    rc, q, guard, so = run_exact(x.to(cuda))
    assert rc == 0 and same_bits(so, 2.0 ** k), so.item()
    assert_bytes("exact", q, quant_ref(x, 2.0 ** k, 0), 0)
    check_ties("exact", q, ti, tc)
    assert (guard == FILL).all()


def test_exact_scale_of_zeros(cuda):
    """An all-zero tensor: all-zero bytes, a finite positive scale (the 1e-12 floor over FMAX), no NaN."""
    z = torch.zeros(64 * 64, dtype=BF16, device=cuda)
    rc, q, _, so = run_exact(z)
    assert rc == 0 and (q == 0).all()
    assert 0 < so.item() < float("inf") and abs(so.item() - 1e-12 / 448.0) <= 2.0 ** -22 * 1e-12 / 448.0
    for fmt in (0, 1):
        so = f32(-1.0, cuda)
        q, qT, _ = fp8.quantize_t(z.view(64, 64), fmt=fmt, exact_out=so)
        torch.cuda.synchronize()
        assert (q == 0).all() and (qT == 0).all() and 0 < so.item() < float("inf")


# ---------------------------------------------------------------- dtf_quant_fp8_t2
T2_SHAPES = [(64, 64), (320, 128), (512, 192)]


@pytest.mark.parametrize("scale", POW2)
@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("M,N", T2_SHAPES)
def test_quant_t2_sweep(cuda, M, N, fmt, scale):
    x, ti, tc = sweep_fill((M, N), fmt, scale)
    amax = f32(0.0, cuda)
    q, qT, _ = run_t2(x.to(cuda), f32(scale, cuda), fmt=fmt, amax=amax)
    check_t2("t2", q, qT, quant_ref(x, scale, fmt), fmt)
    check_ties("t2", q, ti, tc)
    assert same_bits(amax, float("inf"))  # the sweep holds +-inf: recorded as inf


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("M,N", T2_SHAPES)
def test_quant_t2_relu_mask(cuda, M, N, fmt):
    """pre / act = 1: the value is dy where pre > 0 and (signed) zero elsewhere; exact, ties included."""
    scale = 2.0 ** -3
    x, ti, tc = sweep_fill((M, N), fmt, scale, overflow=False)
    g = torch.Generator().manual_seed(5)
    pre = torch.randn(M, N, generator=g).to(BF16)
    pre.view(-1)[ti] = 1.0  # the ties pass the mask
    pre[0, 0], pre[0, 1] = 0.0, -0.0  # not > 0: masked
    v = x.float() * (pre.float() > 0).float()
    amax = f32(0.0, cuda)
    q, qT, _ = run_t2(x.to(cuda), f32(scale, cuda), fmt=fmt, pre=pre.to(cuda), act=1, amax=amax)
    check_t2("t2 relu", q, qT, quant_ref(v, scale, fmt), fmt)
    check_ties("t2 relu", q, ti, tc)
    assert same_bits(amax, v.abs().max().item())


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("M,N", T2_SHAPES[1:])
def test_quant_t2_column_sum_partials(cuda, M, N, masked):
    """Integer values: each row of the [ceil(M / 256), N] partial buffer is the exact sum of its own 256 rows."""
    x = draw_ints((M, N), 9).to(BF16)
    pre = (draw_ints((M, N), 10) - 2).to(BF16) if masked else None
    v = x.double() * (pre.double() > 0).double() if masked else x.double()
    q, qT, cp = run_t2(x.to(cuda), f32(1.0, cuda), fmt=1, pre=None if pre is None else pre.to(cuda),
                       act=1 if masked else 0, colsums=True)
    nstrip = -(-M // 256)
    assert cp.shape == (nstrip, N)
    for s in range(nstrip):
        want = v[256 * s:256 * (s + 1)].sum(0)
        assert torch.equal(cp[s].double(), want), f"strip {s}: column sums differ"
    check_t2("t2 ints", q, qT, quant_ref(v.float(), 1.0, 1), 1)


def test_quant_t2_amax_slot(cuda):
    x = (draw_ints((320, 128), 4) * 0.375).to(BF16)  # max |x| = 3.0
    xd = x.to(cuda)
    for start, want in ((0.0, 3.0), (5.5, 5.5), (1.25, 3.0)):
        amax = f32(start, cuda)
        run_t2(xd, f32(1.0, cuda), amax=amax)
        assert same_bits(amax, want), (start, amax.item())


@pytest.mark.parametrize("fmt", [0, 1])
def test_quant_t2_delayed_scale(cuda, fmt):
    """amax_prev = FMAX * 2^k: scale 2^k, published to scale_used and scale_used2 (the *scale operand is ignored);
    amax_prev = 0: *scale is used and published."""
    k = -2
    x, ti, tc = sweep_fill((320, 128), fmt, 2.0 ** k)
    xd = x.to(cuda)
    used, used2 = f32(-1.0, cuda), f32(-1.0, cuda)
    q, qT, _ = run_t2(xd, f32(7.0, cuda), fmt=fmt, amax_prev=f32(FMAX[fmt] * 2.0 ** k, cuda), scale_used=used,
                      scale_used2=used2)
    assert same_bits(used, 2.0 ** k) and same_bits(used2, 2.0 ** k)
    check_t2("delayed", q, qT, quant_ref(x, 2.0 ** k, fmt), fmt)
    check_ties("delayed", q, ti, tc)
    used, used2 = f32(-1.0, cuda), f32(-1.0, cuda)
    q, qT, _ = run_t2(xd, f32(2.0 ** k, cuda), fmt=fmt, amax_prev=f32(0.0, cuda), scale_used=used, scale_used2=used2)
    assert same_bits(used, 2.0 ** k) and same_bits(used2, 2.0 ** k)
    check_t2("fallback", q, qT, quant_ref(x, 2.0 ** k, fmt), fmt)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("k", [-3, 5])
def test_quant_t2_exact_scale(cuda, fmt, k):
    x, ti, tc = sweep_fill((320, 128), fmt, 2.0 ** k, overflow=False)
    so, amax = f32(-1.0, cuda), f32(0.0, cuda)
    q, qT, _ = run_t2(x.to(cuda), fmt=fmt, exact_out=so, amax=amax)
    assert same_bits(so, 2.0 ** k), so.item()
    check_t2("t2 exact", q, qT, quant_ref(x, 2.0 ** k, fmt), fmt)
    check_ties("t2 exact", q, ti, tc)
    assert same_bits(amax, FMAX[fmt] * 2.0 ** k)


@pytest.mark.parametrize("M,N", [(96, 64), (64, 32)])
def test_quant_t2_refuses_partial_tiles(cuda, M, N):
    x = torch.ones(M, N, dtype=BF16, device=cuda)
    q = torch.full((M, N), FILL, dtype=U8, device=cuda)
    qT = torch.full((N, M), FILL, dtype=U8, device=cuda)
    cp = torch.full((1, N), -7.0, dtype=F32, device=cuda)
    slots = torch.tensor([1.0, 2.0, 0.0, -1.0, -1.0], device=cuda)  # scale, amax, amax_prev, used, used2
    rc = K().dtf_quant_fp8_t2(ptr(x), None, 0, ptr(q), ptr(qT), ptr(cp), ptr(slots[0:1]), ptr(slots[1:2]), M, N, 0, 0,
                              None, None, ptr(slots[2:3]), ptr(slots[3:4]), ptr(slots[4:5]), stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert (q == FILL).all() and (qT == FILL).all() and (cp == -7.0).all()
    assert slots.tolist() == [1.0, 2.0, 0.0, -1.0, -1.0]


def test_quant_t2_gelu_backward(cuda):
    """act = 2: dy * gelu'(pre) with __expf and a hardware reciprocal, so not bit exact. Against the float64 value,
    quantized: the kernel's byte is the reference's, or, only where quantizing ref -+ 2^-12 |dy| gives another byte,
    that byte (see _fp8ref.gelu_band for the size of the band; test_fp8_refs.py bounds its share for this data)."""
    fmt, scale = 1, 2.0 ** -13
    dy, pre = gelu_case((320, 128), 11)
    ref, lo, hi, v = gelu_band(dy, pre, scale, fmt)
    amax = f32(0.0, cuda)
    q, qT, cp = run_t2(dy.to(cuda), f32(scale, cuda), fmt=fmt, pre=pre.to(cuda), act=2, amax=amax, colsums=True)
    assert torch.equal(qT, q.t().contiguous())
    count_adjacent("gelu", q, ref, fmt)
    diff = q != ref
    outside = diff & (q != lo) & (q != hi)
    ADJ["gelu"] = int(diff.sum())
    print(f"  gelu: {ADJ['gelu']} of {q.numel()} bytes differ from the float64 reference, all inside the band: "
          f"{not outside.any().item()}")
    assert not outside.any(), f"{int(outside.sum())} bytes differ outside the 2^-12 |dy| band"
    assert diff.double().mean().item() <= GELU_SHARE_CAP
    # amax and the column sums of the same values, to f32 accuracy of their own terms
    assert abs(amax.item() - v.abs().max().item()) <= 2.0 ** -12 * dy.double().abs().max().item()
    for s in range(2):
        rows = slice(256 * s, 256 * (s + 1))
        err = (cp[s].double() - v[rows].sum(0)).abs()
        assert (err <= 2.0 ** -12 * dy[rows].double().abs().sum(0)).all()


# ---------------------------------------------------------------- scale-update kernels
def test_update_scale_kernels(cuda):
    """scale = amax / fmax * 2^margin, amax reset; amax = 0: 1.0 (first kernel) or the old scale (second); prev
    receives the old scale. Powers of two times fmax: every expected value is exact."""
    for amax0, margin, want in ((448.0 * 2.0 ** -4, 0.0, 2.0 ** -4), (448.0 * 8, 1.0, 16.0), (448.0 * 8, -2.0, 2.0),
                                (0.0, 0.0, 1.0)):
        amax, scale = f32(amax0, cuda), f32(0.3, cuda)
        assert K().dtf_fp8_update_scale(ptr(amax), ptr(scale), margin, stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(scale, want) and same_bits(amax, 0.0), (amax0, margin, scale.item())
    for fmax in (448.0, 57344.0):
        for amax0, margin, want in ((fmax * 2.0 ** -4, 0.0, 2.0 ** -4), (fmax * 8, 1.0, 16.0), (fmax * 8, -2.0, 2.0),
                                    (0.0, 0.0, 0.375)):
            for with_prev in (True, False):
                amax, scale, prev = f32(amax0, cuda), f32(0.375, cuda), f32(-1.0, cuda)
                rc = K().dtf_fp8_update_scale2(ptr(amax), ptr(scale), ptr(prev) if with_prev else None, fmax, margin,
                                               stream())
                torch.cuda.synchronize()
                assert rc == 0 and same_bits(scale, want) and same_bits(amax, 0.0), (fmax, amax0, margin, scale.item())
                assert same_bits(prev, 0.375 if with_prev else -1.0)


# ---------------------------------------------------------------- non-finite policy
NAN_POS = [(0, 5), (319, 77), (100, 127)]  # first row, last row of the partial strip, last column
NAN_IDS = ["first-row", "last-strip-row", "last-column"]
SEEN = {}  # the byte each producer stored for a NaN, printed


def nan_input(pos, fmt):
    """Integers of [-8, 8] times FMAX / 8 (max |x| = FMAX: with scale 1, which the exact-scale mode also arrives at,
    every value is a code and every sum is exact), one NaN at `pos`."""
    x = (draw_ints((320, 128), 21) * (FMAX[fmt] / 8)).to(BF16)
    clean = x.clone()
    x[pos] = float("nan")
    return x, clean


def check_nan_bytes(name, q, ref, pos, fmt, qT=None):
    b = q[pos].item()
    SEEN[name] = b
    print(f"  {name}: NaN stored as 0x{b:02X}")
    assert is_nan_code(q[pos], fmt).item(), f"{name}: NaN stored as 0x{b:02X}, not a NaN code"
    assert_bytes(name, q, ref, fmt)  # every other byte as without the NaN
    assert int(is_nan_code(q, fmt).sum()) == 1
    if qT is not None:
        assert torch.equal(qT, q.t().contiguous()), name + ": qT != q.t()"


@pytest.mark.parametrize("pos", NAN_POS, ids=NAN_IDS)
def test_nan_through_flat_quantizers(cuda, pos):
    x, clean = nan_input(pos, 0)
    ref = quant_ref(x, 1.0, 0)
    assert torch.equal(ref[~torch.isnan(x)], quant_ref(clean, 1.0, 0)[~torch.isnan(x)])
    amax = f32(0.0, cuda)
    rc, q, _ = run_quant(x.to(cuda).view(-1), f32(1.0, cuda), amax)
    assert rc == 0
    check_nan_bytes("quant_fp8", q.view(320, 128), ref, pos, 0)
    assert same_bits(amax, 448.0)  # the maximum over the non-NaN values
    rc, q, _, so = run_exact(x.to(cuda).view(-1))
    assert rc == 0 and same_bits(so, 1.0)  # the scale comes from the non-NaN values
    check_nan_bytes("quant_fp8_exact", q.view(320, 128), ref, pos, 0)


@pytest.mark.parametrize("fmt", [0, 1])
@pytest.mark.parametrize("pos", NAN_POS, ids=NAN_IDS)
def test_nan_through_transposing_quantizer(cuda, pos, fmt):
    x, clean = nan_input(pos, fmt)
    amax = f32(0.0, cuda)
    q, qT, cp = run_t2(x.to(cuda), f32(1.0, cuda), fmt=fmt, amax=amax, colsums=True)
    check_nan_bytes(f"quant_t2 fmt {fmt}", q, quant_ref(x, 1.0, fmt), pos, fmt, qT)
    assert same_bits(amax, FMAX[fmt])
    strip, col = pos[0] // 256, pos[1]
    want = torch.stack([clean[:256].double().sum(0), clean[256:].double().sum(0)])
    assert torch.isnan(cp[strip, col]) and int(torch.isnan(cp).sum()) == 1
    keep = ~torch.isnan(cp)
    assert torch.equal(cp[keep].double(), want[keep])
    # exact-scale mode: the scale comes from the non-NaN values
    so = f32(-1.0, cuda)
    q, qT, _ = run_t2(x.to(cuda), fmt=fmt, exact_out=so)
    assert same_bits(so, 1.0)
    check_nan_bytes(f"quant_t2 exact fmt {fmt}", q, quant_ref(x, 1.0, fmt), pos, fmt, qT)


@pytest.mark.parametrize("act", [1, 2])
@pytest.mark.parametrize("pos", NAN_POS, ids=NAN_IDS)
def test_nan_after_folded_activation_backward(cuda, pos, act):
    """The NaN sits in the pre-activation (GELU: gelu'(NaN) is NaN) or is an inf gradient times a ReLU mask of 0."""
    x = (draw_ints((320, 128), 22) * 0.5).to(BF16)
    pre = torch.ones(320, 128, dtype=BF16)  # gelu'(1) = 1.083: every other element keeps its sign and rough size
    if act == 2:
        pre[pos] = float("nan")
    else:
        x[pos], pre[pos] = float("inf"), -1.0
    amax = f32(0.0, cuda)
    q, qT, cp = run_t2(x.to(cuda), f32(0.125, cuda), fmt=1, pre=pre.to(cuda), act=act, amax=amax, colsums=True)
    name = f"quant_t2 act {act}"
    SEEN[name] = q[pos].item()
    print(f"  {name}: NaN stored as 0x{q[pos].item():02X}")
    assert is_nan_code(q[pos], 1).item(), f"{name}: NaN stored as 0x{q[pos].item():02X}"
    assert int(is_nan_code(q, 1).sum()) == 1 and torch.equal(qT, q.t().contiguous())
    if act == 1:
        v = x.float()
        v[pos] = float("nan")
        assert_bytes(name, q, quant_ref(v, 0.125, 1), 1)
        assert same_bits(amax, 4.0)
    assert torch.isnan(cp[pos[0] // 256, pos[1]]) and int(torch.isnan(cp).sum()) == 1


@pytest.mark.parametrize("fmt", [0, 1])
def test_inf_saturates_everywhere(cuda, fmt):
    x, _ = nan_input((0, 0), fmt)
    x[0, 0], x[319, 127] = float("inf"), float("-inf")
    amax = f32(0.0, cuda)
    q, qT, _ = run_t2(x.to(cuda), f32(1.0, cuda), fmt=fmt, amax=amax)
    check_t2("inf", q, qT, quant_ref(x, 1.0, fmt), fmt)
    assert q[0, 0].item() == TOP[fmt] and q[319, 127].item() == TOP[fmt] | 0x80
    assert same_bits(amax, float("inf"))
    if fmt == 0:
        amax = f32(0.0, cuda)
        rc, qf, _ = run_quant(x.to(cuda).view(-1), f32(1.0, cuda), amax)
        assert rc == 0 and qf[0].item() == TOP[0] and qf[-1].item() == TOP[0] | 0x80 and same_bits(amax, float("inf"))
        assert_bytes("inf flat", qf, quant_ref(x.view(-1), 1.0, 0), 0)


@pytest.fixture(params=[0, 1], ids=["q8-gemm256", "q8-w4"])
def q8_kernel(request):
    """The producer-quantizing GEMM on the 8-wave gemm256 epilogue or on the 4-wave fp8 kernel's, pinned through the
    launch counters (as in test_fp8_fused_gpu.py)."""
    K().dtf_fp8_w4_enable(request.param)
    before = launch_counts()
    yield request.param
    K().dtf_fp8_w4_enable(-1)
    d = launch_delta(before)
    if request.param == 1:
        assert d["w4f8_256"] + d["w4f8_128"] > 0 and d["gemm256_fp8"] == 0, d
    else:
        assert d["gemm256_fp8"] > 0 and d["w4f8_256"] + d["w4f8_128"] == 0, d


@pytest.mark.parametrize("q8fmt", [0, 1])
def test_nan_through_q8_epilogue(cuda, q8_kernel, q8fmt):
    """A q8 GEMM (M 512, N 256, K 128; K 256 on the 8-wave kernel, which takes no fewer than two 128-byte K-tiles and
    answers -6 to K 128) on integer operands with one NaN bias element: that output column is NaN codes in
    q8, that row of q8T, NaN in both 128-row column sums; every other byte equals the reference quantization of the
    bf16 output, amax is the maximum over the other columns and their column sums are exact."""
    M, N, Kd, col = 512, 256, 128 if q8_kernel else 256, 77
    a = fp8_int_operand((M, Kd), 0, 31).to(cuda)
    b = fp8_int_operand((N, Kd), 0, 32).to(cuda)
    bias = draw_ints((N,), 33).float()
    bias[col] = float("nan")
    bias_d = bias.to(cuda)
    scales = torch.tensor([0.5, 0.25], device=cuda)
    k = -1  # delayed scale 2^-1 from amax_prev
    slots = torch.tensor([7.0, 0.0, FMAX[q8fmt] * 2.0 ** k, -1.0, -1.0], device=cuda)  # scale amax prev used used2
    y = torch.full((M, N), 3.0, dtype=BF16, device=cuda)
    q = torch.full((M, N), FILL, dtype=U8, device=cuda)
    qT = torch.full((N, M), FILL, dtype=U8, device=cuda)
    cs = torch.full((M // 128, N), -7.0, dtype=F32, device=cuda)
    rc = K().dtf_gemm_fp8_q8(ptr(a), ptr(b), ptr(y), None, ptr(bias_d), ptr(scales), M, N, Kd, Kd, Kd, 0, 0,
                             None, 0, None, ptr(q), ptr(qT), ptr(cs), q8fmt, ptr(slots[0:1]), ptr(slots[1:2]),
                             ptr(slots[2:3]), ptr(slots[3:4]), ptr(slots[4:5]), stream())
    torch.cuda.synchronize()
    assert rc == 0
    y, q, qT, cs = y.cpu(), q.cpu(), qT.cpu(), cs.cpu()
    ref64 = 0.125 * decode(a.cpu(), 0) @ decode(b.cpu(), 0).t() + bias.double()
    want_y = ref64.float().to(BF16)
    assert torch.isnan(y[:, col]).all() and torch.equal(torch.nan_to_num(y.float()), torch.nan_to_num(want_y.float()))
    assert same_bits(slots[3], 2.0 ** k) and same_bits(slots[4], 2.0 ** k)
    SEEN[f"q8 epilogue {q8_kernel} fmt {q8fmt}"] = q[0, col].item()
    print(f"  q8 epilogue (w4 {q8_kernel}, fmt {q8fmt}): NaN stored as 0x{q[0, col].item():02X}")
    assert is_nan_code(q[:, col], q8fmt).all(), f"NaN column stored as 0x{q[0, col].item():02X}"
    assert_bytes("q8", q, quant_ref(want_y.float(), 2.0 ** k, q8fmt), q8fmt)
    assert torch.equal(qT, q.t().contiguous())
    others = torch.arange(N) != col
    assert same_bits(slots[1], want_y.float()[:, others].abs().max().item())
    want_cs = want_y.double().reshape(M // 128, 128, N).sum(1)
    assert torch.isnan(cs[:, col]).all() and torch.equal(cs[:, others].double(), want_cs[:, others])


def test_layer_propagates_nan(cuda):
    """_Proj(256, gelu, fp8): a NaN in one input row gives a non-finite output row; a NaN in one row of dy gives a
    non-finite dX row and non-finite kernel and bias gradients."""
    from distributed_tensorflow_amd.models.transformer import _Proj
    torch.manual_seed(0)
    layer = _Proj(256, activation="gelu", fp8=True)
    x0 = torch.randn(512, 256, device=cuda).to(BF16)
    xg = x0.clone().requires_grad_(True)
    layer(xg).backward(torch.randn(512, 256, device=cuda).to(BF16))  # build + bootstrap the delayed scales (the
    #                    gradient scale's bootstrap takes max |dy| of the first backward: a finite one)
    x = x0.clone()
    x[37, 5] = float("nan")
    y = layer(x)
    torch.cuda.synchronize()
    bad = ~torch.isfinite(y.float()).all(1)
    assert bad[37].item() and int(bad.sum()) == 1, torch.nonzero(bad).view(-1).tolist()
    layer.kernel.grad = layer.bias.grad = None
    xg = x0.clone().requires_grad_(True)
    y = layer(xg)
    dy = torch.randn(512, 256, device=cuda).to(BF16)
    dy[101, 9] = float("nan")
    y.backward(dy)
    torch.cuda.synchronize()
    bad = ~torch.isfinite(xg.grad.float()).all(1)
    assert bad[101].item() and int(bad.sum()) == 1, torch.nonzero(bad).view(-1).tolist()
    assert not torch.isfinite(layer.kernel.grad.float()).all()
    assert not torch.isfinite(layer.bias.grad.float()).all()
