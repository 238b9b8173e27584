"""Exact tests of the fp8 GEMM routes (gemm_fp8.hip dtf_gemm_fp8_ex / dtf_gemm_fp8 / dtf_gemm_fp8_q8 on the 4-wave kernel
of gemm_w4_fp8.hip, the 8-wave kernel of gemm256.hip and the 128-row tiles of gemm_core.h) against float64.

Operands are fp8 codes of integers in [-8, 8] (exact in e4m3 and e5m2; tests/_fp8ref.py), scales [0.5, 0.25]: the
reference 0.125 * decode(A) @ decode(B)^T is exact in f32 in any summation order, so f32 outputs must equal it and bf16
outputs its nearest-even image (assert_exact of tests/_gemmref.py).

Routes, pinned through dtf_fp8_w4_enable and the launch counters:
  w4     the 4-wave kernel (counters w4f8_256 / w4f8_128), every shape dtf_gemm_fp8_ex admits;
  g256   the 8-wave kernel (gemm256_fp8), w4 off: non-split only where pick256_fp8 finds >= 128 tiles of 256 rows and
         K >= 256 (it takes no fewer than two 128-byte K-tiles), and every split-K call;
  t128   the 128-row tiles, which have no counter: w4 off and a shape the 8-wave kernel does not get (asserted: no
         counter moves). Through dtf_gemm_fp8 the `tile` argument picks 128x128 (0) or 128x64 (2).
"""
import pytest
import torch

from distributed_tensorflow_amd.ops._util import K, launch_counts, launch_delta, ptr, stream, workspace

from _fp8ref import TORCH_DT, decode, draw_ints, fp8_int_operand
from _gemmref import SENTINEL, assert_exact, check_elems, gelu_f64, guarded_out

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
U8 = torch.uint8
WORST = {}  # worst err / bound of the random-normal cases, printed per test
_CACHE = {}


@pytest.fixture(scope="module")
def cuda():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda:0")


def operands(M, N, Kd, fmt_a):
    """(A codes [M, K], B codes [N, K], float64 0.125 * A B^T, float64 0.125 * |A| |B|^T), cached."""
    key = (M, N, Kd, fmt_a)
    if key not in _CACHE:
        A, B = fp8_int_operand((M, Kd), fmt_a, 100 + fmt_a), fp8_int_operand((N, Kd), 0, 200)
        a64, b64 = decode(A, fmt_a), decode(B, 0)
        _CACHE[key] = (A, B, 0.125 * a64 @ b64.t(), 0.125 * a64.abs() @ b64.abs().t())
    return _CACHE[key]


def strided(t, ld, dev, fill=0x38):
    """The code matrix as a [rows, K] view of a [rows, ld] buffer (the padding holds the code of 1.0)."""
    wide = torch.full((t.shape[0], ld), fill, dtype=U8, device=dev)
    wide[:, :t.shape[1]] = t.to(dev)
    return wide[:, :t.shape[1]]


def scales(dev):
    return torch.tensor([0.5, 0.25], device=dev)


def gemm_ex(a, b, out, *, fmt_a=0, beta=0.0, splitk=1, bias=None, act=0, aux=None, zero_slot=None, ws="auto", M=None,
            N=None, Kd=None, lda=None, ldb=None, ws_elems=None):
    """dtf_gemm_fp8_ex with its raw status."""
    ws = workspace(a.device) if (ws == "auto" and splitk > 1) else (None if isinstance(ws, str) else ws)
    rc = K().dtf_gemm_fp8_ex(ptr(a), ptr(b), ptr(out), ptr(aux), ptr(bias), ptr(scales(a.device)),
                             a.shape[0] if M is None else M, b.shape[0] if N is None else N,
                             a.shape[1] if Kd is None else Kd, a.stride(0) if lda is None else lda,
                             b.stride(0) if ldb is None else ldb, out.stride(0), act, fmt_a, int(out.dtype == F32),
                             float(beta), splitk, ptr(ws),
                             (ws.numel() if ws is not None else 0) if ws_elems is None else ws_elems, ptr(zero_slot),
                             stream())
    torch.cuda.synchronize()
    return rc


class Route:
    """Pins a dispatch: `with Route(kind): ...` sets the w4 switch, restores it and asserts the launch counters."""

    def __init__(self, kind, launches=1):
        self.kind, self.n = kind, launches

    def __enter__(self):
        K().dtf_fp8_w4_enable(1 if self.kind == "w4" else 0)
        self.before = launch_counts()
        return self

    def __exit__(self, et, ev, tb):
        K().dtf_fp8_w4_enable(-1)
        if et is None:
            d = launch_delta(self.before)
            got = (d["w4f8_256"] + d["w4f8_128"], d["gemm256_fp8"])
            want = {"w4": (self.n, 0), "g256": (0, self.n), "t128": (0, 0), "none": (0, 0)}[self.kind]
            assert got == want, (self.kind, d)
        return False


# ---------------------------------------------------------------- plain products
# a representative cross of M in {1, 129, 257, 264}, N in {8, 72, 136, 264}, K in {128, 384, 1152}, both A formats, both
# output types; none of these shapes reaches the 8-wave kernel (fewer than 128 tiles), so w4 off means the 128-row tiles
CROSS = [(1, 8, 128, 0, F32), (129, 72, 384, 1, BF), (257, 136, 1152, 0, BF), (264, 264, 128, 1, F32),
         (1, 264, 384, 1, BF), (264, 8, 1152, 0, F32), (129, 136, 128, 0, BF), (257, 72, 384, 1, F32),
         (264, 136, 1152, 1, BF), (129, 264, 1152, 0, F32), (257, 8, 128, 1, BF), (1, 72, 1152, 0, BF)]


@pytest.mark.parametrize("kind", ["w4", "t128"])
@pytest.mark.parametrize("M,N,Kd,fmt_a,dt", CROSS)
def test_ex_exact(cuda, kind, M, N, Kd, fmt_a, dt):
    A, B, ref, _ = operands(M, N, Kd, fmt_a)
    out, check = guarded_out(M, N, N, dt, device=cuda)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=fmt_a) == 0
    assert_exact(f"{kind} {M}x{N}x{Kd}", out, ref)
    check()


@pytest.mark.parametrize("fmt_a,dt", [(0, BF), (1, F32)])
@pytest.mark.parametrize("M,N,Kd", [(4096, 4096, 256), (4096, 1152, 256)], ids=["256x256", "256x128"])
def test_ex_exact_8wave(cuda, M, N, Kd, fmt_a, dt):
    """Shapes whose tile counts satisfy pick256_fp8: 256 tiles of 256x256, and 144 of 256x128 (80 of 256x256)."""
    A, B, ref, _ = operands(M, N, Kd, fmt_a)
    out, check = guarded_out(M, N, N, dt, device=cuda)
    with Route("g256"):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=fmt_a) == 0
    assert_exact(f"g256 {M}x{N}x{Kd}", out, ref)
    check()
    with Route("w4"):
        out.fill_(SENTINEL)
        assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=fmt_a) == 0
    assert_exact(f"w4 {M}x{N}x{Kd}", out, ref)


@pytest.mark.parametrize("tile", [0, 2], ids=["128x128", "128x64"])
def test_ex_128_row_tiles_both_widths(cuda, tile):
    """dtf_gemm_fp8_ex with w4 off and K = 128 (below the 8-wave kernel's minimum): >= 256 tiles of 128x128 take the
    128x128 kernel, fewer the 128x64 one."""
    M, N = (2048, 2056) if tile == 0 else (264, 136)
    for fmt_a in (0, 1):
        A, B, ref, _ = operands(M, N, 128, fmt_a)
        out, check = guarded_out(M, N, N, BF, device=cuda)
        with Route("t128"):
            assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=fmt_a) == 0
        assert_exact(f"t128 {M}x{N}", out, ref)
        check()


# ---------------------------------------------------------------- options, per route
OPT = {"w4": (264, 136, 384), "t128": (264, 136, 384), "g256": (4096, 1152, 256)}
KINDS = ["w4", "t128", "g256"]


@pytest.mark.parametrize("kind", KINDS)
def test_ex_beta_accumulates(cuda, kind):
    M, N, Kd = OPT[kind]
    A, B, ref, _ = operands(M, N, Kd, 1)
    c0 = draw_ints((M, N), 7, -100, 100)
    out, check = guarded_out(M, N, N, F32, device=cuda)
    out.copy_(c0)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=1, beta=1.0) == 0
    assert_exact(f"{kind} beta", out, ref + c0, beta=1.0, partial=(ref,))
    check()


@pytest.mark.parametrize("dt", [BF, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("kind", KINDS)
def test_ex_strided(cuda, kind, dt):
    """lda = K + 16, ldb = K + 32, ldc = N + 8: the padding is never read into the product or written."""
    M, N, Kd = OPT[kind]
    A, B, ref, _ = operands(M, N, Kd, 0)
    a, b = strided(A, Kd + 16, cuda), strided(B, Kd + 32, cuda)
    out, check = guarded_out(M, N, N + 8, dt, device=cuda)
    with Route(kind):
        assert gemm_ex(a, b, out) == 0
    assert_exact(f"{kind} strided", out, ref)
    check()


@pytest.mark.parametrize("kind", KINDS)
def test_ex_bias_relu_aux(cuda, kind):
    M, N, Kd = OPT[kind]
    A, B, ref, _ = operands(M, N, Kd, 0)
    bias = draw_ints((N,), 8, -50, 50)
    out, check = guarded_out(M, N, N, BF, device=cuda)
    aux, check_aux = guarded_out(M, N, N, BF, device=cuda)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, bias=bias.float().to(cuda), act=1, aux=aux) == 0
    assert_exact(f"{kind} aux", aux, ref + bias, partial=(ref,))
    assert_exact(f"{kind} relu", out, torch.relu(ref + bias), partial=(ref,))
    check()
    check_aux()


@pytest.mark.parametrize("kind", KINDS)
def test_ex_bias_gelu(cuda, kind):
    M, N, Kd = OPT[kind]
    A, B, ref, S = operands(M, N, Kd, 0)
    bias = draw_ints((N,), 9, -3, 3)
    out, check = guarded_out(M, N, N, BF, device=cuda)
    aux, _ = guarded_out(M, N, N, BF, device=cuda)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, bias=bias.float().to(cuda), act=2, aux=aux) == 0
    assert_exact(f"{kind} gelu aux", aux, ref + bias, partial=(ref,))
    check_elems(f"{kind} gelu", out, gelu_f64(ref + bias), S + bias.abs(), Kd, bf16_out=True, worst=WORST)
    check()


@pytest.mark.parametrize("kind", KINDS)
def test_ex_zero_slot(cuda, kind):
    """zero_slot: that one float becomes 0.0, its neighbours in a sentinel-filled buffer stay."""
    M, N, Kd = OPT[kind]
    A, B, ref, _ = operands(M, N, Kd, 0)
    slots = torch.full((9,), SENTINEL, dtype=F32, device=cuda)
    out = torch.full((M, N), SENTINEL, dtype=F32, device=cuda)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, zero_slot=slots[4:5]) == 0
    assert slots.tolist() == [SENTINEL] * 4 + [0.0] + [SENTINEL] * 4
    assert_exact(f"{kind} zero_slot", out, ref)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("splitk", [2, 3])
@pytest.mark.parametrize("kind", ["w4", "g256"])
def test_ex_splitk_uneven(cuda, kind, splitk, beta):
    """K = 640 = 5 K-tiles of 128 bytes: 2 splits take 3 + 2, 3 splits 2 + 2 + 1; the f32 slabs sum exactly (and the
    split-K launch clears zero_slot)."""
    M, N, Kd = 264, 136, 640
    A, B, ref, _ = operands(M, N, Kd, 1)
    c0 = draw_ints((M, N), 12, -100, 100)
    out = c0.float().to(cuda)
    slots = torch.full((9,), SENTINEL, dtype=F32, device=cuda)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=1, beta=beta, splitk=splitk, zero_slot=slots[4:5]) == 0
    assert slots.tolist() == [SENTINEL] * 4 + [0.0] + [SENTINEL] * 4
    assert_exact(f"{kind} splitk {splitk}", out, ref + beta * c0, beta=beta, partial=(ref,))


@pytest.mark.parametrize("kind", KINDS)
def test_nan_operand_byte_poisons_its_row_only(cuda, kind):
    M, N, Kd = OPT[kind]
    A, B, ref, _ = operands(M, N, Kd, 0)
    a = A.clone()
    a[130, 77] = 0x7F
    out = torch.full((M, N), SENTINEL, dtype=F32, device=cuda)
    with Route(kind):
        assert gemm_ex(a.to(cuda), B.to(cuda), out) == 0
    host = out.cpu()
    assert torch.isnan(host[130]).all()
    keep = torch.arange(M) != 130
    assert_exact(f"{kind} other rows", host[keep], ref[keep])


# ---------------------------------------------------------------- the old entry
@pytest.mark.parametrize("tile", [-1, 0, 2])
@pytest.mark.parametrize("N", [4, 12, 68])
@pytest.mark.parametrize("Kd", [16, 144, 272])
def test_old_entry_admits_partial_k_tiles(cuda, Kd, N, tile):
    """dtf_gemm_fp8 admits K % 16 == 0 and N % 4 == 0 (dtf_gemm_fp8_ex: K % 128, N % 8): a partial 128-byte K-tile,
    an output whose rows are no whole 16-byte chunks."""
    M = 129
    A, B, ref, _ = operands(M, N, Kd, 0)
    out, check = guarded_out(M, N, N + 8, BF, device=cuda)
    a, b = A.to(cuda), B.to(cuda)
    with Route("none"):
        K().dtf_fp8_w4_enable(-1)  # the default dispatch: neither pipelined kernel takes these shapes
        rc = K().dtf_gemm_fp8(ptr(a), ptr(b), ptr(out), None, None, ptr(scales(cuda)), M, N, Kd, Kd, Kd, out.stride(0),
                              0, tile, stream())
        torch.cuda.synchronize()
    assert rc == 0
    assert_exact(f"old entry {M}x{N}x{Kd} tile {tile}", out, ref)
    check()


# ---------------------------------------------------------------- refusals
def test_ex_refusals_leave_outputs_untouched(cuda):
    M, N, Kd = 264, 136, 384
    A, B, _, _ = operands(M, N, Kd, 0)
    a, b = A.to(cuda), B.to(cuda)
    bias = torch.zeros(N, device=cuda)
    small = torch.zeros(M * N, device=cuda)  # one slab: too small for two
    cases = [(-1, F32, dict(N=132)), (-1, F32, dict(Kd=320)), (-1, F32, dict(lda=Kd + 8)), (-1, F32, dict(ldb=Kd + 8)),
             (-1, F32, dict(M=0)), (-2, F32, dict(beta=0.5)), (-3, BF, dict(beta=1.0)), (-3, BF, dict(splitk=2)),
             (-4, F32, dict(splitk=2, ws=None)), (-4, F32, dict(splitk=2, ws=small)), (-4, F32, dict(splitk=2, bias=bias)),
             (-4, F32, dict(splitk=2, ld_out=N + 8))]
    for want, dt, kw in cases:
        ld = kw.pop("ld_out", N)
        out, check = guarded_out(M, N, ld, dt, device=cuda)
        slots = torch.full((3,), SENTINEL, dtype=F32, device=cuda)
        with Route("none"):
            rc = gemm_ex(a, b, out, zero_slot=slots[1:2], **kw)
        assert rc == want, (want, kw, rc)
        assert (out == SENTINEL).all() and (slots == SENTINEL).all(), (want, kw)
        check()
    # -5: a split-K call that no pipelined kernel takes (w4 off; K = 128 is below the 8-wave kernel's two K-tiles)
    A, B, _, _ = operands(264, 136, 128, 0)
    out, check = guarded_out(264, 136, 136, F32, device=cuda)
    with Route("none"):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, splitk=2) == -5
    assert (out == SENTINEL).all()
    check()


def test_q8_refusals_leave_outputs_untouched(cuda):
    """-1 (operand alignment) and -6 (a shape the pipelined kernels do not take): C and the fp8 copies keep their
    sentinels, the scale slots their values."""
    N, Kd = 256, 256
    for want, M, kw in ((-1, 512, dict(Kd=192)), (-1, 512, dict(N=252)), (-6, 200, {}), (-6, 512, dict(no_scale=True))):
        a = torch.zeros(512, Kd, dtype=U8, device=cuda)
        b = torch.zeros(N, Kd, dtype=U8, device=cuda)
        c = torch.full((512, N), SENTINEL, dtype=BF, device=cuda)
        q = torch.full((512, N), 0xA5, dtype=U8, device=cuda)
        qT = torch.full((N, 512), 0xA5, dtype=U8, device=cuda)
        cs = torch.full((4, N), SENTINEL, dtype=F32, device=cuda)
        slots = torch.tensor([1.0, 2.0, 3.0, -1.0, -1.0], device=cuda)
        with Route("none"):
            rc = K().dtf_gemm_fp8_q8(ptr(a), ptr(b), ptr(c), None, None, ptr(scales(cuda)), M, kw.get("N", N),
                                     kw.get("Kd", Kd), Kd, Kd, 0, 0, None, 0, None, ptr(q), ptr(qT), ptr(cs), 0,
                                     None if kw.get("no_scale") else ptr(slots[0:1]), ptr(slots[1:2]), ptr(slots[2:3]),
                                     ptr(slots[3:4]), ptr(slots[4:5]), stream())
            torch.cuda.synchronize()
        assert rc == want, (want, M, kw, rc)
        assert (c == SENTINEL).all() and (q == 0xA5).all() and (qT == 0xA5).all() and (cs == SENTINEL).all()
        assert slots.tolist() == [1.0, 2.0, 3.0, -1.0, -1.0]


# ---------------------------------------------------------------- random data
@pytest.mark.parametrize("fmt_a", [0, 1])
@pytest.mark.parametrize("kind", ["w4", "g256"])
def test_ex_random_normal_splitk(cuda, kind, fmt_a):
    """Normal data quantized by torch on the CPU, K = 4096 in 4 splits, f32 out: every element within what an f32
    summation of its own K terms can lose (check_elems)."""
    M, N, Kd = 264, 136, 4096
    g = torch.Generator().manual_seed(40 + fmt_a)
    A = (torch.randn(M, Kd, generator=g) * 2).to(TORCH_DT[fmt_a]).view(U8)
    B = (torch.randn(N, Kd, generator=g) * 2).to(TORCH_DT[0]).view(U8)
    a64, b64 = decode(A, fmt_a), decode(B, 0)
    out = torch.full((M, N), SENTINEL, dtype=F32, device=cuda)
    with Route(kind):
        assert gemm_ex(A.to(cuda), B.to(cuda), out, fmt_a=fmt_a, splitk=4) == 0
    check_elems(f"{kind} fmt_a {fmt_a} random", out, 0.125 * a64 @ b64.t(), 0.125 * a64.abs() @ b64.abs().t(), Kd,
                worst=WORST)
