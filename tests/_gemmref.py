"""Float64 references and exact / per-element comparisons for the bf16 GEMM routes (shared by test_gemm_refs.py and
test_gemm_edges_gpu.py).

Exact tests: bf16 holds the integers up to 256 exactly, a product of two bf16 values is exact in f32 and an f32 sum of
integers stays exact in ANY order while every partial sum is below 2^24. With small-integer operands every GEMM route
must therefore reproduce the float64 result bit for bit: f32 outputs as they are, bf16 outputs as the round-to-nearest-
even image of the float64 value. assert_exact first checks that the REFERENCE keeps inside that range (a failure there
is a bug of the test), then compares with torch.equal.

Random data: check_elems bounds every element by what an f32 summation of its own K terms can lose.
"""
import math

import torch

BF16 = torch.bfloat16
EXACT = float(2 ** 24)
SENTINEL = 12288.0  # 1.5 * 2^13: exact in bf16 and f32, far from any value the exact tests produce


def bf16_round(t):
    """float64 -> nearest-even bf16 -> float64."""
    return t.float().bfloat16().double()


def int_operand(shape, lo, hi, seed):
    """bf16 CPU tensor of integers drawn uniformly from [lo, hi]; a zero and both ends of the range are always present
    (when the tensor has room for them)."""
    assert lo <= 0 <= hi and max(-lo, hi) <= 256, (lo, hi)
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    flat = t.view(-1)
    if flat.numel() >= 3:
        pos = torch.randperm(flat.numel(), generator=g)[:3]
        flat[pos[0]], flat[pos[1]], flat[pos[2]] = 0.0, float(lo), float(hi)
    out = t.to(BF16)
    assert torch.equal(out.double(), t)
    return out


def gelu_f64(x):
    """tanh-GELU in float64 (the form the kernels approximate)."""
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


def _logical(t, kouter):
    t = t.detach().double().cpu()
    return t.transpose(-1, -2) if kouter else t


def gemm_f64(A, B, ak=False, bk=False, alpha=1.0, beta=0.0, C0=None, bias=None, act=None):
    """float64 reference of ops.gemm on the (already rounded) stored operands: A [.., M, K] ([.., K, M] with ak), B
    [.., N, K] ([.., K, N] with bk), batched or not. Returns (pre, out): pre = alpha * A B^T + beta * C0 + bias, out =
    act(pre) with act None / 0, "relu" / 1 or "gelu" / 2."""
    a, b = _logical(A, ak), _logical(B, bk)
    pre = alpha * torch.matmul(a, b.transpose(-1, -2))
    if beta != 0:
        pre = pre + beta * C0.detach().double().cpu()
    if bias is not None:
        pre = pre + bias.detach().double().cpu()
    if act in (None, 0, "linear"):
        out = pre
    elif act in (1, "relu"):
        out = torch.relu(pre)
    elif act in (2, "gelu"):
        out = gelu_f64(pre)
    else:
        raise ValueError(act)
    return pre, out


def abs_product(A, B, ak=False, bk=False, alpha=1.0):
    """S = |alpha| * |A| |B|^T in float64: the sum of the absolute values of every output element's K terms."""
    a, b = _logical(A, ak).abs(), _logical(B, bk).abs()
    return abs(alpha) * torch.matmul(a, b.transpose(-1, -2))


def assert_exact(name, out, ref64, beta=0.0, partial=()):
    """out (f32 or bf16) equals the float64 reference exactly (bf16: its nearest-even image). `partial`: float64
    tensors of every other quantity the test relies on being exact in f32 (the product before beta, sums of |terms|)."""
    ref64 = ref64.detach().double().cpu()
    top = ref64.abs().max().item() * (1.0 + abs(beta)) if ref64.numel() else 0.0
    assert top < EXACT, f"{name}: TEST BUG, reference magnitude {top:.0f} leaves the exact f32 range"
    for p in partial:
        pm = p.detach().double().abs().max().item() if p.numel() else 0.0
        assert pm < EXACT, f"{name}: TEST BUG, a partial quantity ({pm:.0f}) leaves the exact f32 range"
    assert out.shape == ref64.shape, (name, out.shape, ref64.shape)
    got = out.detach().double().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    want = bf16_round(ref64) if out.dtype == BF16 else ref64
    if not torch.equal(got, want):
        bad = torch.nonzero(got != want)
        first = tuple(bad[0].tolist())
        msg = (f"{name}: {bad.shape[0]} of {got.numel()} elements differ; first at {first}: got {got[first].item()!r}, "
               f"expected {want[first].item()!r}")
        print("  " + msg)
        raise AssertionError(msg)


def bf16_half_ulp(v):
    """Half a bf16 ulp at |v| (float64): 2^(floor(log2 |v|) - 8), 0 at 0. Between 2^-9 |v| (top of a binade) and
    2^-8 |v| (bottom): what rounding an exact value to the nearest bf16 can move it by."""
    v = v.detach().double().abs()
    _, e = torch.frexp(v)  # v = m * 2^e, m in [0.5, 1)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), e - 9), torch.zeros_like(v))


def check_elems(name, out, ref64, S, K, bf16_out=False, worst=None):
    """Per element |out - ref| <= K * 2^-23 * S (S: abs_product). K * 2^-24 * S bounds a round-to-nearest f32
    summation of K terms in any order (split-K slabs included); the factor 2 allows a truncating accumulator inside
    the MFMA, whose internal rounding is not documented. bf16 outputs add half a bf16 ulp of the largest value the
    bound admits, bf16_half_ulp(|ref| + bound): the exact half ulp, not 2^-9 * (|ref| + bound), which is half an ulp
    only at the top of a binade and which the correctly rounded image of an exact value misses by up to 2x
    (test_gemm_refs.py shows it). Prints, records and returns the worst err / bound; above 1 it fails."""
    ref64, S = ref64.detach().double().cpu(), S.detach().double().cpu()
    got = out.detach().double().cpu()
    assert got.shape == ref64.shape == S.shape, (name, got.shape, ref64.shape, S.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    bound = K * 2.0 ** -23 * S
    if bf16_out:
        bound = bound + bf16_half_ulp(ref64.abs() + bound)
    err = (got - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    w = ratio.max().item() if ratio.numel() else 0.0
    note = ""
    if bf16_out:  # for the record: the same figure with 2^-9 * (|ref| + bound) as the bf16 term
        lit = K * 2.0 ** -23 * S
        lit = lit + 2.0 ** -9 * (ref64.abs() + lit)
        note = f" (with 2^-9 |ref| as the bf16 term: {(err / lit.clamp_min(1e-300)).max().item():.3f})"
    print(f"  {name}: worst err / bound {w:.3f}{note}")
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), w)
    if w > 1.0:
        at = tuple(torch.nonzero(ratio == ratio.max())[0].tolist())
        raise AssertionError(f"{name}: element {at} off by {err[at].item():.3e} > bound {bound[at].item():.3e} "
                             f"(ratio {w:.3f})")
    return w


def guarded_out(M, N, ldc, dtype, sentinel=SENTINEL, device="cpu"):
    """An (M + 8) x ldc buffer filled with `sentinel` (a large finite integer, so equality works) and its [:M, :N]
    view. Returns (view, check); check() asserts that everything outside the view still holds the sentinel. The whole
    buffer belongs to the test: a kernel that stores past row M or column N fails the assertion, nothing faults."""
    assert ldc >= N
    buf = torch.full((M + 8, ldc), sentinel, dtype=dtype, device=device)
    view = buf[:M, :N]

    def check(name="guard"):
        keep = torch.ones(M + 8, ldc, dtype=torch.bool)
        keep[:M, :N] = False
        host = buf.detach().double().cpu()
        bad = torch.nonzero(keep & (host != sentinel))
        assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} elements outside the {M} x {N} output were overwritten; "
                                   f"first at {tuple(bad[0].tolist())}: {host[tuple(bad[0].tolist())].item()!r}")

    return view, check
