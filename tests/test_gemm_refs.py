"""The references of test_gemm_edges_gpu.py (tests/_gemmref.py) checked on the CPU: the exactness guard trips when it
should, check_elems accepts f32 summations in different orders and rejects a result rounded through bf16 or missing one
K-tile; and ops.linalg._pad_operands (pure Python), which every unaligned GEMM goes through."""
import pytest
import torch

from distributed_tensorflow_amd.ops import linalg as LA

from _gemmref import (SENTINEL, abs_product, assert_exact, bf16_half_ulp, bf16_round, check_elems, gemm_f64,
                      guarded_out, int_operand)

BF = torch.bfloat16


def test_int_operand_range_zero_and_signs():
    t = int_operand((5, 7), -3, 3, 0)
    assert t.dtype == BF and t.shape == (5, 7)
    d = t.double()
    assert torch.equal(d, d.round()) and d.min() == -3 and d.max() == 3 and (d == 0).any()
    assert torch.equal(int_operand((5, 7), -3, 3, 0), t) and not torch.equal(int_operand((5, 7), -3, 3, 1), t)


def test_exact_guard_trips_and_passes():
    A, B = int_operand((8, 64), -3, 3, 1), int_operand((8, 64), -3, 3, 2)
    _, ref = gemm_f64(A, B)
    assert_exact("small", ref.float(), ref)
    assert_exact("small bf16", ref.to(BF), ref)
    # integers up to 2^13 over K = 64: products up to 2^26, outside the exact range of an f32 sum
    big = torch.full((8, 64), 8192.0).to(BF)
    _, ref = gemm_f64(big, big)
    with pytest.raises(AssertionError, match="TEST BUG"):
        assert_exact("big", ref.float(), ref)
    # the reference fits but a partial quantity does not
    with pytest.raises(AssertionError, match="TEST BUG"):
        assert_exact("partial", torch.zeros(2, 2), torch.zeros(2, 2, dtype=torch.float64),
                     partial=[torch.full((2,), 2.0 ** 24, dtype=torch.float64)])
    # |beta| enters the guard
    r = torch.full((2, 2), 2.0 ** 23, dtype=torch.float64)
    assert_exact("beta 0", r.float(), r)
    with pytest.raises(AssertionError, match="TEST BUG"):
        assert_exact("beta 1", r.float(), r, beta=1.0)


def test_assert_exact_reports_first_difference(capsys):
    _, ref = gemm_f64(int_operand((8, 64), -3, 3, 1), int_operand((16, 64), -3, 3, 2))
    out = ref.float()
    out[3, 5] += 1
    out[6, 1] -= 2
    with pytest.raises(AssertionError, match=r"2 of 128 elements differ; first at \(3, 5\)"):
        assert_exact("diff", out, ref)
    # bf16 outputs are compared with the nearest-even image: 301 and 303 are ties between bf16 neighbours
    ref = torch.tensor([[301.0, 303.0]], dtype=torch.float64)
    assert torch.equal(bf16_round(ref), torch.tensor([[300.0, 304.0]], dtype=torch.float64))
    assert_exact("rne", torch.tensor([[300.0, 304.0]]).to(BF), ref)
    with pytest.raises(AssertionError, match="differ"):
        assert_exact("rne", torch.tensor([[302.0, 304.0]]).to(BF), ref)


def _f32_sum(a, b, order):
    """A B^T accumulated in f32 one k at a time in the given order of k."""
    acc = torch.zeros(a.shape[0], b.shape[0], dtype=torch.float32)
    af, bfl = a.float(), b.float()
    for k in order:
        acc = acc + af[:, k:k + 1] * bfl[:, k].unsqueeze(0)
    return acc


def test_check_elems_accepts_f32_orders_rejects_bf16_and_missing_tile():
    torch.manual_seed(0)
    K = 256
    a, b = torch.randn(24, K).to(BF), torch.randn(40, K).to(BF)
    _, ref = gemm_f64(a, b)
    S = abs_product(a, b)
    fwd = _f32_sum(a, b, range(K))
    rev = _f32_sum(a, b, reversed(range(K)))
    assert not torch.equal(fwd, rev)  # the two orders do round differently
    assert check_elems("forward", fwd, ref, S, K) <= 1.0
    assert check_elems("reverse", rev, ref, S, K) <= 1.0
    assert check_elems("bf16 out", fwd.to(BF), ref, S, K, bf16_out=True) <= 1.0
    # the nearest bf16 of the EXACT value sits up to 2^-8 |ref| away (half an ulp at the bottom of a binade): the bf16
    # term of the bound has to be the exact half ulp, 2^-9 |ref| alone rejects correct rounding
    exact16 = bf16_round(ref)
    assert ((exact16 - ref).abs() > 2.0 ** -9 * ref.abs()).any()
    assert ((exact16 - ref).abs() <= bf16_half_ulp(ref) + 2.0 ** -24 * ref.abs()).all()  # (+ the f32 step of bf16_round)
    assert check_elems("rounded reference", exact16.to(BF), ref, S, K, bf16_out=True) <= 1.0
    with pytest.raises(AssertionError):  # an f32 accumulator rounded through bf16
        check_elems("through bf16", fwd.to(BF).float(), ref, S, K)
    with pytest.raises(AssertionError):  # one K-tile of 64 left out
        check_elems("tile dropped", _f32_sum(a, b, range(64, K)), ref, S, K)
    with pytest.raises(AssertionError):
        check_elems("tile dropped bf16", _f32_sum(a, b, range(64, K)).to(BF), ref, S, K, bf16_out=True)


def test_gemm_f64_layouts_batch_and_epilogue():
    A, B = int_operand((3, 8, 16), -3, 3, 3), int_operand((3, 24, 16), -3, 3, 4)
    bias, C0 = int_operand((24,), -3, 3, 5).float(), int_operand((3, 8, 24), -3, 3, 6)
    pre, out = gemm_f64(A, B, alpha=0.5, beta=-1.0, C0=C0, bias=bias, act="relu")
    want = 0.5 * torch.einsum("bmk,bnk->bmn", A.double(), B.double()) - C0.double() + bias.double()
    assert torch.equal(pre, want) and torch.equal(out, want.clamp_min(0))
    pre2, _ = gemm_f64(A.transpose(1, 2).contiguous(), B.transpose(1, 2).contiguous(), ak=True, bk=True, alpha=0.5,
                       beta=-1.0, C0=C0, bias=bias)
    assert torch.equal(pre2, want)
    _, g = gemm_f64(A, B, act="gelu")
    x = torch.einsum("bmk,bnk->bmn", A.double(), B.double())
    torch.testing.assert_close(g, torch.nn.functional.gelu(x, approximate="tanh"), rtol=1e-12, atol=1e-12)


def test_guarded_out_catches_stores_outside_the_view():
    view, check = guarded_out(5, 8, 16, torch.float32)
    assert view.shape == (5, 8) and view.stride() == (16, 1)
    view.fill_(1.0)
    check()
    view.as_strided((6, 8), (16, 1))[5, 0] = 0.0  # a row past M
    with pytest.raises(AssertionError, match="overwritten"):
        check()
    view, check = guarded_out(5, 8, 16, BF)
    view.as_strided((5, 9), (16, 1))[2, 8] = 1.0  # a column past N
    with pytest.raises(AssertionError, match=r"first at \(2, 8\)"):
        check()
    assert float(torch.tensor(SENTINEL).to(BF)) == SENTINEL


# ---------------------------------------------------------------- ops.linalg._pad_operands
def test_pad_operands_none_when_aligned():
    a, b = torch.zeros(8, 8, dtype=BF), torch.zeros(8, 8, dtype=BF)
    for ak in (False, True):
        for bk in (False, True):
            assert LA._pad_operands(a, b, ak, bk) is None
    # K-contiguous operands: M is free, N needs % 4 only
    assert LA._pad_operands(torch.zeros(3, 16, dtype=BF), torch.zeros(12, 16, dtype=BF), False, False) is None
    assert LA._pad_operands(torch.zeros(2, 3, 16, dtype=BF), torch.zeros(2, 12, 16, dtype=BF), False, False) is None


def _up(v, m):
    return -(-v // m) * m


@pytest.mark.parametrize("M,N,K", [(3, 10, 7), (13, 24, 5), (8, 8, 8)])
@pytest.mark.parametrize("ak,bk", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("batch", [0, 3])
def test_pad_operands_shapes_and_zero_fill(M, N, K, ak, bk, batch):
    lead = (batch,) if batch else ()
    A, B = int_operand(lead + (M, K), -3, 3, 1), int_operand(lead + (N, K), -3, 3, 2)
    a = A.transpose(-1, -2).contiguous() if ak else A
    b = B.transpose(-1, -2).contiguous() if bk else B
    Kp, Mp, Np = _up(K, 8), (_up(M, 8) if ak else M), (_up(N, 8) if bk else _up(N, 4))
    res = LA._pad_operands(a, b, ak, bk)
    if (Kp, Mp, Np) == (K, M, N):
        assert res is None
        return
    a2, b2, M2, N2 = res
    assert (M2, N2) == (M, N)
    assert a2.shape == lead + ((Kp, Mp) if ak else (Mp, Kp)) and a2.is_contiguous() and a2.dtype == BF
    assert b2.shape == lead + ((Kp, Np) if bk else (Np, Kp)) and b2.is_contiguous() and b2.dtype == BF
    la = a2.transpose(-1, -2) if ak else a2
    lb = b2.transpose(-1, -2) if bk else b2
    assert torch.equal(la[..., :M, :K], A) and torch.equal(lb[..., :N, :K], B)
    assert la.double().abs().sum() == A.double().abs().sum()  # everything outside the original block is zero
    assert lb.double().abs().sum() == B.double().abs().sum()
    # the padded product restricted to M x N is the product
    assert torch.equal(gemm_f64(a2, b2, ak, bk)[1][..., :M, :N], gemm_f64(a, b, ak, bk)[1])
