"""CPU tests of the fp8 references (tests/_fp8ref.py) that test_fp8_edges_gpu.py compares the kernels with: the two
independent roundings agree, ties go to even, saturation and NaN behave as the quantizers' contract says, the integer
operands are exact, and the data of the GELU-folded case keeps inside its cap with the reference alone."""
import pytest
import torch

from _fp8ref import (BF16, FMAX, GELU_SHARE_CAP, NAN_CODE, TOP, TORCH_DT, assert_bytes, count_adjacent, decode,
                     draw_ints, fp8_int_operand, gelu_band, gelu_case, is_nan_code, neighbours, quant_ref, round_table,
                     round_torch, scaled, sweep_fill, sweep_values)
from _gemmref import assert_exact

FMTS = [0, 1]
SCALES = [2.0 ** -3, 1.0, 2.0 ** 5]


@pytest.mark.parametrize("fmt", FMTS)
def test_decode_matches_torch_and_codes_round_trip(fmt):
    codes = torch.arange(256, dtype=torch.uint8)
    v = decode(codes, fmt)
    tv = codes.view(TORCH_DT[fmt]).double()
    assert torch.equal(torch.isnan(v), torch.isnan(tv)) and torch.equal(torch.isnan(v), is_nan_code(codes, fmt))
    fin = torch.isfinite(v)
    assert torch.equal(v[~torch.isnan(v)], tv[~torch.isnan(v)])
    assert v[fin].abs().max().item() == FMAX[fmt] and decode(torch.tensor([TOP[fmt]], dtype=torch.uint8), fmt) == FMAX[fmt]
    # every finite code is a fixed point of both roundings (scale 1)
    assert torch.equal(round_table(v[fin], fmt), codes[fin])
    assert torch.equal(round_torch(v[fin], fmt), codes[fin])
    assert torch.equal(quant_ref(v[fin], 1.0, fmt), codes[fin])


@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("scale", SCALES)
def test_roundings_agree_on_sweep(fmt, scale):
    x, ti, tc = sweep_values(fmt, scale)
    y = scaled(x, scale, fmt)
    a, b = round_torch(y, fmt), round_table(y, fmt)
    assert torch.equal(a, b)
    # ties: both roundings land on the even code, chosen here from the code pair alone
    assert (tc % 2 == 0).all() and torch.equal(a[ti], tc)
    # and one bf16 ulp to either side leaves the tie for the nearer code
    n = TOP[fmt]
    lo_side, hi_side = a[ti + n], a[ti + 2 * n]
    pos = torch.arange(n, dtype=torch.uint8)
    assert torch.equal(lo_side[:n], pos) and torch.equal(hi_side[:n], pos + 1)
    assert torch.equal(lo_side[n:], pos | 0x80) and torch.equal(hi_side[n:], (pos + 1) | 0x80)


@pytest.mark.parametrize("fmt", FMTS)
def test_roundings_agree_on_random(fmt):
    g = torch.Generator().manual_seed(3 + fmt)
    # magnitudes spread over every binade of the format, subnormals and the saturated range included
    e = torch.rand(100000, generator=g) * 30 - (12 if fmt == 0 else 20)
    v = (torch.randn(100000, generator=g) * torch.exp2(e)).float()
    for scale in (1.0, 0.05):
        y = scaled(v, scale, fmt)
        assert torch.equal(round_torch(y, fmt), round_table(y, fmt))


def test_tie_examples():
    """The cases named when the reference was chosen: 17 -> 16, 19 -> 20, 2^-10 -> 0, 1.5 * 2^-10 -> 2^-9 in e4m3."""
    v = torch.tensor([17.0, 19.0, 2.0 ** -10, 1.5 * 2.0 ** -10])
    for r in (round_torch, round_table):
        assert decode(r(v, 0), 0).tolist() == [16.0, 20.0, 0.0, 2.0 ** -9]
    # e5m2: 61440 is the midpoint between 57344 and the next power of two: the conversion alone gives inf, which is why
    # quant_ref clamps first
    assert torch.isinf(decode(round_torch(torch.tensor([61440.0]), 1), 1)).all()
    assert decode(quant_ref(torch.tensor([61440.0]), 1.0, 1), 1).item() == 57344.0


@pytest.mark.parametrize("fmt", FMTS)
def test_saturation_nan_and_floor(fmt):
    inf = float("inf")
    v = torch.tensor([inf, -inf, 3.0e38, -3.0e38, FMAX[fmt] * 1.01, float("nan"), 0.0, -0.0])
    q = quant_ref(v, 1.0, fmt)
    d = decode(q, fmt)
    assert d[:5].tolist() == [FMAX[fmt], -FMAX[fmt], FMAX[fmt], -FMAX[fmt], FMAX[fmt]]
    assert is_nan_code(q, fmt).tolist() == [False] * 5 + [True, False, False]
    assert q[6].item() == 0x00 and q[7].item() == 0x80
    assert is_nan_code(round_table(torch.tensor([float("nan")]), fmt), fmt).all()
    assert is_nan_code(torch.tensor([NAN_CODE], dtype=torch.uint8), fmt).all()
    # a zero scale uses the floor: {0, +-1} -> {0, +-FMAX}, no NaN
    assert decode(quant_ref(torch.tensor([0.0, 1.0, -1.0]), 0.0, fmt), fmt).tolist() == [0.0, FMAX[fmt], -FMAX[fmt]]


@pytest.mark.parametrize("fmt", FMTS)
def test_neighbours_and_compare_helpers(fmt):
    c = torch.tensor([0x00, 0x80, 0x01, 0x81, TOP[fmt], TOP[fmt] | 0x80], dtype=torch.uint8)
    lo, hi = neighbours(c, fmt)
    assert lo.tolist() == [0x81, 0x81, 0x00, 0x82, TOP[fmt] - 1, TOP[fmt] | 0x80]
    assert hi.tolist() == [0x01, 0x01, 0x02, 0x00, TOP[fmt], (TOP[fmt] - 1) | 0x80]
    assert count_adjacent("adj", hi, c, fmt) == 5  # (TOP saturates onto itself)
    with pytest.raises(AssertionError):
        count_adjacent("adj", torch.tensor([0x03], dtype=torch.uint8), torch.tensor([0x01], dtype=torch.uint8), fmt)
    with pytest.raises(AssertionError):
        assert_bytes("b", hi, c, fmt)
    with pytest.raises(AssertionError):  # the old clamp's byte for a NaN is not a NaN code
        assert_bytes("b", torch.tensor([TOP[fmt] | 0x80], dtype=torch.uint8),
                     torch.tensor([NAN_CODE], dtype=torch.uint8), fmt)
    assert_bytes("b", torch.tensor([0xFF], dtype=torch.uint8), torch.tensor([NAN_CODE], dtype=torch.uint8), fmt)


@pytest.mark.parametrize("fmt", FMTS)
def test_sweep_fill_covers_every_code(fmt):
    x, ti, tc = sweep_fill((64, 64), fmt, 2.0 ** 5)
    assert x.dtype == BF16 and x.shape == (64, 64) and ti.numel() == 2 * TOP[fmt]
    q = quant_ref(x, 2.0 ** 5, fmt)
    fin = torch.isfinite(decode(torch.arange(256, dtype=torch.uint8), fmt))
    assert set(torch.arange(256)[fin].tolist()) <= set(q.view(-1).tolist())
    x2, _, _ = sweep_fill((64, 64), fmt, 2.0 ** 5, overflow=False)
    assert x2.double().abs().max().item() == FMAX[fmt] * 2.0 ** 5


@pytest.mark.parametrize("fmt", FMTS)
def test_int_operand_is_exact(fmt):
    b = fp8_int_operand((129, 128), fmt, 7)
    want = draw_ints((129, 128), 7)
    assert b.dtype == torch.uint8 and torch.equal(decode(b, fmt), want)
    assert torch.equal(b.view(TORCH_DT[fmt]).double(), want)
    assert want.min().item() == -8 and want.max().item() == 8 and (want == 0).any()


def test_exact_range_guard_fires():
    """K = 2^19 terms of 8 * 8 leave the exact f32 range: assert_exact reports a bug of the TEST, not of a kernel."""
    ref = torch.full((1, 1), 64.0 * 2 ** 19, dtype=torch.float64)
    with pytest.raises(AssertionError, match="TEST BUG"):
        assert_exact("guard", ref.float(), ref)
    ok = torch.full((1, 1), 64.0 * 4096, dtype=torch.float64)
    assert_exact("guard", ok.float(), ok)


def gelu_share(seed, shape=(320, 128), scale=2.0 ** -13, fmt=1):
    dy, pre = gelu_case(shape, seed)
    ref, lo, hi, _ = gelu_band(dy, pre, scale, fmt)
    return ((lo != ref) | (hi != ref)).double().mean().item()


def test_gelu_band_share_of_the_chosen_seed():
    """The GPU test allows the kernel's byte to differ from the reference's only inside the 2^-12 |dy| band; the
    share of elements whose band crosses a rounding boundary stays under the cap for the data it uses."""
    share = gelu_share(11)
    print(f"  GELU band share {share:.4%}")
    assert 0 < share <= GELU_SHARE_CAP
