"""Byte-exact references for the fp8 quantizers and GEMM routes (shared by test_fp8_refs.py and test_fp8_edges_gpu.py).

Formats: fmt 0 = OCP e4m3fn (bias 7, no infinities, the two all-ones codes 0x7F / 0xFF are NaN, largest finite 448),
fmt 1 = e5m2 (bias 15, IEEE-like: exponent 31 is inf / NaN, largest finite 57344).

quant_ref is the operation the quantizers claim to perform, written plainly: y = v * (1 / max(scale, floor)) in
float32, NaN stays NaN, everything else is clamped to +-FMAX (so +-inf saturates), then y is rounded to the nearest
code, ties to the even mantissa, subnormals included. The rounding exists twice, independently: torch's CPU conversion
to float8 (round_torch) and a search in the sorted table of the finite code values (round_table); test_fp8_refs.py
asserts that they agree.

Exact GEMM tests: the integers of [-8, 8] are exact in both formats, their products are at most 64 and with K <= 4096
every partial sum stays below 2^24: any f32 summation order reproduces the float64 result bit for bit.
"""
import torch

BF16 = torch.bfloat16
FMAX = {0: 448.0, 1: 57344.0}
TORCH_DT = {0: torch.float8_e4m3fn, 1: torch.float8_e5m2}
_MBITS = {0: 3, 1: 2}
_BIAS = {0: 7, 1: 15}
TOP = {0: 0x7E, 1: 0x7B}  # code of +FMAX; the positive finite codes 0 .. TOP increase with their value
NAN_CODE = 0x7F  # a NaN code of both formats


def decode(bytes_u8, fmt):
    """uint8 codes -> float64 values (arithmetic on the bit fields; no torch float8 involved)."""
    b = bytes_u8.to(torch.int64)
    mb = _MBITS[fmt]
    sign = torch.where((b >> 7) == 1, -1.0, 1.0).double()
    e = (b >> mb) & ((1 << (7 - mb)) - 1)
    m = (b & ((1 << mb) - 1)).double() / (1 << mb)
    one = torch.ones_like(m)
    normal = torch.ldexp(1.0 + m, (e - _BIAS[fmt]).to(torch.int32))
    sub = torch.ldexp(m, ((1 - _BIAS[fmt]) * torch.ones_like(e)).to(torch.int32))
    v = torch.where(e == 0, sub, normal)
    if fmt == 0:
        v = torch.where((b & 0x7F) == 0x7F, one * float("nan"), v)
    else:
        v = torch.where(e == 31, torch.where(m == 0, one * float("inf"), one * float("nan")), v)
    return sign * v


def is_nan_code(bytes_u8, fmt):
    b = bytes_u8.to(torch.int64) & 0x7F
    return b == 0x7F if fmt == 0 else b > 0x7C


def _pos_values(fmt):
    return decode(torch.arange(TOP[fmt] + 1, dtype=torch.uint8), fmt)


def round_table(y, fmt):
    """Clamped values (float32 or float64; NaN allowed) -> uint8 codes by the table method: the nearest of the sorted
    finite code values, a tie to the code with the even mantissa (the even code: the mantissa's last bit is the
    code's)."""
    y = y.double()
    vals = _pos_values(fmt)
    a = y.abs()
    nan = torch.isnan(a)
    a = torch.where(nan, torch.zeros_like(a), a)
    assert (a <= FMAX[fmt]).all(), "round_table takes clamped values"
    hi = torch.searchsorted(vals, a.contiguous()).clamp(1, TOP[fmt])  # vals[hi - 1] <= a <= vals[hi] (a = 0: 0, 1)
    lo = hi - 1
    dlo, dhi = a - vals[lo], vals[hi] - a
    code = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi, torch.where(lo % 2 == 0, lo, hi)))
    code = code | (torch.signbit(y).to(torch.int64) << 7)
    code = torch.where(nan, torch.full_like(code, NAN_CODE), code)
    return code.to(torch.uint8)


def round_torch(y, fmt):
    """The same rounding by torch's CPU conversion (float32 in)."""
    return y.float().to(TORCH_DT[fmt]).view(torch.uint8)


def scaled(v, scale, fmt, floor=1e-30):
    """y = v * (1 / max(scale, floor)) in float32, clamped to +-FMAX, NaN kept."""
    s = torch.as_tensor(scale, dtype=torch.float32).reshape(())
    inv = torch.tensor(1.0, dtype=torch.float32) / torch.maximum(s, torch.tensor(floor, dtype=torch.float32))
    y = v.detach().float().cpu() * inv
    return torch.clamp(y, -FMAX[fmt], FMAX[fmt])  # (torch.clamp keeps NaN)


def quant_ref(v, scale, fmt, floor=1e-30):
    """The quantizers' operation on float32 (or bf16) values v with a float32 scale -> uint8 codes."""
    return round_torch(scaled(v, scale, fmt, floor), fmt)


def neighbours(code, fmt):
    """(code - 1 step, code + 1 step) along the value axis, saturating at +-FMAX (uint8 in / out)."""
    c = code.to(torch.int64)
    mag, neg = c & 0x7F, (c >> 7) == 1
    signed = torch.where(neg, -mag, mag)  # monotonic in the value (both zeros at 0)

    def enc(s):
        s = s.clamp(-TOP[fmt], TOP[fmt])
        return torch.where(s < 0, (-s) | 0x80, s).to(torch.uint8)

    return enc(signed - 1), enc(signed + 1)


def assert_bytes(name, got, ref, fmt):
    """got == ref byte for byte, NaN codes as one class (the formats have several)."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    assert got.shape == ref.shape and got.dtype == ref.dtype == torch.uint8, (name, got.shape, ref.shape)
    gn, rn = is_nan_code(got, fmt), is_nan_code(ref, fmt)
    bad = torch.nonzero((gn != rn) | (~rn & (got != ref)))
    if bad.shape[0]:
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} bytes differ; first at {at}: got "
                             f"0x{got[at].item():02X}, expected 0x{ref[at].item():02X}")


def count_adjacent(name, got, ref, fmt):
    """Every byte of got equals ref or one of its two neighbouring codes (+0 / -0 count as one code); returns how
    many differ from ref."""
    got, ref = got.detach().cpu(), ref.detach().cpu()
    lo, hi = neighbours(ref, fmt)
    z = lambda t: torch.where(t == 0x80, torch.zeros_like(t), t)  # noqa: E731
    g = z(got)
    ok = (g == z(ref)) | (g == z(lo)) | (g == z(hi))
    bad = torch.nonzero(~ok)
    if bad.shape[0]:
        at = tuple(bad[0].tolist())
        raise AssertionError(f"{name}: {bad.shape[0]} bytes are more than one code from the reference; first at {at}: "
                             f"got 0x{got[at].item():02X}, expected 0x{ref[at].item():02X}")
    return int((g != z(ref)).sum().item())


def _bf16_step(x, n):
    """The bf16 value n ulps further from zero (n = -1: nearer); x bf16, nonzero finite."""
    return (x.view(torch.int16) + n).view(BF16)


def sweep_values(fmt, scale, overflow=True):
    """(x, tie_idx, tie_code): a bf16 vector whose scaled values x / scale hit every finite code, every midpoint between
    adjacent codes (the ties; half the smallest subnormal is the first of them), each midpoint +- one bf16 ulp, +-0,
    +-FMAX and, with `overflow`, the first bf16 above FMAX, a huge finite value and +-inf. `scale` must be a power of
    two, so that every value is a bf16 (e4m3 midpoints need 4 mantissa bits, e5m2 midpoints 3; asserted). tie_idx /
    tie_code: the positions of the midpoints and the code each must land on, the even one of its two neighbours."""
    vals = _pos_values(fmt)
    codes = torch.arange(TOP[fmt] + 1, dtype=torch.int64)
    mids = (vals[:-1] + vals[1:]) / 2
    even = torch.where(codes[:-1] % 2 == 0, codes[:-1], codes[1:])

    def to_bf16(y):
        x = (y * scale).to(BF16)
        assert torch.equal(x.double(), y * scale), "sweep value not exact in bf16"
        return x

    xm = to_bf16(mids)
    parts, tie_idx, tie_code, at = [], [], [], 0
    for sign, bit in ((1.0, 0), (-1.0, 0x80)):
        seg = [to_bf16(sign * vals), sign * xm, sign * _bf16_step(xm, -1), sign * _bf16_step(xm, 1)]
        tie_idx.append(at + vals.numel() + torch.arange(mids.numel()))
        tie_code.append(even | bit)
        parts += seg
        at += sum(s.numel() for s in seg)
    if overflow:
        top = to_bf16(torch.tensor([FMAX[fmt]], dtype=torch.float64))
        parts += [_bf16_step(top, 1), -_bf16_step(top, 1), torch.tensor([3.0e38, -3.0e38]).to(BF16),
                  torch.tensor([float("inf"), float("-inf")]).to(BF16)]
    return torch.cat(parts), torch.cat(tie_idx), torch.cat(tie_code).to(torch.uint8)


def sweep_fill(shape, fmt, scale, overflow=True):
    """The sweep repeated cyclically into a bf16 tensor of `shape` (+ the tie positions / codes of its first copy,
    as flat indices)."""
    x, ti, tc = sweep_values(fmt, scale, overflow)
    n = 1
    for s in shape:
        n *= s
    reps = -(-n // x.numel())
    flat = x.repeat(reps)[:n]
    keep = ti < n
    return flat.reshape(shape).contiguous(), ti[keep], tc[keep]


def draw_ints(shape, seed, lo=-8, hi=8):
    """float64 integers drawn uniformly from [lo, hi]; 0 and both ends are always present."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(lo, hi + 1, tuple(shape), generator=g).double()
    flat = t.view(-1)
    assert flat.numel() >= 3
    pos = torch.randperm(flat.numel(), generator=g)[:3]
    flat[pos[0]], flat[pos[1]], flat[pos[2]] = 0.0, float(lo), float(hi)
    return t


def encode_exact(v64, fmt):
    """float64 values that ARE code values -> their codes (asserted)."""
    c = round_table(v64, fmt)
    assert torch.equal(decode(c, fmt), v64.double()), "value not representable"
    return c


def fp8_int_operand(shape, fmt, seed):
    """uint8 codes of integers in [-8, 8] (exact in e4m3 and e5m2), 0 and both ends always present."""
    return encode_exact(draw_ints(shape, seed), fmt)


def gelu_grad_f64(x):
    """Derivative of the tanh-GELU in float64."""
    k0, k1 = 0.7978845608028654, 0.044715
    x = x.double()
    t = torch.tanh(k0 * (x + k1 * x ** 3))
    return 0.5 * (1 + t) + 0.5 * x * (1 - t * t) * k0 * (1 + 3 * k1 * x * x)


def gelu_case(shape, seed):
    """(dy, pre) bf16 for the GELU-folded quantizer test: dy ~ N(0, 1), pre ~ N(0.75, 1). The band of gelu_band is
    relative to |dy| while an e5m2 step is relative to |dy gelu'(pre)|: its share grows like 1 / |gelu'|, and with pre
    centred on 0 (gelu' = 0.5, smaller for every negative pre) the reference alone puts 2.7% of the elements inside
    it. Centred on 0.75 the share is 1.2%, with 23% of the pre-activations still negative and 4% below -1."""
    g = torch.Generator().manual_seed(seed)
    dy = torch.randn(shape, generator=g).to(BF16)
    return dy, (torch.randn(shape, generator=g) + 0.75).to(BF16)


GELU_BAND = 2.0 ** -12  # see gelu_band
GELU_SHARE_CAP = 0.02


def gelu_band(dy, pre, scale, fmt):
    """(ref, lo, hi) codes of v = dy * gelu'(pre) computed in float64 and of v -+ 2^-12 |dy|, quantized with `scale` (a
    power of two). gelu' is O(1) and the kernel's fast exp / reciprocal err by a few f32 ulps of it, more than 100x
    below 2^-12: the kernel's byte may differ from ref only where lo or hi does (and must then be one of them)."""
    dy64 = dy.double().cpu()
    v = dy64 * gelu_grad_f64(pre.double().cpu())
    band = GELU_BAND * dy64.abs()
    q = lambda t: round_table(torch.clamp(t / scale, -FMAX[fmt], FMAX[fmt]), fmt)  # noqa: E731
    return q(v), q(v - band), q(v + band), v
