"""3x3 weight gradients into >= 256 output channels on the 4-wave MFMA kernel (csrc/kernels/gemm_w4.hip with the
gathered K-outer X loader W4GatherK of gemm_w4.h): dW = dY^T . X(gathered), split-K over the output pixels into f32
slabs summed in a fixed order, with the split count of the general tiles so that the result is bit for bit theirs.
dtf_conv_wgrad takes the route for splits of >= 128 K-tiles (DTF_W4_WGRAD3 / dtf_set_w4_wgrad3 is the A/B switch);
dtf_conv_wgrad3_w4 is the same route whatever the split length, which is how the small shapes below reach it.

Checked against a plain PyTorch fp32 reference (exact bf16 products with f32 sums in another order: the bound of
tests/test_c3_wgrad_gpu.py) and, bitwise, against the general tiles (switch off). The route that ran is asserted with
the launch counters. The route needs a pixel count that is a multiple of 64 (the batch sizes below are chosen for
that) and >= 256 output channels; other shapes must reach the general tiles. The last test covers the guard of the
64-channel persistent kernel (c3wgrad.hip) for images shorter than 3 rows. The reference's op is the Conv2D weight
gradient of the ResNet-50 trainer (trainer/task.py:62-71)."""
import pytest
import torch
import torch.nn.functional as F

from distributed_tensorflow_amd.ops._util import call, launch_counts, launch_delta, ptr, stream, workspace

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
LC_W4_256, LC_W4_128 = "w4_256", "w4_128"  # ops._util.LAUNCH_COUNTERS


def _out_hw(H, s):
    return (H + 2 - 3) // s + 1


def _inputs(cuda, N, H, W, C, K, s, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed + N * 1000 + H * 10 + W + C + K)
    x = torch.randn(N, H, W, C, generator=g).to(BF).to(cuda)
    dy = torch.randn(N, _out_hw(H, s), _out_hw(W, s), K, generator=g).to(BF).to(cuda)
    return x, dy


def _ref(x, dy, s):
    """dW [K][3][3][C] in fp32: per tap, the einsum of dY with the shifted, strided, zero-padded X."""
    N, H, W, C = x.shape
    P, Q, K = dy.shape[1], dy.shape[2], dy.shape[3]
    xp = F.pad(x.float(), (0, 0, 1, 1, 1, 1))
    out = torch.empty(K, 3, 3, C, device=x.device)
    d = dy.float()
    for a in range(3):
        for b in range(3):
            out[:, a, b, :] = torch.einsum("npqk,npqc->kc", d, xp[:, a:a + (P - 1) * s + 1:s, b:b + (Q - 1) * s + 1:s, :])
    return out


def _geom(x, dy, s):
    N, H, W, C = x.shape
    return (N, H, W, C, dy.shape[3], 3, 3, dy.shape[1], dy.shape[2], s, s, 1, 1)


def _wgrad(x, dy, s, on, out=None):
    """dtf_conv_wgrad with the default routing and the switch on / off; returns (dW, launch-count delta)."""
    call("dtf_set_w4_wgrad3", 1 if on else 0)
    try:
        K, C = dy.shape[3], x.shape[3]
        dw = out.clone() if out is not None else torch.full((K, 3, 3, C), float("nan"), device=x.device)
        ws = workspace(x.device)
        before = launch_counts()
        call("dtf_conv_wgrad", ptr(x), ptr(dy), ptr(dw), *_geom(x, dy, s), 1, 1, int(out is not None), 0, -1, ptr(ws),
             ws.numel(), stream())
        torch.cuda.synchronize()
        return dw, launch_delta(before)
    finally:
        call("dtf_set_w4_wgrad3", 1)


def _direct(x, dy, s, bn, splitk, out=None):
    """The 4-wave route with a forced tile width and split count."""
    K, C = dy.shape[3], x.shape[3]
    dw = out.clone() if out is not None else torch.full((K, 3, 3, C), float("nan"), device=x.device)
    ws = workspace(x.device)
    before = launch_counts()
    call("dtf_conv_wgrad3_w4", ptr(x), ptr(dy), ptr(dw), *_geom(x, dy, s), int(out is not None), splitk, bn, ptr(ws),
         ws.numel(), stream())
    torch.cuda.synchronize()
    return dw, launch_delta(before)


def _w4(delta):
    return delta[LC_W4_256] + delta[LC_W4_128]


def _close(got, ref):
    err = (got - ref).abs().max().item()
    bound = 2e-5 * ref.abs().max().item() + 1e-3
    print(f"max|diff| {err:.3e} bound {bound:.3e}")
    return err <= bound


# (N, H, W, C, Kout, stride): pixel counts N*P*Q are multiples of 64
SHAPES = [
    (64, 3, 5, 128, 256, 1),     # many image boundaries inside one 64-pixel K-tile, every tap masked somewhere
    (128, 1, 1, 128, 256, 1),    # one-pixel images: only the centre tap is non-zero
    (4, 8, 8, 256, 256, 2),      # stride 2, even extent
    (64, 9, 9, 256, 256, 2),     # stride 2, odd extent (5 x 5 outputs)
    (16, 14, 14, 128, 256, 1),   # 9C = 1152: 4.5 column tiles of 256
    (16, 14, 14, 256, 384, 1),   # second M-tile half empty
    (16, 14, 14, 512, 512, 1),   # several M and N tiles
    (16, 14, 14, 192, 256, 1),   # C % 128 != 0
]


@pytest.mark.parametrize("N,H,W,C,K,s", SHAPES)
def test_w4_wgrad3_matches_reference_and_general_tiles(cuda, N, H, W, C, K, s):
    x, dy = _inputs(cuda, N, H, W, C, K, s)
    ref = _ref(x, dy, s)
    new, d_on = _direct(x, dy, s, 0, 0)
    gen, d_off = _wgrad(x, dy, s, False)
    assert _w4(d_on) == 1 and _w4(d_off) == 0
    assert _close(new, ref)
    assert _close(new, gen)
    # the route keeps the general tiles' split count: the same accumulation chains, bit for bit the same gradient
    assert torch.equal(new, gen)


def test_one_pixel_images_leave_the_outer_taps_exactly_zero(cuda):
    x, dy = _inputs(cuda, 128, 1, 1, 128, 256, 1)
    new, d = _direct(x, dy, 1, 0, 0)
    assert _w4(d) == 1
    outer = new.clone()
    outer[:, 1, 1, :] = 0
    assert torch.count_nonzero(outer).item() == 0
    assert torch.count_nonzero(new[:, 1, 1, :]).item() > 0


@pytest.mark.parametrize("N,C,K,bn", [(16, 128, 256, 256), (16, 128, 256, 128), (16, 192, 256, 256)])
def test_forced_tile_width_column_tile_spans_two_taps(cuda, N, C, K, bn):
    # C = 128 with 256-wide column tiles: every tile holds two taps; C = 192: taps start inside tiles
    x, dy = _inputs(cuda, N, 14, 14, C, K, 1)
    got, d = _direct(x, dy, 1, bn, 1)
    assert d[LC_W4_256 if bn == 256 else LC_W4_128] == 1
    assert _close(got, _ref(x, dy, 1))


@pytest.mark.parametrize("N,H,C,K,splitk", [
    (16, 14, 256, 256, 3),   # 49 K-tiles in 3 splits: 17, 17, 15 (the last one short)
    (16, 14, 256, 256, 5),   # 10, 10, 10, 10, 9
    (16, 14, 128, 256, 4),   # 13, 13, 13, 10
    (4, 8, 256, 256, 7),     # 4 K-tiles in 7 splits: three of them empty
])
def test_split_k_uneven_chunks(cuda, N, H, C, K, splitk):
    x, dy = _inputs(cuda, N, H, H, C, K, 1)
    got, d = _direct(x, dy, 1, 0, splitk)
    assert _w4(d) == 1
    assert _close(got, _ref(x, dy, 1))


def test_accumulates_and_is_deterministic(cuda):
    x, dy = _inputs(cuda, 16, 14, 14, 256, 256, 1)
    base = torch.randn(256, 3, 3, 256, device=cuda)
    ref = _ref(x, dy, 1) + base
    a, d = _direct(x, dy, 1, 0, 0, base)
    b, _ = _direct(x, dy, 1, 0, 0, base)
    assert _w4(d) == 1
    assert torch.equal(a, b)
    assert _close(a, ref)
    assert torch.equal(a, _wgrad(x, dy, 1, False, base)[0])
    for splitk in (1, 3):
        c, _ = _direct(x, dy, 1, 256, splitk, base)
        e, _ = _direct(x, dy, 1, 256, splitk, base)
        assert torch.equal(c, e)
        assert _close(c, ref)


@pytest.mark.parametrize("N,H,W,C,K", [
    (3, 7, 9, 128, 256),   # 189 pixels: not a multiple of 64
    (4, 8, 8, 128, 128),   # 128 output channels (the swapped form lost to the general tiles and is not built)
])
def test_shapes_the_route_does_not_take_reach_the_general_tiles(cuda, N, H, W, C, K):
    x, dy = _inputs(cuda, N, H, W, C, K, 1)
    got, d = _wgrad(x, dy, 1, True)
    assert _w4(d) == 0
    assert _close(got, _ref(x, dy, 1))
    dw = torch.zeros(K, 3, 3, C, device=cuda)
    ws = workspace(cuda)
    with pytest.raises(RuntimeError, match="status -2"):  # the direct entry: not eligible, nothing launched
        call("dtf_conv_wgrad3_w4", ptr(x), ptr(dy), ptr(dw), *_geom(x, dy, 1), 0, 0, 0, ptr(ws), ws.numel(), stream())


def test_default_routing_takes_the_route_for_long_splits_only(cuda):
    # 125440 pixels in the general tiles' 15 splits: 131 K-tiles a split -> the 4-wave route, bitwise the general tiles
    x, dy = _inputs(cuda, 640, 14, 14, 256, 256, 1)
    new, d_on = _wgrad(x, dy, 1, True)
    gen, d_off = _wgrad(x, dy, 1, False)
    assert _w4(d_on) == 1 and _w4(d_off) == 0
    assert torch.equal(new, gen)
    assert _close(new, _ref(x, dy, 1))
    # 3136 pixels: short splits stay on the general tiles
    x, dy = _inputs(cuda, 16, 14, 14, 256, 256, 1)
    _, d = _wgrad(x, dy, 1, True)
    assert _w4(d) == 0


@pytest.mark.parametrize("N,H", [(1024, 1), (512, 2)])
def test_c3_wgrad_guard_short_images(cuda, N, H):
    # 64 -> 64 channels with images shorter than 3 rows: the persistent kernel's X ring does not cover them, the
    # default routing must give the right gradient (general tiles)
    x, dy = _inputs(cuda, N, H, H, 64, 64, 1)
    dw = torch.full((64, 3, 3, 64), float("nan"), device=cuda)
    ws = workspace(cuda)
    call("dtf_conv_wgrad", ptr(x), ptr(dy), ptr(dw), *_geom(x, dy, 1), 1, 1, 0, 0, -1, ptr(ws), ws.numel(), stream())
    torch.cuda.synchronize()
    assert _close(dw, _ref(x, dy, 1))
