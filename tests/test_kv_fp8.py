"""The fp8 KV-cache format on the CPU: kv_quantize_reference, the CPU fp8 cache, generate(kv_dtype="fp8") in f32."""
import pytest
import torch

from _fp8ref import decode
from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops.decode import kv_quantize_reference

BF = torch.bfloat16
TOP = 448.0 * 8                                     # 1.75 * 2^11: m = 1.75, e = x - 8 = 3
ABOVE = (torch.tensor(TOP).to(BF).view(torch.int16) + 1).view(BF).float().item()   # the next bf16: e = x - 7 = 4
# (amax, e, code of the amax element): zeros, m = 1.75, just above it, and the clamp e = -64 (2^-26 rounds to code 0)
EDGES = [(0.0, 0, 0x00), (TOP, 3, 0x7E), (ABOVE, 4, 0x76), (2.0 ** -90, -64, 0x00)]


def edge_rows():
    """[4, 64] f32: the four edge rows of the store tests, each amax at column 7 with smaller random values around it."""
    g = torch.Generator().manual_seed(0)
    x = torch.rand(4, 64, generator=g).to(BF).float() * torch.tensor([a for a, _, _ in EDGES])[:, None] * 0.5
    x[:, 7] = torch.tensor([a for a, _, _ in EDGES])
    return x.to(BF).float()


def test_quantize_reference_edge_rows():
    x = edge_rows()
    codes, scale = kv_quantize_reference(x)
    assert codes.dtype == torch.uint8 and scale.dtype == torch.float32
    assert scale.tolist() == [2.0 ** e for _, e, _ in EDGES]
    assert codes[:, 7].tolist() == [c for _, _, c in EDGES]
    deq = decode(codes, 0) * scale[:, None].double()
    cache = ops.KVCache(1, 1, 2, 64, "cpu", kv_dtype="fp8")
    qkv = torch.cat([torch.zeros(2, 64), x[:2], x[2:]]).reshape(1, 1, 6 * 64)   # [q | k | v] of two heads
    cache.store(0, qkv)
    K, V = cache.dequantized(0)
    assert torch.equal(K[0, :, 0].double(), deq[:2]) and torch.equal(V[0, :, 0].double(), deq[2:])
    nan = torch.full((1, 64), float("nan"))
    nan[0, 1], nan[0, 2] = float("inf"), -3.0
    c, s = kv_quantize_reference(nan)
    assert c[0, :3].tolist() == [0x7F, 0x7E, 0xFC] and s.item() == 2.0 ** -7   # amax 3 = 1.5 * 2^1: e = -7, -384


def test_generate_fp8_cache_on_the_cpu():
    with context.device("cpu"):
        initializers.set_seed(0)
        torch.manual_seed(0)
        model = GPT2(vocab=200, ctx=96, hidden=128, layers=2, heads=2)
        ids = torch.randint(0, 200, (2, 5))
        out = model.generate(ids, 8, kv_dtype="fp8")
        g8 = model.last_generation
        model.generate(ids, 8)
        g16 = model.last_generation
        with pytest.raises(ValueError):
            model.generate(ids, 8, kv_dtype="int8")
        with pytest.raises(ValueError):
            model.generate(ids[:, :1], 1, cache=g16["cache"], kv_dtype="fp8")
    assert tuple(out.shape) == (2, 13)
    assert g8["cache"].kv_dtype == "fp8" and g16["cache"].kv_dtype == "bf16"
    assert g8["cache"].lens.tolist() == [13, 13] and g16["cache"].lens.tolist() == [13, 13]
    a, b = g8["logits"].float(), g16["logits"].float()
    assert not torch.equal(a, b), "the fp8 cache did not round anything"
    assert (a - b).abs().max() <= 0.25 * b.abs().max(), ((a - b).abs().max(), b.abs().max())
