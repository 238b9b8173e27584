"""The CPU paths agree with the kernels on the rows the kernels define specially: a negative label is an ignored
cross-entropy row (loss 0, gradient 0), and a softmax / attention row with no visible key is 0 with a finite (zero)
gradient, not NaN."""
import importlib

import torch

from distributed_tensorflow_amd import ops

A = importlib.import_module("distributed_tensorflow_amd.ops.mha")
NEG = float("-inf")


def test_cpu_cross_entropy_ignores_every_negative_label():
    torch.manual_seed(0)
    x = torch.randn(6, 11)
    lab = torch.tensor([3, -1, 0, -100, 10, -7])
    out = {}
    for fill in (-1, -100):
        xs = x.clone().requires_grad_(True)
        l = ops.sparse_softmax_cross_entropy(xs, torch.where(lab < 0, torch.full_like(lab, fill), lab),
                                             label_smoothing=0.1)
        (l * torch.arange(1.0, 7.0)).sum().backward()
        out[fill] = (l.detach(), xs.grad)
    l, g = out[-1]
    assert torch.equal(l, out[-100][0]) and torch.equal(g, out[-100][1])
    ign = lab < 0
    assert (l[ign] == 0).all() and (g[ign] == 0).all()
    ref = torch.nn.functional.cross_entropy(x[~ign], lab[~ign], reduction="none", label_smoothing=0.1)
    assert torch.allclose(l[~ign], ref, rtol=1e-6, atol=1e-6)
    assert (g[~ign].abs().amax(-1) > 0).all()
    # mixed shapes: labels [2, 3] against logits [2, 3, V]
    l2 = ops.sparse_softmax_cross_entropy(x.reshape(2, 3, 11), lab.reshape(2, 3), label_smoothing=0.1)
    assert l2.shape == (2, 3) and torch.equal(l2.reshape(-1), l)


def test_cpu_softmax_empty_rows_are_zero():
    torch.manual_seed(1)
    x = torch.randn(3, 9, 5, requires_grad=True)
    y = ops.softmax(x, scale=0.7, causal=True)  # Sq > Sk: the first four queries see no key
    assert torch.isfinite(y).all()
    assert (y[:, :4] == 0).all()
    assert torch.allclose(y[:, 4:].sum(-1), torch.ones(3, 5), atol=1e-6)
    assert torch.allclose(y[:, 4, 1:], torch.zeros(3, 4)) and torch.allclose(y[:, 4, 0], torch.ones(3))
    (g,) = torch.autograd.grad(y, x, torch.randn_like(y))
    assert torch.isfinite(g).all() and (g[:, :4] == 0).all() and g[:, 5:].abs().max() > 0
    am = torch.zeros(3, 5)
    am[1] = NEG
    am[2, 3:] = NEG
    x2 = torch.randn(3, 4, 5, requires_grad=True)
    y2 = ops.softmax(x2, add_mask=am)
    assert torch.isfinite(y2).all() and (y2[1] == 0).all() and (y2[2, :, 3:] == 0).all()
    assert torch.allclose(y2[0], torch.softmax(x2[0].detach(), -1), atol=1e-6)
    assert torch.allclose(y2[2, :, :3], torch.softmax(x2[2, :, :3].detach(), -1), atol=1e-6)
    (g2,) = torch.autograd.grad(y2, x2, torch.randn_like(y2))
    assert torch.isfinite(g2).all() and (g2[1] == 0).all()


def _attn_cases():
    torch.manual_seed(2)
    B, H, D = 2, 2, 8
    mask = torch.zeros(B, 7)
    mask[1] = NEG
    yield "causal Sq > Sk", 6, 4, True, None, (slice(None), slice(None), slice(0, 2))
    yield "fully masked batch entry", 5, 7, False, mask, (slice(1, 2),)


def test_cpu_attention_empty_rows_are_zero():
    for name, Sq, Sk, causal, mask, dead in _attn_cases():
        q = torch.randn(2, 2, Sq, 8, requires_grad=True)
        k = torch.randn(2, 2, Sk, 8, requires_grad=True)
        v = torch.randn(2, 2, Sk, 8, requires_grad=True)
        do = torch.randn(2, 2, Sq, 8)
        for fn in (ops.attention, A.reference_attention):
            o = fn(q, k, v, causal=causal, mask=mask)
            assert torch.isfinite(o).all(), (name, fn.__name__)
            assert (o[dead] == 0).all(), (name, fn.__name__)
            live = torch.ones(2, 2, Sq, dtype=torch.bool)
            live[dead] = False
            assert (o[live].abs().amax(-1) > 0).all(), (name, fn.__name__)
            grads = torch.autograd.grad(o, [q, k, v], do)
            for g in grads:
                assert torch.isfinite(g).all(), (name, fn.__name__)
            assert (grads[0][dead] == 0).all(), (name, fn.__name__)
            assert all(g.abs().max() > 0 for g in grads), (name, fn.__name__)
        if mask is not None:  # the other batch entry is the plain attention of its own keys
            r = torch.softmax(q[0] @ k[0].transpose(-1, -2) / 8 ** 0.5, -1) @ v[0]
            assert torch.allclose(ops.attention(q, k, v, mask=mask)[0], r, atol=1e-5)
