"""Per-row comparison against float64 references (shared by test_softmax_family_gpu.py and test_attention_edges_gpu.py).

A tensor-wide max-error check lets one wrong row of ordinary magnitude pass when another row is large, so errors are
measured per last-axis vector: err_r = max_i |out - ref| / max(max_i |ref_r|, floor), where floor is one bf16 ulp
(2^-8) of the tensor's largest reference value, which keeps rows whose reference is all zero in the comparison.

The references are plain PyTorch in float64 on the already-rounded inputs. A softmax row with no visible key is
DEFINED as 0 (output and gradient): what the kernels write for it.
"""
import math

import torch

ULP = 2.0 ** -8   # one bf16 ulp, relative
NEG = float("-inf")
LOG2E = 1.0 / math.log(2.0)


def row_err(out, ref):
    """Per-row relative error (float64 CPU tensor of shape out.shape[:-1]); every element of out must be finite."""
    assert out.shape == ref.shape, (out.shape, ref.shape)
    assert torch.isfinite(out).all(), "non-finite output"
    out, ref = out.detach().double().cpu(), ref.detach().double().cpu()
    floor = ref.abs().max().item() * ULP
    den = ref.abs().amax(-1).clamp_min(max(floor, 1e-300))
    return (out - ref).abs().amax(-1) / den


def check_rows(name, out, ref, tol, worst=None, base=None):
    """Assert err_r <= tol for every row; prints (and records in `worst`) the largest one. base: the rounded baseline's
    own worst err_r, printed with the ratio to it."""
    err = row_err(out, ref)
    w = err.max().item() if err.numel() else 0.0
    note = "" if base is None else f", rounded baseline {base:.3e}, ratio {w / max(base, 1e-300):.2f}"
    print(f"  {name}: worst err_r {w:.3e} (bound {tol:.1e}{note})")
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), w)
    where = tuple(torch.nonzero(err == err.max())[0].tolist()) if err.numel() else ()
    assert w <= tol, f"{name}: worst row error {w:.3e} > {tol:.1e} at row {where}"
    return w


def dead_softmax(z):
    """float64 softmax over the last axis of -inf-masked scores; rows with no visible key are 0."""
    dead = (z == NEG).all(-1, keepdim=True)
    return torch.softmax(z.masked_fill(dead, 0.0), -1).masked_fill(dead, 0.0), dead


def causal_keep(Sq, Sk, device):
    """[Sq, Sk] bool: key j visible to query i (the last query sees the last key)."""
    return torch.ones(Sq, Sk, dtype=torch.bool, device=device).tril(Sk - Sq)


def bf16_round(t):
    """float64 -> nearest bf16 -> float64."""
    return t.float().bfloat16().double()


def attention_rounded(q, k, v, do, causal=False, mask=None, scale=None, keep_mask=None, keep=1.0, composed=False):
    """The same float64 attention with bf16 rounding applied where the kernels round, computed on the CPU; its own
    err_r against attention_f64 is what bf16 storage alone costs at a shape, whatever the kernel.

    Flash kernels: the probabilities are rounded before P V as exp(s - m) with m the running row maximum after the
    64-key tile they belong to (normalised by the f32 row sum afterwards), dS is rounded before the dQ / dK products,
    and O, dQ, dK, dV are rounded; D = rowsum(dO * O) reads the rounded O. composed: the batched-GEMM route stores the
    raw scores Q K^T, the normalised probabilities, dP and the softmax gradient in bf16."""
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    q, k, v, do = (t.detach().double().cpu() for t in (q, k, v, do))
    s = torch.matmul(q, k.transpose(-1, -2))
    if composed:
        s = bf16_round(s)
    s = s * scale
    if causal:
        s = s.masked_fill(~causal_keep(Sq, Sk, s.device), NEG)
    if mask is not None:
        s = s + mask.reshape(B, 1, 1, Sk).double().cpu()
    p, dead = dead_softmax(s)
    drop = 1.0 if keep_mask is None else keep_mask.double().cpu() / keep
    if composed:
        p = bf16_round(p)
        pb = bf16_round(p * drop)
    else:
        nt = (Sk + 63) // 64
        tmax = torch.stack([s[..., t * 64:(t + 1) * 64].amax(-1) for t in range(nt)], -1)
        run = torch.cummax(tmax, -1).values                        # running maximum after each key tile
        top = run[..., -1:]
        m = run.repeat_interleave(64, -1)[..., :Sk]
        m, top = m.masked_fill(m == NEG, 0.0), top.masked_fill(top == NEG, 0.0)
        rowsum = torch.exp(s - top).sum(-1, keepdim=True).clamp_min(1e-300)
        pb = (bf16_round(torch.exp(s - m)) * torch.exp(m - top) / rowsum).masked_fill(dead, 0.0) * drop
    o = bf16_round(torch.matmul(pb, v))
    dp = torch.matmul(do, v.transpose(-1, -2)) * drop
    if composed:
        dp = bf16_round(dp)
        dvec = (dp * p).sum(-1, keepdim=True)
    else:
        dvec = (do * o).sum(-1, keepdim=True)
    ds = bf16_round(p * (dp - dvec) * (scale if composed else 1.0))
    post = 1.0 if composed else scale
    dq = bf16_round(torch.matmul(ds, k) * post)
    dk = bf16_round(torch.matmul(ds.transpose(-1, -2), q) * post)
    dv = bf16_round(torch.matmul(pb.transpose(-1, -2), do))
    return o, dq, dk, dv


def softmax_bwd_rounded(y, dy, scale):
    """float64 softmax gradient from the bf16-rounded probabilities the backward kernel is given, rounded to bf16."""
    yb = bf16_round(y)
    return bf16_round(scale * yb * (dy - (dy * yb).sum(-1, keepdim=True)))


def attention_f64(q, k, v, do, causal=False, mask=None, scale=None, keep_mask=None, keep=1.0):
    """float64 attention of [B,H,S,D] tensors and its gradients for the output gradient `do`.

    Returns (o, dq, dk, dv, lse2, dead): lse2 is the row logsumexp in log2 units (+inf for rows with no visible key,
    the kernel's convention), dead the [B,H,Sq,1] mask of those rows. keep_mask / keep: dropout on the probabilities.
    """
    B, H, Sq, D = q.shape
    Sk = k.shape[2]
    scale = scale if scale is not None else 1.0 / math.sqrt(D)
    q, k, v = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    s = torch.matmul(q, k.transpose(-1, -2)) * scale
    if causal:
        s = s.masked_fill(~causal_keep(Sq, Sk, s.device), NEG)
    if mask is not None:
        s = s + mask.reshape(B, 1, 1, Sk).double()
    p, dead = dead_softmax(s)
    lse2 = torch.logsumexp(s.detach().masked_fill(dead, 0.0), -1) * LOG2E
    lse2 = lse2.masked_fill(dead[..., 0], float("inf"))
    if keep_mask is not None:
        p = p * keep_mask.double() / keep
    o = torch.matmul(p, v)
    dq, dk, dv = torch.autograd.grad(o, [q, k, v], do.double())
    return o.detach(), dq, dk, dv, lse2, dead
