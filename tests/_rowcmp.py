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


# ------------------------------------------------------------------ per-channel helpers (batch norm, pooling)
def check_chans(name, out, ref, tol, worst=None, base=None):
    """check_rows per CHANNEL of channels-last tensors: [..., C] is flattened to [M, C] and transposed, so err_c =
    max_m |out - ref| / max(max_m |ref_c|, floor) with the same floor (one bf16 ulp of the tensor's largest value)."""
    C = ref.shape[-1]
    assert out.shape == ref.shape, (out.shape, ref.shape)
    return check_rows(name, out.detach().reshape(-1, C).t(), ref.detach().reshape(-1, C).t(), tol, worst, base)


def check_sums(name, out, ref, scale, tol=1e-4, worst=None):
    """f32 per-channel reductions: |out_c - ref_c| <= tol * scale_c, scale_c the float64 sum of the absolute values of
    channel c's terms (what an f32 summation in any order can lose). Records the worst |err| / scale."""
    out, ref, scale = (t.detach().double().cpu().reshape(-1) for t in (out, ref, scale))
    assert out.shape == ref.shape == scale.shape, (out.shape, ref.shape, scale.shape)
    assert torch.isfinite(out).all(), f"{name}: non-finite output"
    err = (out - ref).abs()
    ratio = err / scale.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    w = ratio.max().item() if ratio.numel() else 0.0
    print(f"  {name}: worst |err| / scale {w:.3e} (bound {tol:.1e})")
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), w)
    bad = torch.nonzero(err > tol * scale)
    assert bad.numel() == 0, (f"{name}: channel {bad[0].item()} off by {err[bad[0]].item():.3e} > "
                              f"{tol:.1e} * {scale[bad[0]].item():.3e}")
    return w


def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def _pool_geo(H, W, k, s, p):
    (R, S), (sh, sw), (ph, pw) = _pair(k), _pair(s), _pair(p)
    return R, S, sh, sw, ph, pw, (H + 2 * ph - R) // sh + 1, (W + 2 * pw - S) // sw + 1


def maxpool_first(x, k, s, p):
    """Max pool of a channels-last [N,H,W,C] tensor with -inf padding. The taps are walked in (r, s) order and a
    later tap replaces the best only when strictly greater: the FIRST maximal tap wins, maxpool_fwd_kernel's rule
    (nothing here depends on how PyTorch breaks ties). Returns (values in x's dtype, tap index r*S+s as int64),
    both [N,P,Q,C]."""
    N, H, W, C = x.shape
    R, S, sh, sw, ph, pw, P, Q = _pool_geo(H, W, k, s, p)
    xp = torch.full((N, H + 2 * ph, W + 2 * pw, C), NEG, dtype=torch.float64, device=x.device)
    xp[:, ph:ph + H, pw:pw + W] = x.double()
    best = torch.full((N, P, Q, C), NEG, dtype=torch.float64, device=x.device)
    idx = torch.zeros((N, P, Q, C), dtype=torch.int64, device=x.device)
    for r in range(R):
        for c in range(S):
            v = xp[:, r:r + (P - 1) * sh + 1:sh, c:c + (Q - 1) * sw + 1:sw]
            upd = v > best
            best = torch.where(upd, v, best)
            idx = torch.where(upd, torch.full_like(idx, r * S + c), idx)
    return best.to(x.dtype), idx


def maxpool_scatter(dy, idx, H, W, k, s, p):
    """float64 gradient of maxpool_first: every pooled gradient goes to the input pixel its tap index names."""
    N, P, Q, C = dy.shape
    R, S, sh, sw, ph, pw, P2, Q2 = _pool_geo(H, W, k, s, p)
    assert (P, Q) == (P2, Q2), (P, Q, P2, Q2)
    dxp = torch.zeros((N, H + 2 * ph, W + 2 * pw, C), dtype=torch.float64, device=dy.device)
    for r in range(R):
        for c in range(S):
            dxp[:, r:r + (P - 1) * sh + 1:sh, c:c + (Q - 1) * sw + 1:sw] += dy.double() * (idx == r * S + c)
    return dxp[:, ph:ph + H, pw:pw + W].contiguous()


class BNRef:
    """Result of bn_f64 (float64 CPU tensors; the backward fields are None without dy)."""
    y = mean = var = invstd = xhat = mask = None
    dz = dx = dgamma = dbeta = dres = dgamma_scale = dbeta_scale = None


def bn_f64(x, gamma, beta, eps, res=None, relu=False, dy=None):
    """float64 training batch norm over all but the last axis of the (already bf16-rounded) x, y = [relu](gamma * xhat
    + beta [+ res]), and for a given dy its gradients: dz = dy where the ReLU passed, dbeta = sum dz, dgamma = sum
    dz * xhat, dx = gamma * invstd * (dz - dbeta / M - xhat * dgamma / M), dres = dz. The ReLU mask is taken from the
    bf16-rounded output, as the kernel's mask bits are (f2bf(o) != 0 && o > 0). var is the biased batch variance;
    dgamma_scale / dbeta_scale are the sums of |terms| for check_sums."""
    o = BNRef()
    xd = x.detach().double().cpu()
    C = xd.shape[-1]
    x2 = xd.reshape(-1, C)
    M = x2.shape[0]
    g = torch.ones(C, dtype=torch.float64) if gamma is None else gamma.detach().double().cpu()
    b = torch.zeros(C, dtype=torch.float64) if beta is None else beta.detach().double().cpu()
    o.mean = x2.mean(0)
    o.var = ((x2 - o.mean) ** 2).mean(0)
    o.invstd = torch.rsqrt(o.var + eps)
    o.xhat = (x2 - o.mean) * o.invstd
    y = o.xhat * g + b
    if res is not None:
        y = y + res.detach().double().cpu().reshape(-1, C)
    o.mask = torch.ones_like(y, dtype=torch.bool)
    if relu:
        y = torch.relu(y)
        o.mask = bf16_round(y) > 0
    o.y = y.reshape(xd.shape)
    if dy is not None:
        dz = dy.detach().double().cpu().reshape(-1, C) * o.mask
        o.dbeta, o.dbeta_scale = dz.sum(0), dz.abs().sum(0)
        o.dgamma, o.dgamma_scale = (dz * o.xhat).sum(0), (dz * o.xhat).abs().sum(0)
        o.dx = (g * o.invstd * (dz - o.dbeta / M - o.xhat * o.dgamma / M)).reshape(xd.shape)
        o.dz = dz.reshape(xd.shape)
        o.dres = o.dz if res is not None else None
    return o


# (H, W, kernel, stride, pad) of the max-pool edge tests: odd maps, pad 0, overlapping stride-1 windows, stride ==
# kernel, the 1x1 identity and a rectangular window with rectangular stride / pad
POOL_GEOS = [(7, 7, 3, 2, 1), (8, 6, 2, 2, 0), (5, 9, 3, 1, 1), (6, 6, 3, 3, 0), (4, 4, 1, 1, 0),
             (9, 7, (3, 2), (2, 1), (1, 0))]


def maxpool_unique(x, k, s, p):
    """[N,P,Q,C] bool: exactly one tap of the window holds its maximum (the winning tap does not depend on a tie rule)."""
    N, H, W, C = x.shape
    R, S, sh, sw, ph, pw, P, Q = _pool_geo(H, W, k, s, p)
    xp = torch.full((N, H + 2 * ph, W + 2 * pw, C), NEG, dtype=torch.float64, device=x.device)
    xp[:, ph:ph + H, pw:pw + W] = x.double()
    best = maxpool_first(x, k, s, p)[0].double()
    n = torch.zeros((N, P, Q, C), dtype=torch.int64, device=x.device)
    for r in range(R):
        for c in range(S):
            n += xp[:, r:r + (P - 1) * sh + 1:sh, c:c + (Q - 1) * sw + 1:sw] == best
    return n == 1


def chan_base(ref):
    """Worst per-channel err of the float64 reference rounded to bf16: what bf16 storage alone costs."""
    C = ref.shape[-1]
    r = ref.detach().double().cpu().reshape(-1, C).t()
    return row_err(bf16_round(r), r).max().item()
