"""The flash attention kernels (csrc/kernels/attention.hip, D = 64) at their edges, against a float64 reference:
one query / one key, shapes under one tile, three causal query blocks with a ragged last tile, queries with no visible
key (causal with Sq > Sk, -inf key masks over whole tiles or a whole batch entry), causal together with a key mask,
dropout with Sk % 4 != 0, an explicit scale, and the packed-QKV entry point with causal masking.

Every case checks O, dQ, dK, dV and the saved lse, with both backward routes (the recompute dQ kernel and the dS^T
scratch), on B*H = 3 or 6 (grids that are no multiple of the 8 XCDs). Errors are per row (tests/_rowcmp.py) against
the project's attention tolerances: 2e-2 forward, 3e-2 gradients. Rows with no visible key are exactly 0 (O, dQ) with
lse = +inf.

One case needs more than the project tolerance, and takes it from the rounded baseline (_rowcmp.attention_rounded: the
float64 reference with bf16 rounding where the kernels round, evaluated on the CPU, never from the kernels' output):
causal Sq = 130, Sk = 70, where query 61 sees two keys and its dQ (row maximum 0.016 against 2.6 for the tensor)
is the difference of two nearly equal terms, D = rowsum(dO * O) being read from the bf16 O. The baseline's own worst
row there is err_r = 1.19e-1 for dQ, so the bound is 2 x that + 2^-8 = 0.24 (2 x: another summation order); measured
on the GPU 1.19e-1 on both backward routes, ratio 1.00. Every other case and tensor meets 2e-2 / 3e-2 per row; the
worst measured there: O 5.3e-3, dQ 2.4e-2, dK 1.9e-2, dV 6.7e-3; packed O 4.7e-3, dQKV 7.6e-3.

lse is compared in log2 units to 1e-3 * max(1, |ref|): the scores are f32 MFMA sums of 64 exact bf16
products and the exp2 / log2 instructions are good to an ulp, so this is > 100x the expected error.
"""
import importlib

import pytest
import torch

from distributed_tensorflow_amd import ops
from distributed_tensorflow_amd.ops._util import call_log

from _rowcmp import NEG, ULP, attention_f64, attention_rounded, check_rows, row_err
from test_attention import keep_mask

A = importlib.import_module("distributed_tensorflow_amd.ops.mha")

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
TOL_FWD, TOL_GRAD = 2e-2, 3e-2
_WORST = {}


def _check_lse(lse, ref, dead):
    lse, ref, dead = lse.double().cpu().reshape(ref.shape), ref.cpu(), dead.cpu()[..., 0]
    assert (lse[dead] == float("inf")).all(), "lse of a row with no visible key must be +inf"
    assert torch.isfinite(lse[~dead]).all()
    err = ((lse - ref)[~dead].abs() / ref[~dead].abs().clamp_min(1.0))
    w = err.max().item() if err.numel() else 0.0
    _WORST["lse"] = max(_WORST.get("lse", 0.0), w)
    assert w <= 1e-3, f"lse error {w:.3e}"


def _zero_ref_floor(do, v, other, scale):
    """Sk = 1: the softmax of one key has no gradient, so the dQ / dK reference is identically 0 and has no ulp of its
    own. The kernel forms dS = P (dP - D) from dP = dO.V and D = dO.O, two f32 sums of the same terms in another order;
    the floor is then one bf16 ulp of the magnitude of those cancelling terms times the operand dS multiplies."""
    return ULP * scale * (do.double() * v.double()).abs().sum(-1).max().item() * other.double().abs().max().item()


def _run(cuda, monkeypatch, B, H, Sq, Sk, causal, mask=None, scale=None, dropout=0.0, seed=11, baseline=False):
    g = torch.Generator().manual_seed(Sq * 1009 + Sk * 17 + int(causal))
    q, k, v = (torch.randn(B, H, s, 64, generator=g).to(BF).to(cuda).requires_grad_(True) for s in (Sq, Sk, Sk))
    do = torch.randn(B, H, Sq, 64, generator=g).to(BF).to(cuda)
    if mask is not None:
        mask = mask.to(cuda)
    km, keff = (None, 1.0)
    if dropout:
        km, keff = keep_mask(seed, B, H, Sq, Sk, 1 - dropout)
        km = km.to(cuda)
    ro, rdq, rdk, rdv, rlse, dead = attention_f64(q, k, v, do, causal=causal, mask=mask, scale=scale, keep_mask=km,
                                                  keep=keff)
    tols, base = {"O": TOL_FWD, "dQ": TOL_GRAD, "dK": TOL_GRAD, "dV": TOL_GRAD}, {}
    if baseline:  # a shape where bf16 storage alone costs more than the project tolerance (module docstring)
        rounded = attention_rounded(q, k, v, do, causal=causal, mask=mask, scale=scale, keep_mask=km, keep=keff)
        for name, b, r in zip(tols, rounded, (ro, rdq, rdk, rdv)):
            base[name] = row_err(b, r).max().item()
            tols[name] = max(tols[name], 2 * base[name] + ULP)
    sc = scale if scale is not None else 0.125
    floors = {}
    if Sk == 1:
        assert rdq.abs().max() == 0 and rdk.abs().max() == 0
        floors = {"dQ": _zero_ref_floor(do, v, k, sc), "dK": _zero_ref_floor(do, v, q, sc)}
    print(f"flash attention B={B} H={H} Sq={Sq} Sk={Sk} causal={causal} mask={mask is not None} scale={scale} "
          f"dropout={dropout}: {int(dead.sum())} rows with no visible key")
    out = {}
    for ds in (False, True):
        monkeypatch.setattr(A, "_ATTN_DS", ds)
        with call_log() as log:
            o = ops.attention(q, k, v, causal=causal, mask=mask, scale=scale, dropout=dropout, training=dropout > 0,
                              seed=seed)
            lse = o.grad_fn.saved_tensors[4]
            dq, dk, dv = torch.autograd.grad(o, [q, k, v], do)
        assert log["dtf_attn_fwd"] == 1 and log["dtf_attn_bwd_ds" if ds else "dtf_attn_bwd"] == 1, dict(log)
        assert len(log) == 2, dict(log)
        tag = "ds" if ds else "recompute"
        check_rows("O", o, ro, tols["O"], _WORST, base.get("O"))
        for name, got, ref in (("dQ", dq, rdq), ("dK", dk, rdk), ("dV", dv, rdv)):
            if name in floors:
                err = got.double().abs().max().item() / floors[name]
                print(f"  {name} [{tag}]: reference is 0, |{name}| / (ulp floor) = {err:.3e}")
                assert torch.isfinite(got).all() and err <= TOL_GRAD, (name, err)
            else:
                check_rows(f"{name} [{tag}]", got, ref, tols[name], _WORST, base.get(name))
        _check_lse(lse, rlse, dead)
        dr = dead[..., 0]
        assert (o[dr] == 0).all() and (dq[dr] == 0).all(), "rows with no visible key must be exactly 0"
        out[ds] = (o, dq, dk, dv)
    return out, dead


CASES = [
    # B, H, Sq, Sk, causal
    (1, 3, 1, 1, False),
    (2, 3, 17, 17, False),
    (2, 3, 17, 17, True),
    (1, 3, 63, 65, True),
    (2, 3, 1, 200, False),
    (2, 3, 1, 200, True),
    (1, 3, 321, 321, True),
]


@pytest.mark.parametrize("B,H,Sq,Sk,causal", CASES)
def test_flash_edges(cuda, monkeypatch, B, H, Sq, Sk, causal):
    _, dead = _run(cuda, monkeypatch, B, H, Sq, Sk, causal)
    assert not dead.any()


def test_flash_causal_more_queries_than_keys(cuda, monkeypatch):
    """Sq = 130, Sk = 70: queries 0..59 see no key (the light query block of the causal pair walks no key tile at
    all); their O and dQ are 0 and lse +inf, and dK / dV hold only the other queries' contributions."""
    _, dead = _run(cuda, monkeypatch, 2, 3, 130, 70, True, baseline=True)
    assert dead[:, :, :60].all() and not dead[:, :, 60:].any()


def test_flash_causal_with_key_mask(cuda, monkeypatch):
    """Three causal query blocks with a ragged last tile and ragged key lengths on top."""
    mask = torch.zeros(2, 321)
    mask[0, 300:] = -10000.0
    mask[1, 129:] = NEG
    _, dead = _run(cuda, monkeypatch, 2, 3, 321, 321, True, mask=mask)
    assert not dead.any()


def _inf_mask(kind):
    mask = torch.zeros(2, 200)
    if kind == "tail":
        mask[0, 150:] = NEG
        mask[1, 199:] = NEG
    elif kind == "first_tile":
        mask[0, :64] = NEG
        mask[1, 190:] = NEG
    elif kind == "middle_tile":
        mask[0, 64:128] = NEG
        mask[1, :3] = NEG
    else:
        mask[1, :] = NEG
    return mask


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
@pytest.mark.parametrize("kind", ["tail", "first_tile", "middle_tile", "whole_entry"])
def test_flash_neg_inf_key_mask(cuda, monkeypatch, kind, causal):
    out, dead = _run(cuda, monkeypatch, 2, 3, 200, 200, causal, mask=_inf_mask(kind))
    dead = dead[..., 0]
    if kind == "whole_entry":
        assert dead[1].all() and not dead[0].any()
        for o, dq, dk, dv in out.values():  # the masked entry: outputs and ALL gradients exactly 0
            assert all((t[1] == 0).all() for t in (o, dq, dk, dv))
    elif causal and kind == "first_tile":
        assert dead[0, :, :64].all() and not dead[0, :, 64:].any() and not dead[1].any()
    elif causal and kind == "middle_tile":
        assert dead[1, :, :3].all() and int(dead.sum()) == 9
    else:
        assert not dead.any()


@pytest.mark.parametrize("causal", [False, True], ids=["full", "causal"])
def test_flash_dropout_ragged(cuda, monkeypatch, causal):
    """Dropout 0.3 at Sk = 70 (Sk % 4 != 0: the last quad of the counter hash is partial), against the host replica of
    the keep-mask."""
    _run(cuda, monkeypatch, 2, 3, 50, 70, causal, dropout=0.3, seed=2 ** 33 + 5)


def test_flash_explicit_scale(cuda, monkeypatch):
    _run(cuda, monkeypatch, 1, 3, 100, 164, True, scale=0.3)


def test_flash_packed_causal(cuda, monkeypatch):
    """ops.attention_packed, causal: O [B, S, H*64] and the packed dQKV against the reference."""
    B, S, H = 2, 200, 3
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(B, S, 3 * H * 64, generator=g) * 0.5).to(BF).to(cuda).requires_grad_(True)
    do = torch.randn(B, S, H * 64, generator=g).to(BF).to(cuda)
    q, k, v = A.split_qkv(qkv.detach(), H)
    ro, rdq, rdk, rdv, rlse, dead = attention_f64(q, k, v, A.split_heads(do, H), causal=True)
    ro = ro.permute(0, 2, 1, 3)                                        # [B, S, H, 64]
    rg = torch.stack([rdq, rdk, rdv]).permute(1, 3, 0, 2, 4)           # [B, S, 3, H, 64]
    print("flash attention packed causal")
    for ds in (False, True):
        monkeypatch.setattr(A, "_ATTN_DS", ds)
        with call_log() as log:
            o = ops.attention_packed(qkv, H, causal=True)
            lse = o.grad_fn.saved_tensors[2]
            (dqkv,) = torch.autograd.grad(o, [qkv], do)
        assert log["dtf_attn_fwd"] == 1 and log["dtf_attn_bwd_ds" if ds else "dtf_attn_bwd"] == 1, dict(log)
        tag = "ds" if ds else "recompute"
        check_rows("packed O", o.reshape(B, S, H, 64), ro, TOL_FWD, _WORST)
        got = dqkv.reshape(B, S, 3, H, 64)
        for j, name in enumerate(("dQ", "dK", "dV")):
            check_rows(f"packed {name} [{tag}]", got[:, :, j], rg[:, :, j], TOL_GRAD, _WORST)
        _check_lse(lse, rlse, dead)
