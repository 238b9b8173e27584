"""LARS and LAMB (layer-wise adaptive optimizers) on a CPU arena against a float64 numpy oracle of the rules.

The case layout (shared with tests/test_layerwise_optim_gpu.py): one arena of nine variables whose sizes sit around
the arena alignment (64) and the kernels' tile (T): a zero variable (||w|| = 0: ratio 1), a variable whose
gradient is all zero at step 2 (LARS: ||g|| = 0), one variable excluded from weight decay only and one from layer
adaptation only; five steps, weight decay 0.01 and a warm-up + polynomial-decay schedule so lr changes every step.
Bound: the project's optimizer bound, max error <= 1e-4 of each variable's largest reference value (weights and
slots); an f32 evaluation of either rule stays within 7e-6 of the oracle on this layout.
"""
import math

import numpy as np
import pytest
import torch

from distributed_tensorflow_amd import Variable
from distributed_tensorflow_amd.keras import optimizers
from distributed_tensorflow_amd.ops.optim import LW_TILE as T

NUMEL = [1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 5, 70001]
ZERO_VAR, ZERO_GRAD_VAR, NODECAY_VAR, NOADAPT_VAR = 2, 4, 5, 7
NAMES = [f"v{i}" + {NODECAY_VAR: "_nodecay", NOADAPT_VAR: "_noadapt"}.get(i, "") for i in range(len(NUMEL))]
STEPS, WD = 5, 0.01
SLOTS = {"lars": ["Momentum"], "lamb": ["m", "v"]}
HYPER = {"lars": dict(momentum=0.9, eeta=0.02, epsilon=0.0, nesterov=False),
         "lamb": dict(beta_1=0.9, beta_2=0.999, epsilon=1e-6)}
PEAK_LR = {"lars": 2.0, "lamb": 2e-2}


def schedule(kind):
    return optimizers.PolynomialDecay(PEAK_LR[kind], decay_steps=10, end_learning_rate=PEAK_LR[kind] / 100,
                                      warmup_steps=2)


def make_optimizer(kind, **kw):
    cls = {"lars": optimizers.LARS, "lamb": optimizers.LAMB}[kind]
    return cls(schedule(kind), weight_decay=WD, exclude_from_weight_decay=["nodecay"],
               exclude_from_layer_adaptation=["noadapt"], **HYPER[kind], **kw)


_CASE = {}


def case():
    """(initial weights, per-step gradients), float32 numpy, generated once."""
    if not _CASE:
        rng = np.random.default_rng(1234)
        w0 = [(rng.standard_normal(n) * (0.02 if i % 2 else 1.0)).astype(np.float32) for i, n in enumerate(NUMEL)]
        w0[ZERO_VAR][:] = 0
        grads = []
        for s in range(STEPS):
            g = [rng.standard_normal(n).astype(np.float32) for n in NUMEL]
            if s == 1:
                g[ZERO_GRAD_VAR][:] = 0
            grads.append(g)
        _CASE["c"] = (w0, grads)
    return _CASE["c"]


_ORACLE = {}


def oracle(kind, clipnorm=None):
    """Float64, per variable, sequential: {"w": [...], slot name: [...]} after STEPS steps."""
    key = (kind, clipnorm)
    if key in _ORACLE:
        return _ORACLE[key]
    w0, grads = case()
    h, sched = HYPER[kind], schedule(kind)
    w = [x.astype(np.float64) for x in w0]
    s1 = [np.zeros_like(x) for x in w]
    s2 = [np.zeros_like(x) for x in w]
    for t in range(1, STEPS + 1):
        lr = sched(t - 1)
        g = [x.astype(np.float64) for x in grads[t - 1]]
        if clipnorm:
            n = math.sqrt(sum(float((x * x).sum()) for x in g))
            if n > clipnorm:
                g = [x * (clipnorm / n) for x in g]
        for i in range(len(w)):
            wd = 0.0 if i == NODECAY_VAR else WD
            adapt = i != NOADAPT_VAR
            wn = math.sqrt(float((w[i] ** 2).sum()))
            if kind == "lamb":
                b1, b2, eps = h["beta_1"], h["beta_2"], h["epsilon"]
                s1[i] = b1 * s1[i] + (1 - b1) * g[i]
                s2[i] = b2 * s2[i] + (1 - b2) * g[i] * g[i]
                u = (s1[i] / (1 - b1 ** t)) / (np.sqrt(s2[i] / (1 - b2 ** t)) + eps) + wd * w[i]
                un = math.sqrt(float((u ** 2).sum()))
                r = wn / un if adapt and wn > 0 and un > 0 else 1.0
                w[i] = w[i] - lr * r * u
            else:
                gn = math.sqrt(float((g[i] ** 2).sum()))
                r = h["eeta"] * wn / (gn + wd * wn + h["epsilon"]) if adapt and wn > 0 and gn > 0 else 1.0
                gp = g[i] + wd * w[i]
                s1[i] = h["momentum"] * s1[i] + gp
                w[i] = w[i] - lr * r * (gp + h["momentum"] * s1[i] if h["nesterov"] else s1[i])
    out = {"w": w, SLOTS[kind][0]: s1}
    if kind == "lamb":
        out["v"] = s2
    _ORACLE[key] = out
    return out


def make_variables(device="cpu"):
    w0, _ = case()
    return [Variable(torch.from_numpy(x.copy()), name=nm, device=device) for x, nm in zip(w0, NAMES)]


def run_steps(opt, vs, first=0, last=STEPS):
    _, grads = case()
    for s in range(first, last):
        opt.apply_gradients([(torch.from_numpy(g).to(v.device), v) for g, v in zip(grads[s], vs)])


def state(opt, vs, kind):
    out = {"w": [v.detach().cpu().numpy().copy() for v in vs]}
    for nm in SLOTS[kind]:
        out[nm] = [opt.get_slot(v, nm).detach().cpu().numpy().copy() for v in vs]
    return out


def close(a, b, tol):
    a = torch.as_tensor(a).float()
    b = torch.as_tensor(b).float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max err {err} vs ref scale {ref} (tol {tol})"


def check_against_oracle(got, kind, clipnorm=None):
    want = oracle(kind, clipnorm)
    assert sorted(got) == sorted(want)
    for nm in want:
        for i, (a, b) in enumerate(zip(got[nm], want[nm])):
            err = np.abs(a - b).max() / (np.abs(b).max() + 1e-6)
            print(f"{kind} clip={clipnorm} {nm}[{i}] n={a.size}: rel err {err:.3g}")
    for nm in want:
        for a, b in zip(got[nm], want[nm]):
            close(a, b, 1e-4)


@pytest.mark.parametrize("kind,clipnorm", [("lars", None), ("lamb", None), ("lamb", 1.0), ("lars", 1.0)])
def test_cpu_arena_matches_oracle(kind, clipnorm):
    opt = make_optimizer(kind, global_clipnorm=clipnorm)
    vs = make_variables()
    run_steps(opt, vs)
    assert opt.host_iterations() == int(opt.iterations.item()) == STEPS
    got = state(opt, vs, kind)
    check_against_oracle(got, kind, clipnorm)
    a = vs[0]._dtf_arena  # the gradient arena is cleared and the zero padding of every variable stayed zero
    assert float(a.grad.abs().max()) == 0.0
    assert all(float(a.flat[o + v.numel():o + (v.numel() + 63) // 64 * 64].abs().sum()) == 0.0
               for v, o in zip(a.variables, a.offsets)), "zero padding moved"


def test_registry_and_slot_names():
    lamb, lars = optimizers.get("lamb"), optimizers.get("lars")
    assert type(lamb) is optimizers.LAMB and type(lars) is optimizers.LARS
    assert lamb.get_slot_names() == ["m", "v"]
    assert lars.get_slot_names() == ["Momentum"]
    assert lamb.hyper["epsilon"] == 1e-6 and lamb.hyper["weight_decay"] == 0.0 and lamb.learning_rate == 1e-3
    assert lars.hyper["momentum"] == 0.9 and lars.hyper["eeta"] == 0.001 and lars.hyper["epsilon"] == 0.0
    assert not lamb.supports_ranges() and not lars.supports_ranges()
    assert "lamb" not in optimizers._TF1_FACTORY and "lars" not in optimizers._TF1_FACTORY
    import json
    json.dumps(make_optimizer("lamb").hyper)  # the parameter server rebuilds the optimizer from {"kind", "hyper"}


def test_exclusion_defaults_follow_weight_decay_list():
    """exclude_from_layer_adaptation=None means the weight-decay list (TF-Addons)."""
    from distributed_tensorflow_amd.ops.optim import LW_ADAPT, LW_DECAY
    vs = [Variable(torch.ones(3), name="dense/kernel"), Variable(torch.ones(3), name="dense/bias")]
    o = optimizers.LAMB(exclude_from_weight_decay=["bias"])
    assert o._lw_flags(vs) == [LW_DECAY | LW_ADAPT, 0]
    o = optimizers.LAMB(exclude_from_weight_decay=["bias"], exclude_from_layer_adaptation=[])
    assert o._lw_flags(vs) == [LW_DECAY | LW_ADAPT, LW_ADAPT]


def test_bare_optimizer_rebuilt_from_kind_and_hyper_runs_the_rule():
    """How a parameter-server shard builds its optimizer: the layer-wise logic lives in the base class."""
    ref = make_optimizer("lamb")
    bare = optimizers.Optimizer.__new__(optimizers.Optimizer)
    optimizers.Optimizer.__init__(bare, schedule("lamb"), **ref.hyper)
    bare.kind = ref.kind
    va, vb = make_variables(), make_variables()
    run_steps(ref, va, last=2)
    run_steps(bare, vb, last=2)
    for x, y in zip(va, vb):
        assert torch.equal(x.detach(), y.detach())


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_checkpoint_round_trip_continues_exactly(kind, tmp_path):
    from distributed_tensorflow_amd.train import Checkpoint
    opt, vs = make_optimizer(kind), make_variables()
    run_steps(opt, vs, last=3)
    p = Checkpoint(vars=vs, optimizer=opt).write(str(tmp_path / "ck"))
    run_steps(opt, vs, first=3)
    opt2 = make_optimizer(kind)
    vs2 = [Variable(torch.zeros(n), name=nm) for n, nm in zip(NUMEL, NAMES)]
    opt2.build(vs2)
    Checkpoint(vars=vs2, optimizer=opt2).restore(p).assert_consumed()
    assert opt2.host_iterations() == 3
    run_steps(opt2, vs2, first=3)
    a, b = state(opt, vs, kind), state(opt2, vs2, kind)
    for nm in a:
        for x, y in zip(a[nm], b[nm]):
            np.testing.assert_array_equal(x, y)


def test_saver_round_trip_continues_exactly(tmp_path):
    from distributed_tensorflow_amd.train import checkpoint as C
    kind = "lamb"
    opt, vs = make_optimizer(kind), make_variables()
    run_steps(opt, vs, last=3)
    named = lambda o, vv: {**{v.name: v for v in vv}, **dict(o.variables()[1:]), "iterations": o.iterations}  # noqa: E731
    p = C.Saver(named(opt, vs)).save(None, str(tmp_path / "model.ckpt"), global_step=3)
    run_steps(opt, vs, first=3)
    opt2 = make_optimizer(kind)
    vs2 = [Variable(torch.zeros(n), name=nm) for n, nm in zip(NUMEL, NAMES)]
    opt2.build(vs2)
    C.Saver(named(opt2, vs2)).restore(None, p)
    opt2.reset_host_state()
    run_steps(opt2, vs2, first=3)
    a, b = state(opt, vs, kind), state(opt2, vs2, kind)
    for nm in a:
        for x, y in zip(a[nm], b[nm]):
            np.testing.assert_array_equal(x, y)


def test_lars_without_adaptation_and_decay_is_sgd_momentum_step_for_step():
    sched = schedule("lars")
    lars = optimizers.LARS(sched, momentum=0.9, weight_decay=0.0, exclude_from_layer_adaptation=["v"])
    sgd = optimizers.SGD(sched, momentum=0.9)
    va, vb = make_variables(), make_variables()
    for s in range(STEPS):
        run_steps(lars, va, first=s, last=s + 1)
        run_steps(sgd, vb, first=s, last=s + 1)
        for x, y in zip(va, vb):
            assert torch.equal(x.detach(), y.detach()), f"step {s + 1}: {x.name}"
            assert torch.equal(lars.get_slot(x, "Momentum"), sgd.get_slot(y, "Momentum"))


def test_tile_table_layout():
    """Tiles never cross a variable, hold at most T elements in multiples of 16 and list a variable's tiles
    consecutively; together they cover the arena exactly once."""
    opt, vs = make_optimizer("lamb"), make_variables()
    opt.build(vs)
    a = vs[0]._dtf_arena
    rows = opt._lw_plan(a).host.tolist()
    ext = list(zip(a.offsets, a.offsets[1:] + [a.numel]))
    pos, last_var = 0, 0
    for po, go, n, var in rows:
        assert po == go == pos and 0 < n <= T and n % 16 == 0 and po % 16 == 0
        assert ext[var][0] <= po and po + n <= ext[var][1] and var >= last_var
        pos, last_var = po + n, var
    assert pos == a.numel and a.offsets[-1] + 70016 == a.numel
