"""LARS and LAMB on the GPU (csrc/kernels/optim_layerwise.hip: tile-table pass 1 / per-variable finalize / pass 2)
against the float64 oracle and the case layout of tests/test_layerwise_optim.py, plus determinism, the bf16 copy,
table validation, a hipGraph-captured Keras step and ZeRO-1 on RCCL."""
import multiprocessing as mp
import os
import socket
import traceback

import numpy as np
import pytest
import torch

import test_layerwise_optim as L

pytestmark = pytest.mark.gpu

_RUNS = {}


def _run(kind, clipnorm=None, fresh=False):
    """State after the five steps of the shared case on the GPU (+ bf16 copy, f32 master, gradient arena)."""
    key = (kind, clipnorm)
    if fresh or key not in _RUNS:
        dev = torch.device("cuda:0")
        opt = L.make_optimizer(kind, global_clipnorm=clipnorm)
        vs = L.make_variables(dev)
        L.run_steps(opt, vs)
        torch.cuda.synchronize()
        out = L.state(opt, vs, kind)
        a = vs[0]._dtf_arena
        out["_arena"] = (a.flat.cpu(), a.bf16.cpu(), a.grad.cpu())
        assert opt.host_iterations() == int(opt.iterations.item()) == L.STEPS
        if fresh:
            return out
        _RUNS[key] = out
    return _RUNS[key]


@pytest.mark.parametrize("kind,clipnorm", [("lars", None), ("lamb", None), ("lamb", 1.0)])
def test_gpu_arena_matches_oracle(cuda, kind, clipnorm):
    got = {k: v for k, v in _run(kind, clipnorm).items() if not k.startswith("_")}
    L.check_against_oracle(got, kind, clipnorm)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_two_fresh_runs_are_bitwise_equal(cuda, kind):
    a, b = _run(kind), _run(kind, fresh=True)
    for nm in ["w"] + L.SLOTS[kind]:
        for x, y in zip(a[nm], b[nm]):
            np.testing.assert_array_equal(x, y)
    assert torch.equal(a["_arena"][0], b["_arena"][0])


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_bf16_copy_and_zeroed_gradient(cuda, kind):
    flat, bf16, grad = _run(kind)["_arena"]
    assert torch.equal(bf16, flat.to(torch.bfloat16))
    assert float(grad.abs().max()) == 0.0
    assert float(flat.abs().max()) > 0.0


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_tile_past_the_arena_end_is_refused_before_any_launch(cuda, kind):
    from distributed_tensorflow_amd.ops import optim as O
    opt = L.make_optimizer(kind)
    vs = L.make_variables(cuda)
    opt.build(vs)
    a = vs[0]._dtf_arena
    a.grad.normal_()
    good = opt._lw_plan(a)
    hp = torch.tensor([1e-2, 1.0, 0.0, 0.0, 10.0, 1000.0, 0.0, 0.0], device=cuda)
    s = [a.slots[nm] for nm in L.SLOTS[kind]]
    s1, s2 = s[0], (s[1] if len(s) > 1 else None)
    bufs = [a.flat, a.grad, a.bf16, good.partials, good.scale] + s
    torch.cuda.synchronize()
    before = [b.clone() for b in bufs]
    for bad_row in ("end", "var", "align", "order"):
        rows = good.host.tolist()
        po, go, n, var = rows[-1]
        assert po + n == a.numel and n + 64 <= O.LW_TILE
        if bad_row == "end":
            rows[-1] = [po, go, n + 64, var]       # crosses the arena end
        elif bad_row == "var":
            rows[-1] = [po, go, n, len(vs)]        # variable index out of range
        elif bad_row == "align":
            rows[-1] = [po + 2, go + 2, n - 4, var]  # not a multiple of 4
        else:
            rows[-1] = [po, go, n, 0]              # variable indices decrease: tiles no longer consecutive
        plan = O.LayerwisePlan(rows, good.flags_host, a.numel, a.numel, cuda)
        plan.partials, plan.scale = good.partials, good.scale
        with pytest.raises(RuntimeError, match="dtf_lw_pass1 failed with status -1"):
            O.layerwise_pass1(kind, plan, a.flat, a.grad, s1, s2, hp)
        with pytest.raises(RuntimeError, match="dtf_lw_finalize failed with status -1"):
            O.layerwise_finalize(kind, plan)
        with pytest.raises(RuntimeError, match="dtf_lw_pass2 failed with status -1"):
            O.layerwise_pass2(kind, plan, a.flat, a.grad, s1, a.bf16, hp)
    torch.cuda.synchronize()
    for b, c in zip(bufs, before):
        assert torch.equal(b, c), "a refused call changed a buffer"


def test_captured_lamb_step_matches_eager(cuda):
    from distributed_tensorflow_amd.graphs import CapturedStep
    from distributed_tensorflow_amd.keras import Sequential, initializers, layers, losses, optimizers
    torch.manual_seed(0)
    xs = [torch.randn(64, 128, device=cuda) for _ in range(6)]
    ys = [torch.randint(0, 16, (64,), device=cuda) for _ in range(6)]
    outs = []
    for jit in (False, True):
        initializers.set_seed(3)
        model = Sequential([layers.Dense(256, activation="relu"), layers.Dense(16)])
        sched = optimizers.PolynomialDecay(2e-2, decay_steps=10, end_learning_rate=2e-4, warmup_steps=2)
        model.compile(optimizer=optimizers.LAMB(sched, weight_decay=0.01, exclude_from_weight_decay=["bias"]),
                      loss=losses.SparseCategoricalCrossentropy(from_logits=True), jit_compile=jit)
        fn = model.make_train_function(force=True)
        assert isinstance(fn, CapturedStep) == jit
        losses_seen = [float(fn((x, y))["loss"]) for x, y in zip(xs, ys)]
        torch.cuda.synchronize()
        if jit:
            assert fn.captured, "the LAMB step was not captured"
        o = model.optimizer
        outs.append((losses_seen, [w.detach().float().cpu().clone() for w in model.weights] +
                     [o.get_slot(v, nm).detach().float().cpu().clone() for nm in ("m", "v")
                      for v in model.trainable_variables], o.host_iterations(), int(o.iterations.item())))
    (l0, w0, h0, i0), (l1, w1, h1, i1) = outs
    assert h0 == h1 == i0 == i1 == 6
    assert l0[-1] < l0[0]
    for a, b in zip(w0, w1):
        L.close(b, a, 1e-4)


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gpt2(seed):
    from distributed_tensorflow_amd.keras import initializers, losses, optimizers
    from distributed_tensorflow_amd.models.transformer import GPT2
    initializers.set_seed(seed)
    m = GPT2(vocab=320, ctx=128, hidden=128, layers=2, heads=2, dropout=0.0)
    m.compile(optimizer=optimizers.LAMB(1e-3, weight_decay=0.01),
              loss=losses.SparseCategoricalCrossentropy(from_logits=True))
    return m


def _batches(dev, steps=5):
    g = torch.Generator().manual_seed(5)
    out = []
    for _ in range(steps):
        ids = torch.randint(0, 320, (8, 128), generator=g)
        out.append((ids.to(dev), torch.roll(ids, -1, 1).to(dev)))
    return out


def _worker_rccl1(port, q):
    os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                      DTF_FORCE_COLLECTIVE="1")
    os.environ.pop("DTF_COLLECTIVE_BACKEND", None)
    try:
        import torch.distributed as dist
        from distributed_tensorflow_amd import parallel
        from distributed_tensorflow_amd.parallel.collective import ShardedGradientBucketer
        s = parallel.MultiWorkerMirroredStrategy(bucket_mb=0.25, shard_optimizer=True)
        assert dist.get_backend() == "nccl"
        with s.scope():
            m = _gpt2(100)
        losses = [float(m.train_step((x, y))["loss"]) for x, y in _batches(s.device)]
        torch.cuda.synchronize()
        b = s._bucketers[id(m._arena)]
        assert isinstance(b, ShardedGradientBucketer)
        q.put(([w.detach().float().cpu().numpy() for w in m.trainable_variables], losses, len(b.buckets)))
        dist.destroy_process_group()
    except Exception:
        q.put((None, traceback.format_exc(), 0))


def test_zero1_lamb_on_rccl_world1_matches_single_process(cuda):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_worker_rccl1, args=(_port(), q))
    p.start()
    try:
        ws, losses, nb = q.get(timeout=100)
    finally:
        p.join(30)
        if p.is_alive():
            p.kill()
    assert ws is not None, losses
    assert nb > 3
    m = _gpt2(100)
    ref = [float(m.train_step((x, y))["loss"]) for x, y in _batches(cuda)]
    torch.cuda.synchronize()
    tol = dict(rtol=2e-3, atol=2e-4)
    for a, b in zip(losses, ref):
        assert abs(a - b) <= tol["rtol"] * abs(b) + 1e-4, (losses, ref)
    for a, w in zip(ws, m.trainable_variables):
        torch.testing.assert_close(torch.from_numpy(a), w.detach().float().cpu(), **tol)
