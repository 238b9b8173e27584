"""LAMB with sharded optimizer state (ZeRO-1) on CPU: 2 and 3 gloo processes with tiny buckets, so shard boundaries
cut variables and the per-variable sums of squares must be reduced over the replicas before the trust ratios are
formed. All ranks must hold identical weights and gathered slots, equal to single-process training."""
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest
import torch


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _train_mlp(strategy, x, y, epochs=2, batch=64, seed=0):
    from distributed_tensorflow_amd.keras import initializers, losses, optimizers
    from distributed_tensorflow_amd.models.mlp import MnistMLP
    initializers.set_seed(seed)
    with strategy.scope():
        m = MnistMLP(hidden=32)
        m.compile(optimizers.LAMB(1e-2, weight_decay=0.01), losses.SparseCategoricalCrossentropy(from_logits=True),
                  metrics=["accuracy"])
    h = m.fit(x, y, batch_size=batch, epochs=epochs, shuffle=False, verbose=0)
    return m, h


def _state(m):
    return [w.detach().numpy().copy() for w in m.weights] + \
        [m.optimizer.get_slot(v, nm).detach().numpy().copy() for nm in ("m", "v") for v in m.trainable_variables]


def _worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port), DTF_CPU_ALLREDUCE="gloo", HIP_VISIBLE_DEVICES="",
                      CUDA_VISIBLE_DEVICES="", DTF_ALLREDUCE_DTYPE="f32", DTF_ZERO="1", DTF_BUCKET_MB="0.0001",
                      DTF_OVERLAP_UPDATE="0")
    try:
        from distributed_tensorflow_amd import parallel
        from distributed_tensorflow_amd.models.mlp import synthetic_mnist
        from distributed_tensorflow_amd.parallel.collective import ShardedGradientBucketer
        n, batch = (576, 96) if world == 3 else (512, 64)
        x, y = synthetic_mnist(n)
        s = parallel.MultiWorkerMirroredStrategy()
        m, h = _train_mlp(s, torch.as_tensor(x), torch.as_tensor(y), seed=rank, batch=batch)
        bs = [b for b in s._bucketers.values() if isinstance(b, ShardedGradientBucketer)]
        assert bs and len(bs[0].buckets) > 1, "expected sharded state over several buckets"
        # at least one owned range must cut a variable, or the cross-replica reduction of the norms is not exercised
        a = bs[0].arena
        bounds = set(a.offsets) | {a.numel}
        assert any(lo not in bounds or hi not in bounds for lo, hi, _ in bs[0].segments()) or world == 1
        s.sync_optimizer_state(m.optimizer)
        q.put((rank, _state(m), h.history["loss"]))
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    except Exception:
        import traceback
        q.put((rank, None, traceback.format_exc()))


@pytest.mark.parametrize("world", [2, 3])
def test_zero1_lamb_matches_single_process(world):
    from distributed_tensorflow_amd import parallel
    from distributed_tensorflow_amd.models.mlp import synthetic_mnist
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    [p.start() for p in ps]
    res = sorted([q.get(timeout=240) for _ in range(world)], key=lambda t: t[0])
    [p.join(60) for p in ps]
    for r in res:
        assert r[1] is not None, r[2]
    for other in res[1:]:
        for a, b in zip(res[0][1], other[1]):
            np.testing.assert_allclose(a, b, rtol=0, atol=0)
    n, batch = (576, 96) if world == 3 else (512, 64)
    x, y = synthetic_mnist(n)
    m, h = _train_mlp(parallel.OneDeviceStrategy("cpu"), torch.as_tensor(x), torch.as_tensor(y), batch=batch)
    for a, w in zip(res[0][1], _state(m)):
        print("max abs diff", float(np.abs(a - w).max()), "ref max", float(np.abs(w).max()))
    for a, w in zip(res[0][1], _state(m)):
        np.testing.assert_allclose(a, w, rtol=1e-4, atol=1e-5)
    assert res[0][2][-1] < res[0][2][0]
