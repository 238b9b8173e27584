"""ops.dense_wide (the weight stream for up to 64 rows, csrc/kernels/dense_wide.hip) against float64, and the wide
one-token step of GPT-2 (generate(step="wide")) that runs on it."""
import pytest
import torch

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops._util import launch_counts, launch_delta

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
DENSE_TOL = 1e-2   # the project's bf16-epilogue tolerance
VOCAB = 200
CFG = dict(vocab=VOCAB, ctx=96, hidden=128, layers=2, heads=2)


def close(a, b, tol):
    a, b = a.float(), b.float()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item() + 1e-6
    assert err <= tol * ref, f"max err {err} vs ref scale {ref} (tol {tol})"


def bits(t):
    return t.contiguous().view(torch.int16)


def reference(x, w, bias=None, gelu=False):
    y = x.cpu().double() @ w.cpu().double().t() + (0 if bias is None else bias.cpu().double())
    return torch.nn.functional.gelu(y, approximate="tanh") if gelu else y


@pytest.mark.parametrize("epilogue", [False, True])
@pytest.mark.parametrize("N,K", [(64, 64), (200, 264), (1000, 2048), (4104, 72), (16392, 72)])
def test_dense_wide_matches_float64(cuda, N, K, epilogue):
    torch.manual_seed(N + K)
    w = (torch.randn(N, K, device=cuda) * K ** -0.5).to(BF)
    bias = torch.randn(N, device=cuda) if epilogue else None
    act = "gelu" if epilogue else None
    for M in (17, 32, 33, 48, 64):
        x = torch.randn(M, K, device=cuda).to(BF)
        before = launch_counts()
        y = ops.dense_wide(x, w, bias, act)
        d = launch_delta(before)
        assert d["dense_wide"] == 1 and sum(d.values()) == 1, d
        close(y.cpu(), reference(x, w, bias, epilogue), DENSE_TOL)
        assert torch.equal(bits(y), bits(ops.dense_wide(x, w, bias, act))), "not reproducible run to run"


@pytest.mark.parametrize("M", [64, 17])
@pytest.mark.parametrize("N,K", [(1000, 2048), (200, 264), (4104, 72), (16392, 72)])
def test_dense_wide_one_hot_rows_return_weight_columns(cuda, N, K, M):
    """x[m] = e_{k_m}, distinct k_m over the waves' K ranges, asymmetric w: out[m, n] = w[n, k_m] exactly."""
    torch.manual_seed(9)
    w = torch.randn(N, K, device=cuda).to(BF)
    km = [(m * 139 + 7) % K for m in range(M)]
    x = torch.zeros(M, K, device=cuda, dtype=BF)
    x[torch.arange(M), km] = 1.0
    assert torch.equal(bits(ops.dense_wide(x, w)), bits(w[:, km].t()))


def test_dense_wide_accepts_1_to_64_rows_only(cuda):
    def run(M, N, K):
        x, w = torch.randn(M, K, device=cuda).to(BF), torch.randn(N, K, device=cuda).to(BF)
        return ops.dense_wide(x, w).cpu(), reference(x, w)
    for M in (1, 16):
        close(*run(M, 200, 264), DENSE_TOL)
    for M, N, K in ((65, 64, 64), (20, 64, 66), (20, 10, 64)):
        with pytest.raises(RuntimeError):
            run(M, N, K)


@pytest.fixture(scope="module")
def models(cuda):
    initializers.set_seed(0)
    probe = torch.randint(0, VOCAB, (1, 4))
    with context.device(cuda), torch.no_grad():
        gpu = GPT2(**CFG)
        gpu(probe.to(cuda), training=False)   # builds the layers
    with context.device("cpu"), torch.no_grad():
        cpu = GPT2(**CFG)
        cpu(probe, training=False)
        cpu.set_weights(gpu.get_weights())
    return gpu, cpu


def test_wide_step_runs_every_projection_on_dense_wide_and_tracks_the_full_forward(cuda, models):
    """B = 20, 8 teacher-forced steps: each launches dense_wide 4 * layers + 1 times, the attention, and no GEMM tile;
    the logits' error against the f32 CPU model is within 1.5x of the full-forward GPU path's (test_generate_gpu.py)."""
    gpu, cpu = models
    torch.manual_seed(1)
    B, S0, S = 20, 5, 13
    seq = torch.randint(0, VOCAB, (B, S))
    with context.device("cpu"), torch.no_grad():
        ref = cpu(seq, training=False).float()[:, S0:, :VOCAB]
    dseq = seq.to(cuda)
    with context.device(cuda), torch.no_grad():
        full = gpu(dseq, training=False).float()[:, S0:, :VOCAB].cpu()
        cache = gpu.new_cache(B, S, cuda)
        gpu(dseq[:, :S0], training=False, cache=cache)
        cache.advance(S0)
        steps = []
        for t in range(S0, S):
            before = launch_counts()
            steps.append(gpu(dseq[:, t:t + 1].contiguous(), training=False, cache=cache, wide=True))
            d = launch_delta(before)
            assert d["dense_wide"] == 4 * CFG["layers"] + 1 and sum(d.values()) == 5 * CFG["layers"] + 1, d
            cache.advance(1)
        cached = torch.cat(steps, 1).float()[:, :, :VOCAB].cpu()
    err_full, err_wide = (full - ref).abs().max().item(), (cached - ref).abs().max().item()
    assert err_wide <= 1.5 * err_full, (err_wide, err_full)


def test_wide_generate_graph_equals_eager_and_refuses_65_rows(cuda, models):
    gpu, _ = models
    torch.manual_seed(3)
    ids = torch.randint(1, VOCAB, (20, 5), device=cuda)
    with context.device(cuda):
        a = gpu.generate(ids, 8, graph=True, step="wide")
        ga = gpu.last_generation
        b = gpu.generate(ids, 8, graph=False, step="wide")
        gb = gpu.last_generation
        assert ga["step"] is not None and ga["step"].captured and gb["step"] is None
        assert torch.equal(a, b) and torch.equal(bits(ga["logits"]), bits(gb["logits"]))
        with pytest.raises(ValueError):
            gpu.generate(torch.ones(65, 5, dtype=torch.long, device=cuda), 2, step="wide")
        c = gpu.generate(ids[:8], 8, graph=True, step="wide")   # replayed wide step against the eager default step
        lc = gpu.last_generation["logits"]
        e = gpu.generate(ids[:8], 8, graph=False)
        assert torch.equal(c, e) and torch.equal(bits(lc), bits(gpu.last_generation["logits"]))
