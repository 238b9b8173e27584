"""ops.dense_tall (the weight stream for up to 256 rows, csrc/kernels/dense_tall.hip) against float64, and the tall
one-token step of GPT-2 (generate(step="tall")) that runs on it."""
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
SHAPES = [(64, 64), (200, 264), (1000, 2048), (4104, 72)]


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
@pytest.mark.parametrize("N,K", SHAPES)
def test_dense_tall_matches_float64(cuda, N, K, epilogue):
    torch.manual_seed(N + K)
    w = (torch.randn(N, K, device=cuda) * K ** -0.5).to(BF)
    bias = torch.randn(N, device=cuda) if epilogue else None
    act = "gelu" if epilogue else None
    for M in (65, 80, 128, 129, 255, 256):
        x = torch.randn(M, K, device=cuda).to(BF)
        before = launch_counts()
        y = ops.dense_tall(x, w, bias, act)
        d = launch_delta(before)
        assert d["dense_tall"] == 1 and sum(d.values()) == 1, d
        close(y.cpu(), reference(x, w, bias, epilogue), DENSE_TOL)
        assert torch.equal(bits(y), bits(ops.dense_tall(x, w, bias, act))), "not reproducible run to run"


@pytest.mark.parametrize("variant", range(len(ops.decode.TALL_VARIANTS)))
def test_dense_tall_every_variant_matches_float64(cuda, variant):
    """Every block shape and split budget the benchmark times, where K splits for real and N, K fit no tile."""
    torch.manual_seed(variant)
    for M, N, K in ((129, 200, 2056), (256, 1000, 2048)):
        x, w = torch.randn(M, K, device=cuda).to(BF), (torch.randn(N, K, device=cuda) * K ** -0.5).to(BF)
        bias = torch.randn(N, device=cuda)
        close(ops.dense_tall(x, w, bias, "gelu", variant=variant).cpu(), reference(x, w, bias, True), DENSE_TOL)


@pytest.mark.parametrize("M", [256, 65])
@pytest.mark.parametrize("N,K", SHAPES[1:])
def test_dense_tall_one_hot_rows_return_weight_columns(cuda, N, K, M):
    """x[m] = e_{k_m}, k_m spread over the K-tiles and splits, asymmetric w: out[m, n] = w[n, k_m] exactly."""
    torch.manual_seed(9)
    w = torch.randn(N, K, device=cuda).to(BF)
    km = [(m * 139 + 7) % K for m in range(M)]
    x = torch.zeros(M, K, device=cuda, dtype=BF)
    x[torch.arange(M), km] = 1.0
    assert torch.equal(bits(ops.dense_tall(x, w)), bits(w[:, km].t()))


def test_dense_tall_accepts_1_to_256_rows_only(cuda):
    def run(M, N, K):
        x, w = torch.randn(M, K, device=cuda).to(BF), torch.randn(N, K, device=cuda).to(BF)
        return ops.dense_tall(x, w).cpu(), reference(x, w)
    for M in (1, 16, 64):
        close(*run(M, 200, 264), DENSE_TOL)
    for M, N, K in ((257, 64, 64), (80, 64, 66), (80, 10, 64)):
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


def test_tall_step_runs_every_projection_on_dense_tall_and_tracks_the_full_forward(cuda, models):
    """B = 80, 4 teacher-forced steps: each launches dense_tall 4 * layers + 1 times (the tiny LM head is not in
    TALL_EXCLUDE), the attention, and no GEMM tile; the logits' error against the f32 CPU model is within 1.5x of the
    full-forward GPU path's (the wide step's criterion)."""
    gpu, cpu = models
    torch.manual_seed(1)
    B, S0, S = 80, 5, 9
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
            steps.append(gpu(dseq[:, t:t + 1].contiguous(), training=False, cache=cache, tall=True))
            d = launch_delta(before)
            assert d["dense_tall"] == 4 * CFG["layers"] + 1 and sum(d.values()) == 5 * CFG["layers"] + 1, d
            cache.advance(1)
        cached = torch.cat(steps, 1).float()[:, :, :VOCAB].cpu()
    err_full, err_tall = (full - ref).abs().max().item(), (cached - ref).abs().max().item()
    print(f"max |logits - f32 reference|: full forward {err_full:.5f}, tall step {err_tall:.5f}")
    assert err_tall <= 1.5 * err_full, (err_tall, err_full)


def test_tall_generate_graph_equals_eager_and_matches_the_other_steps_below_65_rows(cuda, models):
    gpu, _ = models
    torch.manual_seed(3)
    ids = torch.randint(1, VOCAB, (80, 5), device=cuda)

    def run(rows, **kw):
        out = gpu.generate(ids[:rows], 6, **kw)
        return out, bits(gpu.last_generation["logits"]), gpu.last_generation["step"]

    with context.device(cuda):
        a, la, sa = run(80, graph=True, step="tall")
        b, lb, sb = run(80, graph=False, step="tall")
        assert sa is not None and sa.captured and sb is None
        assert torch.equal(a, b) and torch.equal(la, lb)
        for rows, other in ((8, None), (20, "wide")):
            c, lc, _ = run(rows, graph=True, step="tall")
            e, le, _ = run(rows, graph=False, step=other)
            assert torch.equal(c, e) and torch.equal(lc, le), rows
        with pytest.raises(ValueError):
            gpu.generate(torch.ones(257, 5, dtype=torch.long, device=cuda), 2, step="tall")


def test_tall_generate_samples_run_on_dense_tall(cuda, models):
    gpu, _ = models
    torch.manual_seed(4)
    ids = torch.randint(1, VOCAB, (10, 5), device=cuda)
    with context.device(cuda):
        before = launch_counts()
        out = gpu.generate(ids, 4, num_return_sequences=8, temperature=0.8, top_k=40, seed=1, step="tall")
        assert tuple(out.shape) == (80, 9) and launch_delta(before)["dense_tall"] > 0
