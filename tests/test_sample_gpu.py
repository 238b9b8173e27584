"""The fused token sampler on the GPU (csrc/kernels/sample.hip) against its host replica (ops.sample_reference): exact
equality of tokens and bookkeeping for every elements-per-thread instance, both dtypes, every filter setting and both
kinds of draw; the index order of the final scan; the launch counter; and GPT2.generate(sampler="fused") replayed from
a hipGraph against eager steps, with no aten sampling op left in the loop."""
import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from distributed_tensorflow_amd import context, ops
from distributed_tensorflow_amd.keras import initializers
from distributed_tensorflow_amd.models.transformer import GPT2
from distributed_tensorflow_amd.ops import _util

pytestmark = pytest.mark.gpu
TOP = (1 << 32) - 1
WIDTH = 12

SHAPES = [(2, 200, 256), (5, 1000, 1000), (3, 8191, 8192), (3, 50257, 50304), (1, 65536, 65536)]
SETTINGS = [
    dict(temperature=1.0),
    dict(temperature=0.7, top_k=40),
    dict(temperature=0.9, top_p=0.9),
    dict(temperature=1.3, top_k=50, top_p=0.8, repetition_penalty=1.2),
    dict(temperature=1.0, top_k=1),
    dict(temperature=1.0, top_k=1 << 20),
    dict(temperature=1.0, top_p=1.0),
    dict(temperature=1.0, top_p=1e-4),
    dict(temperature=0.0, repetition_penalty=1.5),   # greedy, with a planted tie at the maximum
]


def _logits(B, n, ld, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, ld, generator=g) * 4.0
    x[:, n:] = 1e4                                   # the padding of a row must never be read as a logit
    x[0, 1] = float("-inf")
    x[B - 1, n // 2] = float("nan")
    top = x[:, :n].nan_to_num(nan=-1e9).max(-1).values + 1.0
    for b in range(B):                               # two entries share the maximum (lowest index wins greedy)
        x[b, n - 1] = top[b]
        x[b, n // 3] = top[b]
    return x.to(dtype)


def _state(B, n, seed):
    g = torch.Generator().manual_seed(seed + 99)
    out = torch.randint(0, n, (B, WIDTH), generator=g)
    out[:, 0] = n - 1                                # the maximum is in every history that is not empty
    out[0, 1], out[0, 2] = -3, n + 5                 # ids outside [0, n) are ignored
    pos = torch.tensor([(3 + 4 * b) % (WIDTH + 1) for b in range(B)])
    if B > 1:
        pos[B - 1] = WIDTH                           # at the end of out: nothing is written
    done = torch.zeros(B, dtype=torch.bool)
    return out, pos, done


def _both(x, n, cuda, state, **kw):
    """(tok, out, pos, done) of the replica and of the kernel from equal starting states."""
    got = []
    for dev in ("cpu", cuda):
        out, pos, done = (t.clone().to(dev) for t in state)
        u = kw.get("uniform")
        k = dict(kw, uniform=None if u is None else u.to(dev))
        tok = ops.sample_logits(x.to(dev), n=n, out=out, pos=pos, done=done, **k)
        got.append(tuple(t.cpu() for t in (tok, out, pos, done)))
    return got


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_equals_replica(cuda, shape, dtype):
    B, n, ld = shape
    x = _logits(B, n, ld, dtype, seed=n)
    state = _state(B, n, seed=n)
    g = torch.Generator().manual_seed(7)
    injected = torch.randint(0, 1 << 32, (B,), generator=g)
    injected[0] = TOP
    for i, kw in enumerate(SETTINGS):
        for uniform in (injected, None):
            want, got = _both(x, n, cuda, state, seed=1000 + i, uniform=uniform, **kw)
            for name, w, h in zip(("tok", "out", "pos", "done"), want, got):
                assert torch.equal(w, h), (f"{name} differs for {kw}, {'injected' if uniform is not None else 'hash'} "
                                           f"draw: replica {w.tolist()}, kernel {h.tolist()}")
    # the planted tie: greedy takes the lower of the two indices unless the penalty (history holds n - 1) decides
    out, pos, done = (t.clone().to(cuda) for t in _state(B, n, seed=n))
    pos.zero_()
    tok = ops.sample_logits(x.to(cuda), n=n, temperature=0.0, out=out, pos=pos, done=done)
    assert tok.tolist() == [n // 3] * B


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "f32"])
def test_draws_at_the_edges_of_the_kept_set(cuda, dtype):
    """48 rows of flat logits (many survivors, bf16 ties) with the draw at 0, at 2^32 - 1 and at random: the first and
    the last kept index of a row show a threshold that is off by one element."""
    B, n, ld = 48, 1000, 1000
    g = torch.Generator().manual_seed(11)
    x = torch.randn(B, ld, generator=g).to(dtype)
    U = torch.randint(0, 1 << 32, (B,), generator=g)
    U[0::3], U[1::3] = 0, TOP
    out = torch.randint(0, n, (B, WIDTH), generator=g)
    state = (out, torch.full((B,), WIDTH // 2), torch.zeros(B, dtype=torch.bool))
    for kw in (dict(top_k=7), dict(top_k=200, top_p=0.5), dict(top_p=0.3), dict(top_p=0.97, repetition_penalty=1.3),
               dict(top_k=999), dict(top_p=0.999)):
        want, got = _both(x, n, cuda, state, temperature=1.1, uniform=U, **kw)
        assert torch.equal(want[0], got[0]), f"{kw}: rows {(want[0] != got[0]).nonzero().flatten().tolist()} differ"
        assert torch.equal(want[1], got[1])


def test_bookkeeping_equals_replica(cuda):
    """Rows that are done, rows that emit eos now, and a row whose pos is at the end of out, over two calls."""
    B, n, ld = 6, 1000, 1000
    x = _logits(B, n, ld, torch.bfloat16, seed=3)
    out, pos, done = _state(B, n, seed=3)
    done[1] = True
    kw = dict(temperature=0.8, top_k=30, top_p=0.95, repetition_penalty=1.1, seed=21, pad=7)
    free = ops.sample_reference(x, n=n, out=out.clone(), pos=pos.clone(), done=done.clone(), **kw)
    eos = int(free[2])                                   # row 2 emits eos in this very call
    cpu = [t.clone() for t in (out, pos, done)]
    gpu = [t.clone().to(cuda) for t in (out, pos, done)]
    xg = x.to(cuda)
    for call in range(2):
        want = ops.sample_logits(x, n=n, out=cpu[0], pos=cpu[1], done=cpu[2], eos=eos, **kw)
        got = ops.sample_logits(xg, n=n, out=gpu[0], pos=gpu[1], done=gpu[2], eos=eos, **kw)
        assert torch.equal(want, got.cpu()), f"call {call}"
        for w, h in zip(cpu, gpu):
            assert torch.equal(w, h.cpu()), f"call {call}"
        assert int(want[1]) == 7 and bool(cpu[2][2])
    assert int(want[2]) == 7                             # after its eos the row emits pad
    assert cpu[1][B - 1] == WIDTH + 2 and torch.equal(cpu[0][B - 1], out[B - 1])


@pytest.mark.parametrize("m", [1, 7, 1025])
def test_scan_walks_the_index_order(cuda, m):
    """m positions hold one finite logit, the rest -inf: the masses are equal, so the token is the
    floor(U * m / 2^32)-th finite index."""
    n, ld, B = 50257, 50304, 8
    g = torch.Generator().manual_seed(m)
    U = torch.randint(0, 1 << 32, (B,), generator=g)
    U[0], U[1] = 0, TOP
    x = torch.full((B, ld), float("-inf"))
    want = []
    for b in range(B):
        where = torch.randperm(n, generator=g)[:m].sort().values
        x[b, where] = 1.5
        want.append(int(where[(int(U[b]) * m) >> 32]))
    for dtype in (torch.bfloat16, torch.float32):
        out = torch.zeros(B, 1, dtype=torch.int64, device=cuda)
        pos = torch.zeros(B, dtype=torch.int64, device=cuda)
        done = torch.zeros(B, dtype=torch.bool, device=cuda)
        tok = ops.sample_logits(x.to(dtype).to(cuda), n=n, temperature=1.0, out=out, pos=pos, done=done,
                                uniform=U.to(cuda))
        assert tok.tolist() == want
        assert out[:, 0].tolist() == want and pos.tolist() == [1] * B


def test_one_sample_launch_per_call(cuda):
    x = torch.randn(3, 256, device=cuda).bfloat16()
    out = torch.zeros(3, 4, dtype=torch.int64, device=cuda)
    pos = torch.zeros(3, dtype=torch.int64, device=cuda)
    done = torch.zeros(3, dtype=torch.bool, device=cuda)
    ops.sample_logits(x, n=200, temperature=1.0, out=out, pos=pos, done=done)   # the table upload is not counted
    before = _util.launch_counts()
    with _util.call_log() as log:
        ops.sample_logits(x, n=200, temperature=0.9, top_k=5, top_p=0.9, repetition_penalty=1.1, out=out, pos=pos,
                          done=done)
    delta = _util.launch_delta(before)
    assert delta["sample"] == 1 and sum(delta.values()) == 1
    assert dict(log) == {"dtf_sample_logits": 1}
    assert pos.tolist() == [2, 2, 2]


def test_argument_checks_on_the_gpu(cuda):
    out = torch.zeros(2, 4, dtype=torch.int64, device=cuda)
    pos = torch.zeros(2, dtype=torch.int64, device=cuda)
    done = torch.zeros(2, dtype=torch.bool, device=cuda)
    ok = dict(out=out, pos=pos, done=done)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 65544, device=cuda), n=65537, **ok)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 12, device=cuda), n=8, **ok)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 8, device=cuda), n=9, **ok)
    with pytest.raises(ValueError):
        ops.sample_logits(torch.zeros(2, 16, device=cuda), n=8, out=out.cpu(), pos=pos, done=done)
    assert pos.tolist() == [0, 0]


# ---------------------------------------------------------------- GPT2.generate(sampler="fused")
VOCAB, CTX = 200, 96
CFG = dict(vocab=VOCAB, ctx=CTX, hidden=128, layers=2, heads=2)
BANNED = ("topk", "sort", "multinomial", "softmax", "argmax", "scatter_")


class _NoAtenSampling(TorchDispatchMode):
    """Records every banned aten op that runs with a CUDA operand."""

    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        name = func.overloadpacket.__name__
        if name.lstrip("_") in BANNED or name in BANNED:
            flat = list(args) + list((kwargs or {}).values())
            if any(isinstance(a, torch.Tensor) and a.is_cuda for a in flat):
                self.seen.append(name)
        return func(*args, **(kwargs or {}))


@pytest.fixture(scope="module")
def tiny(cuda):
    initializers.set_seed(0)
    torch.manual_seed(0)
    with context.device(cuda), torch.no_grad():
        model = GPT2(**CFG)
        model(torch.randint(0, VOCAB, (1, 4), device=cuda), training=False)
    return model


@pytest.mark.parametrize("B", [1, 3])
def test_fused_graph_replay_equals_eager_steps(cuda, tiny, B):
    torch.manual_seed(2 + B)
    new, pad = 12, 0
    ids = torch.randint(1, VOCAB, (B, 5), device=cuda)
    plens = [5, 3, 4][:B]
    for b in range(B):
        ids[b, plens[b]:] = pad
    kw = dict(prompt_lens=torch.tensor(plens), pad_token_id=pad, temperature=0.9, top_k=50, top_p=0.9,
              repetition_penalty=1.2, seed=17)
    with context.device(cuda):
        guard = _NoAtenSampling()
        with guard:
            a = tiny.generate(ids, new, graph=True, **kw)
        ga = tiny.last_generation
        b_ = tiny.generate(ids, new, graph=False, **kw)
        gb = tiny.last_generation
        c = tiny.generate(ids, new, graph=True, **dict(kw, seed=18))
    assert guard.seen == [], f"aten sampling ops on the fused route: {guard.seen}"
    assert ga["step"] is not None and ga["step"].captured, "the sampler + model step was not captured"
    assert gb["step"] is None
    assert torch.equal(a, b_)
    assert not torch.equal(a, c), "another seed gave the same tokens"
    assert torch.equal(ga["logits"].view(torch.int16), gb["logits"].view(torch.int16))
    want = [p + new for p in plens]
    assert ga["cache"].lens.tolist() == want and gb["cache"].lens.tolist() == want
    assert a.dtype == torch.int64 and tuple(a.shape) == (B, 5 + new)
    assert int(a.max()) < VOCAB and int(a.min()) >= 0
    for b in range(B):
        assert torch.equal(a[b, :plens[b]], ids[b, :plens[b]]), "prompt not preserved"
        assert (a[b, plens[b] + new:] == pad).all(), "tail is not padding"


def test_fused_rows_together_equal_rows_alone_and_eos_pads(cuda, tiny):
    torch.manual_seed(9)
    ids = torch.randint(0, VOCAB, (2, 5), device=cuda)
    kw = dict(temperature=0.9, top_p=0.9, repetition_penalty=1.2, seed=4, sampler="fused")
    with context.device(cuda):
        both = tiny.generate(ids, 8, graph=False, **kw)
        for b in range(2):   # the draw is keyed by the row index: row b alone is a batch of two copies of it
            alone = tiny.generate(ids[b:b + 1].expand(2, 5).contiguous(), 8, graph=False, **kw)
            assert torch.equal(alone[b], both[b]), f"row {b}"
        greedy = tiny.generate(ids, 8, graph=False)
        assert torch.equal(tiny.generate(ids, 8, graph=False, sampler="fused"), greedy)
        eos = int(both[0, 6])
        first = int((both[0, 5:] == eos).nonzero()[0]) + 5
        e = tiny.generate(ids, 8, graph=True, eos_token_id=eos, pad_token_id=199, **kw)
    assert torch.equal(e[0, :first + 1], both[0, :first + 1]) and (e[0, first + 1:] == 199).all()
