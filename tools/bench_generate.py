"""KV-cached generation on random-init GPT-2-medium: what a decode step costs, against the recompute forward.

  python tools/bench_generate.py [--out profiles/generate_decode.txt] [--rounds 5]

Sections (every arm is warmed up, the arms of a comparison alternate inside each round, and the median with the
min..max spread over the rounds is reported; times are host clocks around work that ends in a device synchronise):
 1. B in {1, 8}, context ~384 and ~1024: prefill, ms/token of the one-token step eager and hipGraph-captured, and the
    recompute baseline (one full model(ids) at the same context: the only way to get the next token without a cache).
 2. dtf_attn_decode alone at B*H = 128, L = 1024: bytes of K and V it must read over its time, as a share of the
    6.29 TB/s copy bandwidth. The cache rotates over 16 layers (537 MB) so the reads come from HBM, not from a cache.
 3. ops.dense_skinny against ops.dense on the five GPT-2-medium projection shapes at M = 1, 8, 16, rotating over
    enough weight copies (>= 512 MB where they fit) that each call streams its weights from HBM as a decode step does.
 4. (--sections 4) token choice: generate(graph=True, temperature=0.8, top_k=40) at B in {1, 8} with the torch route
    (aten topk / softmax / multinomial between two replays) against sampler="fused" (ops.sample_logits captured with the
    step), ms/token from the difference of a long and a short call of the same arm; and ops.sample_logits alone at
    n = 50257.
 5. (--sections 5) continuing a filled cache: N in {16, 64, 256} new tokens behind L in {1, 256, 768} cached ones at
    B in {1, 8}: token by token (extend(chunk=1), and the captured one-token step replayed N times) against one chunked
    extend on a chunked=True cache; and dtf_attn_append alone with the K/V bytes it must read over its time.
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_amd import context, ops  # noqa: E402
from distributed_tensorflow_amd.graphs import CapturedStep  # noqa: E402
from distributed_tensorflow_amd.models.transformer import gpt2_medium  # noqa: E402

COPY_BW = 6.29e12  # measured copy bandwidth of the MI355X, bytes/s
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, iters):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters


def rounds_of(arms, rounds, iters):
    """arms: {name: fn}. Warm each, then `rounds` rounds in which the arms alternate. -> {name: [seconds per call]}"""
    for fn in arms.values():
        timed(fn, 2)
    res = {k: [] for k in arms}
    for _ in range(rounds):
        for k, fn in arms.items():
            res[k].append(timed(fn, iters))
    return res


def fmt(ts, unit=1e3, u="ms"):
    return f"{statistics.median(ts) * unit:8.3f} {u} ({min(ts) * unit:.3f}..{max(ts) * unit:.3f})"


def graph_of(fn):
    """fn captured into one hipGraph (after a warm-up on a side stream); returns the replay callable."""
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g.replay


def section_generate(dev, rounds):
    say("== 1. GPT-2-medium (random init, bf16), KV-cached step vs recompute forward")
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        for B in (1, 8):
            for L in (384, 1024):
                S0, steps = L - 64, 48
                torch.manual_seed(B * 10000 + L)
                ids = torch.randint(0, model.vocab, (B, L), device=dev)
                tok = ids[:, :1].contiguous()
                cache = model.new_cache(B, L, dev)

                def prefill():
                    cache.reset()
                    model(ids[:, :S0], training=False, cache=cache)
                    cache.lens.fill_(S0)

                def step(t):
                    lg = model(t, training=False, cache=cache)
                    cache.advance(1)
                    return lg

                prefill()
                cap = CapturedStep(step, split=False)
                for _ in range(4):
                    cap(tok)
                assert cap.captured

                def run_steps(f):
                    def go():
                        cache.lens.fill_(S0)  # stay at context S0 .. S0 + steps
                        for _ in range(steps):
                            f(tok)
                    return go

                r = rounds_of({"eager": run_steps(step), "captured": run_steps(cap),
                               "recompute": lambda: model(ids, training=False)}, rounds, 1)
                pf = rounds_of({"prefill": prefill}, rounds, 1)["prefill"]
                eager = [t / steps for t in r["eager"]]
                capt = [t / steps for t in r["captured"]]
                ratio = statistics.median(r["recompute"]) / statistics.median(capt)
                say(f"B={B} context {S0}..{S0 + steps} (capacity {cache.capacity}): prefill({S0}) {fmt(pf)}")
                say(f"    step eager    {fmt(eager)} /token")
                say(f"    step captured {fmt(capt)} /token")
                say(f"    recompute model(ids[{B},{L}]) {fmt(r['recompute'])} /token  -> captured step is "
                    f"{ratio:.1f}x faster")
                del cap, cache
        del model
    torch.cuda.empty_cache()


def section_attention(dev, rounds):
    say("== 2. dtf_attn_decode alone, B*H = 128 (B=8, H=16), L = 1024")
    B, H, L, layers = 8, 16, 1024, 16
    with torch.no_grad():
        cache = ops.KVCache(layers, B, H, L, dev)
        cache.k.normal_()
        cache.v.normal_()
        cache.lens.fill_(L - 1)
        qkv = torch.randn(B, 1, 3 * H * 64, device=dev).to(torch.bfloat16)

        def sweep():
            for l in range(layers):
                cache.attend(l, qkv)

        rep = graph_of(sweep)
        ts = [t / layers for t in rounds_of({"attn": rep}, rounds, 20)["attn"]]
    nbytes = 2 * B * H * L * 64 * 2
    bw = nbytes / statistics.median(ts)
    say(f"per call (partials + merge launch, inside a replayed graph of {layers} calls over {layers} layers): "
        f"{fmt(ts, 1e6, 'us')}; K+V bytes {nbytes / 1e6:.1f} MB -> {bw / 1e12:.2f} TB/s = "
        f"{100 * bw / COPY_BW:.0f}% of the 6.29 TB/s copy bandwidth")


def section_dense(dev, rounds):
    say("== 3. ops.dense_skinny vs ops.dense, GPT-2-medium projections (K -> N), weights rotating through HBM")
    slower = []
    with torch.no_grad():
        for K, N in ((1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024), (1024, 50304)):
            wbytes = N * K * 2
            copies = max(2, min(64, (512 << 20) // wbytes))
            ws = [torch.randn(N, K, device=dev) * 0.02 for _ in range(copies)]
            bias = torch.zeros(N, device=dev)
            for w in ws:
                ops._util.bf16_shadow(w)
            for M in (1, 8, 16):
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)

                def skinny():
                    for w in ws:
                        ops.dense_skinny(x, w, bias)

                def dense():
                    for w in ws:
                        ops.dense(x, w, bias)

                r = rounds_of({"skinny": graph_of(skinny), "dense": graph_of(dense)}, rounds, 10)
                sk = [t / copies for t in r["skinny"]]
                de = [t / copies for t in r["dense"]]
                bw = wbytes / statistics.median(sk)
                verdict = "" if statistics.median(sk) <= statistics.median(de) else "   <-- SLOWER than ops.dense"
                if verdict:
                    slower.append((K, N, M))
                say(f"{K:5d}->{N:5d} M={M:2d} ({copies:2d} copies): skinny {fmt(sk, 1e6, 'us')} "
                    f"[{bw / 1e12:.2f} TB/s, {100 * bw / COPY_BW:.0f}% of copy bw]   dense {fmt(de, 1e6, 'us')}   "
                    f"x{statistics.median(de) / statistics.median(sk):.2f}{verdict}")
            del ws
            torch.cuda.empty_cache()
    say("shapes where dense_skinny is slower (these keep ops.dense in the decode step, ops.decode.SKINNY_EXCLUDE): "
        + (", ".join(f"{k}->{n} at M={m}" for k, n, m in slower) if slower else "none"))


def section_sampler(dev, rounds):
    say("== 4. token choice in generate(graph=True, temperature=0.8, top_k=40), GPT-2-medium: torch route vs "
        "sampler=\"fused\"")
    short, long_ = 16, 112
    ratios = {}
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        for B in (1, 8):
            torch.manual_seed(B)
            ids = torch.randint(0, model.vocab, (B, 64), device=dev)

            def per_token(sampler):
                def go():
                    ts = []
                    for n in (short, long_):
                        torch.cuda.synchronize()
                        t = time.perf_counter()
                        model.generate(ids, n, temperature=0.8, top_k=40, seed=1, graph=True, sampler=sampler)
                        torch.cuda.synchronize()
                        ts.append(time.perf_counter() - t)
                    return (ts[1] - ts[0]) / (long_ - short)
                return go

            arms = {"torch": per_token("torch"), "fused": per_token("fused")}
            for fn in arms.values():
                fn()
            res = {k: [] for k in arms}
            for _ in range(rounds):
                for k, fn in arms.items():
                    res[k].append(fn())
            ratios[B] = statistics.median(res["fused"]) / statistics.median(res["torch"])
            say(f"B={B} prompt 64, tokens {short}..{long_} of a call (prefill and capture cancel in the difference):")
            say(f"    torch route  {fmt(res['torch'])} /token")
            say(f"    fused route  {fmt(res['fused'])} /token  -> fused / torch = {ratios[B]:.3f}")
        del model
    torch.cuda.empty_cache()
    say("ops.sample_logits alone, n = 50257 (ld 50304, bf16 logits ~ N(0, 4^2)), 16 calls inside one replayed graph:")
    with torch.no_grad():
        for B in (1, 8):
            x = (torch.randn(B, 50304, device=dev) * 4).to(torch.bfloat16)
            out = torch.randint(0, 50257, (B, 256), device=dev)
            done = torch.zeros(B, dtype=torch.bool, device=dev)
            for name, kw in (("T=0.8 k=40", dict(temperature=0.8, top_k=40)),
                             ("T=0.9 p=0.9", dict(temperature=0.9, top_p=0.9)),
                             ("T=1.3 k=50 p=0.8 r=1.2", dict(temperature=1.3, top_k=50, top_p=0.8,
                                                            repetition_penalty=1.2)),
                             ("greedy", dict(temperature=0.0))):
                pos = torch.full((B,), 128, dtype=torch.int64, device=dev)

                def sweep():
                    for _ in range(16):
                        ops.sample_logits(x, n=50257, seed=3, out=out, pos=pos, done=done, **kw)

                ts = [t / 16 for t in rounds_of({"s": graph_of(sweep)}, rounds, 10)["s"]]
                say(f"    B={B} {name:24s} {fmt(ts, 1e6, 'us')} per call")
    return ratios


def section_append(dev, rounds):
    say("== 5. N new tokens behind a cache holding L (GPT-2-medium, capacity 1024): token by token vs one chunked call")
    say("token by token: extend(chunk=1) on a default cache (eager, the route without the append kernel) and the "
        "captured one-token step replayed N times; chunked: extend() of all N on a chunked=True cache, eager")
    ratios = {}
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        for B in (1, 8):
            caches = {}
            for chunked in (False, True):
                c = model.new_cache(B, 1024, dev, chunked=chunked)
                c.k.normal_()
                c.v.normal_()
                c.empty = False  # "filled": only lens says how far
                caches[chunked] = c
            tok = torch.randint(0, model.vocab, (B, 1), device=dev)

            def step(t):
                lg = model(t, training=False, cache=caches[False])
                caches[False].advance(1)
                return lg

            caches[False].lens.fill_(1)
            cap = CapturedStep(step, split=False)
            for _ in range(4):
                cap(tok)
            assert cap.captured
            for L in (1, 256, 768):
                for N in (16, 64, 256):
                    if L + N > 1024:
                        continue
                    torch.manual_seed(B * 100000 + L * 1000 + N)
                    ids = torch.randint(0, model.vocab, (B, N), device=dev)

                    def one_by_one():
                        caches[False].lens.fill_(L)
                        model.extend(ids, caches[False], chunk=1)

                    def replayed():
                        caches[False].lens.fill_(L)
                        for _ in range(N):
                            cap(tok)

                    def chunk_call():
                        caches[True].lens.fill_(L)
                        model.extend(ids, caches[True])

                    r = rounds_of({"one": one_by_one, "replay": replayed, "chunk": chunk_call}, rounds, 1)
                    med = {k: statistics.median(v) for k, v in r.items()}
                    ratios[(B, L, N)] = (med["one"] / med["chunk"], med["replay"] / med["chunk"])
                    say(f"B={B} L={L:3d} N={N:3d}: extend(chunk=1) {fmt(r['one'])}   captured step x N "
                        f"{fmt(r['replay'])}   one chunked call {fmt(r['chunk'])}   -> x{ratios[(B, L, N)][0]:.1f} / "
                        f"x{ratios[(B, L, N)][1]:.1f}")
            del cap, caches
        layers, H = model.cfg["layers"], model.cfg["heads"]
        del model
    torch.cuda.empty_cache()
    say(f"dtf_attn_append alone (H = {H}, capacity 1024, rotating over {layers} layers inside one replayed graph): K+V "
        "bytes it must read (each once) over its time; MFMA work 4 * 64 * visible (query, key) pairs")
    with torch.no_grad():
        for B in (1, 8):
            cache = ops.KVCache(layers, B, H, 1024, dev, chunked=True)
            cache.k.normal_()
            cache.v.normal_()
            for L in (1, 256, 768):
                for N in (16, 64, 256):
                    if L + N > 1024:
                        continue
                    cache.lens.fill_(L)
                    qkv = torch.randn(B, N, 3 * H * 64, device=dev).to(torch.bfloat16)

                    def sweep():
                        for l in range(layers):
                            cache.attend_chunk(l, qkv)

                    ts = [t / layers for t in rounds_of({"a": graph_of(sweep)}, rounds, 20)["a"]]
                    t = statistics.median(ts)
                    nbytes = 2 * B * H * (L + N) * 64 * 2
                    flops = 4 * 64 * B * H * (N * L + N * (N + 1) // 2)
                    say(f"    B={B} L={L:3d} N={N:3d} ({-(-N // 64) * B * H:4d} blocks): {fmt(ts, 1e6, 'us')}; K+V "
                        f"{nbytes / 1e6:6.2f} MB -> {nbytes / t / 1e12:.3f} TB/s ({100 * nbytes / t / COPY_BW:.0f}% of "
                        f"copy bw), {flops / t / 1e12:.2f} TFLOP/s")
            del cache
    torch.cuda.empty_cache()
    return ratios


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  "profiles", "generate_decode.txt"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sections", default="1,2,3")
    ap.add_argument("--append", action="store_true", help="append to --out instead of replacing it")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_generate needs a GPU: nothing here can be measured on a CPU")
    dev = torch.device("cuda", 0)
    say(f"tools/bench_generate.py on {torch.cuda.get_device_name(0)}; rounds {a.rounds}; median (min..max)")
    sec = set(a.sections.split(","))
    if "2" in sec:
        section_attention(dev, a.rounds)
    if "3" in sec:
        section_dense(dev, a.rounds)
    if "1" in sec:
        section_generate(dev, a.rounds)
    if "4" in sec:
        section_sampler(dev, a.rounds)
    if "5" in sec:
        section_append(dev, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
