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
 6. (--sections 6) each launch of the fused one-token step (generate(step="fused")) alone against the calls it replaces,
    on the GPT-2-medium shapes at M = 1, 8, 16 (weights rotating through HBM as in section 3, every arm a replayed
    graph). Section 1 carries the whole step: "step captured, fused" next to "step captured", alternating inside each
    round, with the ratio fused / unfused per round.
 7. (--sections 7) past 16 rows: ops.dense_wide, and each (R, T) variant of its kernel, against ops.dense at M = 17,
    32, 48, 64 on the same shapes (as section 3), and the captured one-token step at B = 32 and 64, context ~350 and
    ~1000, default against wide=True (generate(step="wide")).
 8. (--sections 8) the fp8 KV cache (kv_dtype="fp8") against the bf16 one: KVCache.attend alone at B in {1, 8, 32, 64},
    cached length 256 and 768, H = 16, capacity 1024 (as section 2: a replayed graph over layers that rotate through
    HBM) with the K + V + scale bytes of the valid rows over its time; the captured one-token step of GPT-2-medium,
    default at B = 8 and wide at B = 32 and 64, context ~350 and ~1000; and the cache bytes at B = 64.
 9. (--sections 9) G = 16 samples per prompt: KVCache.attend on a forked cache (the prompt's K/V read once per group)
    against a plain cache of the same B0*G rows, B0 in {1, 4}, prefix 256 and 768, suffix 16 and 64 (as section 2: a
    replayed graph over layers that rotate through HBM), and generate(num_return_sequences=16) against generate on
    ids.repeat_interleave(16, 0) at 4 prompts of 768 tokens.
10. (--sections 10) past 64 rows: ops.dense_tall, and each variant of its kernel (block shape x slab budget), against
    ops.dense at M = 65, 128, 192, 256 on the same shapes (as section 7), and the captured one-token step at B = 128
    and 256, context ~350 and ~1000, default against tall=True (generate(step="tall")).
11. (--sections 11) beam search: ops.beam_select + KVCache.reorder against torch log_softmax + topk + index_select of
    24 layers' own K/V at B0 in {1, 4}, G in {4, 16} and the GPT-2 vocabulary; KVCache.attend on fork(beams=True)
    against the plain fork at the shapes of section 9; and generate(num_beams=16) against
    generate(num_return_sequences=16) at 4 prompts of 768 tokens.
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

                def step_fused(t):
                    lg = model(t, training=False, cache=cache, fused=True)
                    cache.advance(1)
                    return lg

                capf = CapturedStep(step_fused, split=False)
                for _ in range(4):
                    capf(tok)
                assert capf.captured

                def run_steps(f):
                    def go():
                        cache.lens.fill_(S0)  # stay at context S0 .. S0 + steps
                        for _ in range(steps):
                            f(tok)
                    return go

                r = rounds_of({"eager": run_steps(step), "captured": run_steps(cap), "fused": run_steps(capf),
                               "recompute": lambda: model(ids, training=False)}, rounds, 1)
                pf = rounds_of({"prefill": prefill}, rounds, 1)["prefill"]
                eager = [t / steps for t in r["eager"]]
                capt = [t / steps for t in r["captured"]]
                ratio = statistics.median(r["recompute"]) / statistics.median(capt)
                say(f"B={B} context {S0}..{S0 + steps} (capacity {cache.capacity}): prefill({S0}) {fmt(pf)}")
                say(f"    step eager    {fmt(eager)} /token")
                say(f"    step captured {fmt(capt)} /token")
                fus = [t / steps for t in r["fused"]]
                rat = [f / c for f, c in zip(fus, capt)]   # per round: the arms alternate
                say(f"    step captured, fused {fmt(fus)} /token  -> fused / unfused = {statistics.median(rat):.3f} "
                    f"({min(rat):.3f}..{max(rat):.3f}); the unfused step's rounds spread "
                    f"{min(capt) / statistics.median(capt):.3f}..{max(capt) / statistics.median(capt):.3f} of their median")
                say(f"    recompute model(ids[{B},{L}]) {fmt(r['recompute'])} /token  -> captured step is "
                    f"{ratio:.1f}x faster")
                del cap, capf, cache
        del model
    torch.cuda.empty_cache()


def section_fused_parts(dev, rounds):
    say("== 6. each fused launch alone vs the calls it replaces (GPT-2-medium shapes, H = 16, cache capacity 1024 at "
        "length 512; us per layer-call inside a replayed graph, weights rotating through HBM)")
    H, L = 16, 1024
    parts = (("LN1+QKV+store", 1024, 3072, None, True, False, True),
             ("out-proj+residual", 1024, 1024, None, False, True, False),
             ("LN2+FFN1+GELU", 1024, 4096, "gelu", True, False, False),
             ("FFN2+residual", 4096, 1024, None, False, True, False),
             ("ln_f+LM head", 1024, 50304, None, True, False, False))
    with torch.no_grad():
        for M in (1, 8, 16):
            cache = ops.KVCache(1, M, H, L, dev)
            cache.k.normal_()
            cache.v.normal_()
            cache.lens.fill_(L // 2)
            for name, K, N, act, ln, res, store in parts:
                copies = max(2, min(64, (512 << 20) // (N * K * 2)))
                ws = [torch.randn(N, K, device=dev) * 0.02 for _ in range(copies)]
                for w in ws:
                    ops._util.bf16_shadow(w)
                bias = torch.zeros(N, device=dev)
                gamma, beta = torch.ones(K, device=dev), torch.zeros(K, device=dev)
                x = torch.randn(M, 1, K, device=dev).to(torch.bfloat16)
                r0 = torch.randn(M, 1, N, device=dev).to(torch.bfloat16)

                def unfused():
                    for w in ws:
                        y = ops.dense_skinny(ops.layer_norm(x, gamma, beta, 1e-5) if ln else x, w, bias, act)
                        if store:
                            cache.store(0, y)
                        if res:
                            ops.add(r0, y)

                def fused():
                    for w in ws:
                        ops.dense_skinny_fused(x, w, bias, act, ln=(gamma, beta, 1e-5) if ln else None,
                                               residual=r0 if res else None, store=(cache, 0) if store else None)

                r = rounds_of({"unfused": graph_of(unfused), "fused": graph_of(fused)}, rounds, 10)
                un = [t / copies for t in r["unfused"]]
                fu = [t / copies for t in r["fused"]]
                say(f"M={M:2d} {name:18s} {K:5d}->{N:5d}: replaced calls {fmt(un, 1e6, 'us')}   fused "
                    f"{fmt(fu, 1e6, 'us')}   fused / unfused = {statistics.median(fu) / statistics.median(un):.2f}")
                del ws
                torch.cuda.empty_cache()
            qkv = torch.randn(M, 1, 3 * H * 64, device=dev).to(torch.bfloat16)
            cache.lens.fill_(L - 1)
            r = rounds_of({"two": graph_of(lambda: [cache.attend(0, qkv) for _ in range(16)]),
                           "one": graph_of(lambda: [cache.attend(0, qkv, fused=True) for _ in range(16)])}, rounds, 10)
            two, one = [t / 16 for t in r["two"]], [t / 16 for t in r["one"]]
            say(f"M={M:2d} attention+merge    L = {L}, one layer: two launches {fmt(two, 1e6, 'us')}   one launch "
                f"{fmt(one, 1e6, 'us')}   fused / unfused = {statistics.median(one) / statistics.median(two):.2f}")
            del cache


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


def section_wide(dev, rounds):
    say("== 7. ops.dense_wide vs ops.dense at 17 to 64 rows, GPT-2-medium projections (K -> N), weights rotating "
        "through HBM; every (R, T) variant of the kernel, `wide` is the one dtf_dense_wide launches")
    from distributed_tensorflow_amd.ops.decode import WIDE_VARIANTS, dense_wide
    not_faster = []
    with torch.no_grad():
        for K, N in ((1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024), (1024, 50304)):
            wbytes = N * K * 2
            copies = max(2, min(64, (512 << 20) // wbytes))
            ws = [torch.randn(N, K, device=dev) * 0.02 for _ in range(copies)]
            bias = torch.zeros(N, device=dev)
            for w in ws:
                ops._util.bf16_shadow(w)
            for M in (17, 32, 48, 64):
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)

                def arm(variant):
                    return graph_of(lambda: [dense_wide(x, w, bias, variant=variant) for w in ws])

                arms = {"dense": graph_of(lambda: [ops.dense(x, w, bias) for w in ws]), "wide": arm(None)}
                arms.update({f"R{r}T{t}": arm(v) for v, (r, t) in enumerate(WIDE_VARIANTS)})
                res = {k: [t / copies for t in ts] for k, ts in rounds_of(arms, rounds, 10).items()}
                de, wi = res["dense"], res["wide"]
                bw = wbytes / statistics.median(wi)
                # faster only by more than the baseline's own spread: the slowest wide round under the fastest dense one
                verdict = "" if max(wi) < min(de) else "   <-- NOT FASTER than ops.dense beyond the spread"
                if verdict:
                    not_faster.append((K, N, M))
                say(f"{K:5d}->{N:5d} M={M:2d} ({copies:2d} copies): wide {fmt(wi, 1e6, 'us')} "
                    f"[{bw / 1e12:.2f} TB/s, {100 * bw / COPY_BW:.0f}% of copy bw]   dense {fmt(de, 1e6, 'us')}   "
                    f"x{statistics.median(de) / statistics.median(wi):.2f}{verdict}")
                say("        " + "   ".join(f"({r:2d},{t}) {fmt(res[f'R{r}T{t}'], 1e6, 'us')}" for r, t in WIDE_VARIANTS))
                del arms
            del ws
            torch.cuda.empty_cache()
    say("shapes where dense_wide is not faster than ops.dense (these belong in ops.decode.WIDE_EXCLUDE): "
        + (", ".join(f"{k}->{n} at M={m}" for k, n, m in not_faster) if not_faster else "none"))
    say("per token: the captured one-token step of GPT-2-medium, default (projections on ops.dense past 16 rows) "
        "against wide=True, alternating inside each round")
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        for B in (32, 64):
            for L in (384, 1024):
                S0, steps = L - 32, 24
                torch.manual_seed(B * 10000 + L)
                tok = torch.randint(0, model.vocab, (B, 1), device=dev)
                cache = model.new_cache(B, L, dev)
                cache.k.normal_()
                cache.v.normal_()
                cache.empty = False  # "filled": only lens says how far
                cache.lens.fill_(S0)

                def stepper(wide):
                    def step(t):
                        lg = model(t, training=False, cache=cache, wide=wide)
                        cache.advance(1)
                        return lg
                    cap = CapturedStep(step, split=False)
                    for _ in range(4):
                        cap(tok)
                    assert cap.captured

                    def go():
                        cache.lens.fill_(S0)  # stay at context S0 .. S0 + steps
                        for _ in range(steps):
                            cap(tok)
                    return go

                r = rounds_of({"default": stepper(False), "wide": stepper(True)}, rounds, 1)
                de = [t / steps for t in r["default"]]
                wi = [t / steps for t in r["wide"]]
                rat = [a / b for a, b in zip(wi, de)]
                say(f"B={B} context {S0}..{S0 + steps}: step captured {fmt(de)} /token   wide {fmt(wi)} /token  -> "
                    f"wide / default = {statistics.median(rat):.3f} ({min(rat):.3f}..{max(rat):.3f}); the default "
                    f"step's rounds spread {min(de) / statistics.median(de):.3f}..{max(de) / statistics.median(de):.3f} "
                    "of their median")
                del cache
        del model
    torch.cuda.empty_cache()


def _fill(cache, n):
    """Arbitrary finite contents (fp8: codes below the NaN code, scale 2^-6) and lens = n."""
    if cache.fp8:
        for codes, sc in ((cache.k, cache.k_scale), (cache.v, cache.v_scale)):
            codes.random_(0, 0x78)
            sc.fill_(2.0 ** -6)
    else:
        cache.k.normal_()
        cache.v.normal_()
    cache.empty = False
    cache.lens.fill_(n)


def section_kv_fp8(dev, rounds):
    say("== 8. fp8 KV cache (e4m3 codes + one f32 power-of-two scale a row, 68 B) against bf16 (128 B)")
    H, cap = 16, 1024
    say(f"KVCache.attend alone, H = {H}, capacity {cap}, inside a replayed graph over layers rotating through HBM; "
        "bytes: K + V (+ scales) of the valid rows")
    with torch.no_grad():
        for B in (1, 8, 32, 64):
            layers = max(2, min(16, -(-(537 << 20) // (2 * B * H * cap * 128))))
            caches = {d: ops.KVCache(layers, B, H, cap, dev, kv_dtype=d) for d in ("bf16", "fp8")}
            qkv = torch.randn(B, 1, 3 * H * 64, device=dev).to(torch.bfloat16)
            for L in (256, 768):
                arms = {}
                for d, cache in caches.items():
                    _fill(cache, L - 1)
                    arms[d] = graph_of(lambda cache=cache: [cache.attend(l, qkv) for l in range(layers)])
                res = rounds_of(arms, rounds, 20)
                line = f"B={B:2d} L={L}: "
                for d, row in (("bf16", 128), ("fp8", 68)):
                    ts = [t / layers for t in res[d]]
                    nbytes = 2 * B * H * L * row
                    bw = nbytes / statistics.median(ts)
                    line += (f"{d} {fmt(ts, 1e6, 'us')} {nbytes / 1e6:6.2f} MB {bw / 1e12:.2f} TB/s "
                             f"{100 * bw / COPY_BW:3.0f}%   ")
                say(line + f"fp8 / bf16 = {statistics.median(res['fp8']) / statistics.median(res['bf16']):.2f}")
            del caches, arms
            torch.cuda.empty_cache()
    say("per token: the captured one-token step of GPT-2-medium, bf16 against fp8 cache, alternating inside each round")
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        for B, wide in ((8, False), (32, True), (64, True)):
            for L in (384, 1024):
                S0, steps = L - 32, 24
                torch.manual_seed(B * 10000 + L)
                tok = torch.randint(0, model.vocab, (B, 1), device=dev)

                def stepper(cache):
                    def step(t):
                        lg = model(t, training=False, cache=cache, wide=wide)
                        cache.advance(1)
                        return lg
                    cap_ = CapturedStep(step, split=False)
                    for _ in range(4):
                        cap_(tok)
                    assert cap_.captured

                    def go():
                        cache.lens.fill_(S0)  # stay at context S0 .. S0 + steps
                        for _ in range(steps):
                            cap_(tok)
                    return go

                caches = {d: model.new_cache(B, L, dev, kv_dtype=d) for d in ("bf16", "fp8")}
                for cache in caches.values():
                    _fill(cache, S0)
                r = rounds_of({d: stepper(c) for d, c in caches.items()}, rounds, 1)
                bf, f8 = ([t / steps for t in r[d]] for d in ("bf16", "fp8"))
                rat = [a / b for a, b in zip(f8, bf)]
                say(f"B={B} {'wide' if wide else 'default'} step, context {S0}..{S0 + steps}: bf16 {fmt(bf)} /token   "
                    f"fp8 {fmt(f8)} /token  -> fp8 / bf16 = {statistics.median(rat):.3f} ({min(rat):.3f}..{max(rat):.3f})")
                del caches
        c = model.cfg
        rows = 2 * c["layers"] * 64 * c["heads"] * 1024
        say(f"cache bytes, GPT-2-medium, B = 64, capacity 1024: bf16 {rows * 128 / 1e9:.2f} GB, fp8 {rows * 68 / 1e9:.2f} GB "
            "(codes + scales)")
        del model
    torch.cuda.empty_cache()


def section_shared_prefix(dev, rounds):
    say("== 9. shared-prefix decode attention (KVCache.fork, generate(num_return_sequences=G)) against repeated prompts")
    H, cap, G = 16, 1024, 16
    say(f"KVCache.attend alone, G = {G}, H = {H}, capacity {cap}, inside a replayed graph over layers rotating through "
        "HBM: a fork (prefix read once per group) against a plain cache of the same B0*G rows")
    with torch.no_grad():
        for B0 in (1, 4):
            B = B0 * G
            layers = max(2, min(16, -(-(537 << 20) // (2 * B * H * cap * 128))))
            parent, plain = ops.KVCache(layers, B0, H, cap, dev), ops.KVCache(layers, B, H, cap, dev)
            qkv = torch.randn(B, 1, 3 * H * 64, device=dev).to(torch.bfloat16)
            for Lp in (256, 768):
                _fill(parent, Lp)
                fork = parent.fork(G)
                fork.k.normal_()
                fork.v.normal_()
                for Ls in (16, 64):
                    _fill(plain, Lp + Ls - 1)
                    fork.lens.fill_(Lp + Ls - 1)
                    arms = {"plain": graph_of(lambda: [plain.attend(l, qkv) for l in range(layers)]),
                            "fork": graph_of(lambda: [fork.attend(l, qkv) for l in range(layers)])}
                    res = rounds_of(arms, rounds, 20)
                    pl, fk = ([t / layers for t in res[k]] for k in ("plain", "fork"))
                    rat = [a / b for a, b in zip(fk, pl)]
                    mb = [2 * H * n * 128 / 1e6 for n in (B * (Lp + Ls), B0 * Lp + B * Ls)]
                    say(f"B0={B0} x G={G} prefix {Lp} suffix {Ls}: plain {fmt(pl, 1e6, 'us')} {mb[0]:6.2f} MB   "
                        f"fork {fmt(fk, 1e6, 'us')} {mb[1]:6.2f} MB  -> fork / plain = {statistics.median(rat):.2f} "
                        f"({min(rat):.2f}..{max(rat):.2f})")
                    del arms
                del fork
            del parent, plain
            torch.cuda.empty_cache()
    say("generate end to end, GPT-2-medium, 4 prompts of 768 tokens x 16 samples, 64 new tokens, sampler=\"fused\", "
        "step=\"wide\", graph=True (prefill and capture included)")
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        torch.manual_seed(9)
        ids = torch.randint(0, model.vocab, (4, 768), device=dev)
        rep = ids.repeat_interleave(G, 0)
        kw = dict(temperature=0.8, top_k=40, seed=1, sampler="fused", step="wide")
        res = rounds_of({"repeated": lambda: model.generate(rep, 64, **kw),
                         "shared": lambda: model.generate(ids, 64, num_return_sequences=G, **kw)}, rounds, 1)
        rat = [a / b for a, b in zip(res["shared"], res["repeated"])]
        say(f"repeated ids {fmt(res['repeated'])}   num_return_sequences={G} {fmt(res['shared'])}  -> shared / repeated "
            f"= {statistics.median(rat):.3f} ({min(rat):.3f}..{max(rat):.3f})")
        del model
    torch.cuda.empty_cache()


def section_beam(dev, rounds):
    say("== 11. beam search (generate(num_beams=G)): ops.beam_select + KVCache.reorder, the slot-indirect attention, "
        "and the captured step")
    H, cap, n, ld, own = 16, 1024, 50257, 50304, 64
    say(f"token choice alone, vocabulary {n} (ld {ld}, bf16 logits ~ N(0, 4^2)), inside a replayed graph: beam_select + "
        f"reorder (slot table [B, {cap}] and history [B, {cap}]) against torch log_softmax + topk + index_select of 24 "
        f"layers' own K/V ({own} positions, H = {H})")
    with torch.no_grad():
        for B0 in (1, 4):
            for G in (4, 16):
                B = B0 * G
                base = ops.KVCache(1, B0, 1, cap, dev)
                base.empty = False
                base.lens.fill_(768)
                fork = base.fork(G, beams=True)
                fork.lens.fill_(768 + own)
                logits = (4 * torch.randn(B, ld, device=dev)).to(torch.bfloat16)
                scores = -torch.rand(B, device=dev)
                done = torch.zeros(B, dtype=torch.bool, device=dev)
                hist = torch.zeros(B, cap, dtype=torch.int64, device=dev)
                kv = torch.randn(2, 24, B, H, own, 64, device=dev).to(torch.bfloat16)
                rows0 = (torch.arange(B, device=dev) // G * G)

                def kernels():
                    parent, tok = ops.beam_select(logits, n=n, scores=scores.clone(), done=done, group=G, pad=0)
                    fork.reorder(parent, history=hist, token=tok)

                def torch_route():
                    val = scores[:, None] + torch.log_softmax(logits.float()[:, :n], -1)
                    top = val.view(B0, G * n).topk(G, -1).indices.view(-1)
                    rows = rows0 + top // n
                    return kv.index_select(2, rows), hist.index_select(0, rows), top % n

                res = rounds_of({"kernels": graph_of(kernels), "torch": graph_of(torch_route)}, rounds, 50)
                rat = [a / b for a, b in zip(res["kernels"], res["torch"])]
                say(f"B0={B0} x G={G}: beam_select + reorder {fmt(res['kernels'], 1e6, 'us')}   torch "
                    f"{fmt(res['torch'], 1e6, 'us')}  -> kernels / torch = {statistics.median(rat):.3f} "
                    f"({min(rat):.3f}..{max(rat):.3f})")
                del kv
        G = 16
        say(f"KVCache.attend alone, G = {G}, H = {H}, capacity {cap}, as section 9: fork(beams=True) with a random slot "
            "table against the plain fork")
        for B0 in (1, 4):
            B = B0 * G
            layers = max(2, min(16, -(-(537 << 20) // (2 * B * H * cap * 128))))
            parent = ops.KVCache(layers, B0, H, cap, dev)
            qkv = torch.randn(B, 1, 3 * H * 64, device=dev).to(torch.bfloat16)
            for Lp in (256, 768):
                _fill(parent, Lp)
                plain, beam = parent.fork(G), parent.fork(G, beams=True)
                plain.k.normal_()
                plain.v.normal_()
                beam.k, beam.v = plain.k, plain.v
                beam.slots = torch.randint(0, G, (B, cap), device=dev).to(torch.uint8)
                for Ls in (16, 64):
                    plain.lens.fill_(Lp + Ls - 1)
                    beam.lens.fill_(Lp + Ls - 1)
                    arms = {"plain": graph_of(lambda: [plain.attend(l, qkv) for l in range(layers)]),
                            "beam": graph_of(lambda: [beam.attend(l, qkv) for l in range(layers)])}
                    res = rounds_of(arms, rounds, 20)
                    pl, bm = ([t / layers for t in res[k]] for k in ("plain", "beam"))
                    rat = [a / b for a, b in zip(bm, pl)]
                    say(f"B0={B0} x G={G} prefix {Lp} suffix {Ls}: plain fork {fmt(pl, 1e6, 'us')}   beams "
                        f"{fmt(bm, 1e6, 'us')}  -> beams / plain = {statistics.median(rat):.2f} "
                        f"({min(rat):.2f}..{max(rat):.2f})")
                    del arms
                del plain, beam
            del parent
            torch.cuda.empty_cache()
    say("generate end to end, GPT-2-medium, 4 prompts of 768 tokens x 16 rows, 64 new tokens, step=\"wide\", graph=True "
        "(prefill and capture included): num_beams=16 against num_return_sequences=16 with sampler=\"fused\"")
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        torch.manual_seed(9)
        ids = torch.randint(0, model.vocab, (4, 768), device=dev)
        res = rounds_of({"samples": lambda: model.generate(ids, 64, num_return_sequences=G, temperature=0.8, top_k=40,
                                                            seed=1, sampler="fused", step="wide"),
                         "beams": lambda: model.generate(ids, 64, num_beams=G, step="wide")}, rounds, 1)
        rat = [a / b for a, b in zip(res["beams"], res["samples"])]
        say(f"num_return_sequences={G} {fmt(res['samples'])}   num_beams={G} {fmt(res['beams'])}  -> beams / samples "
            f"= {statistics.median(rat):.3f} ({min(rat):.3f}..{max(rat):.3f})")
        del model
    torch.cuda.empty_cache()


def section_tall(dev, rounds):
    say("== 10. ops.dense_tall vs ops.dense at 65 to 256 rows, GPT-2-medium projections (K -> N), weights rotating "
        "through HBM; every variant (weight rows x x rows, slab budget b) of the kernel, `tall` is the one "
        "dtf_dense_tall launches")
    from distributed_tensorflow_amd.ops.decode import TALL_VARIANTS, dense_tall
    not_faster = []
    with torch.no_grad():
        for K, N in ((1024, 3072), (1024, 1024), (1024, 4096), (4096, 1024), (1024, 50304)):
            wbytes = N * K * 2
            copies = max(2, min(64, (512 << 20) // wbytes))
            ws = [torch.randn(N, K, device=dev) * 0.02 for _ in range(copies)]
            bias = torch.zeros(N, device=dev)
            for w in ws:
                ops._util.bf16_shadow(w)
            for M in (65, 128, 192, 256):
                x = torch.randn(M, K, device=dev).to(torch.bfloat16)

                def arm(variant):
                    return graph_of(lambda: [dense_tall(x, w, bias, variant=variant) for w in ws])

                arms = {"dense": graph_of(lambda: [ops.dense(x, w, bias) for w in ws]), "tall": arm(None)}
                arms.update({f"v{v}": arm(v) for v in range(len(TALL_VARIANTS))})
                res = {k: [t / copies for t in ts] for k, ts in rounds_of(arms, rounds, 10).items()}
                de, ta = res["dense"], res["tall"]
                bw = wbytes / statistics.median(ta)
                # faster only by more than the baseline's own spread: the slowest tall round under the fastest dense one
                verdict = "" if max(ta) < min(de) else "   <-- NOT FASTER than ops.dense beyond the spread"
                if verdict:
                    not_faster.append((K, N, M))
                say(f"{K:5d}->{N:5d} M={M:3d} ({copies:2d} copies): tall {fmt(ta, 1e6, 'us')} "
                    f"[{bw / 1e12:.2f} TB/s, {100 * bw / COPY_BW:.0f}% of copy bw]   dense {fmt(de, 1e6, 'us')}   "
                    f"x{statistics.median(de) / statistics.median(ta):.2f}{verdict}")
                for lo in range(0, len(TALL_VARIANTS), 3):
                    say("        " + "   ".join(f"({bn}x{bm:3d},b{b}) {fmt(res[f'v{v}'], 1e6, 'us')}"
                                                for v, (bn, bm, b) in list(enumerate(TALL_VARIANTS))[lo:lo + 3]))
                del arms
            del ws
            torch.cuda.empty_cache()
    say("shapes where dense_tall is not faster than ops.dense (these belong in ops.decode.TALL_EXCLUDE): "
        + (", ".join(f"{k}->{n} at M={m}" for k, n, m in not_faster) if not_faster else "none"))
    say("per token: the captured one-token step of GPT-2-medium, default (projections on ops.dense past 16 rows) "
        "against tall=True, alternating inside each round")
    with context.device(dev), torch.no_grad():
        model = gpt2_medium(dropout=0.0)
        for B in (128, 256):
            for L in (384, 1024):
                S0, steps = L - 32, 24
                torch.manual_seed(B * 10000 + L)
                tok = torch.randint(0, model.vocab, (B, 1), device=dev)
                cache = model.new_cache(B, L, dev)
                _fill(cache, S0)

                def stepper(tall):
                    def step(t):
                        lg = model(t, training=False, cache=cache, tall=tall)
                        cache.advance(1)
                        return lg
                    cap = CapturedStep(step, split=False)
                    for _ in range(4):
                        cap(tok)
                    assert cap.captured

                    def go():
                        cache.lens.fill_(S0)  # stay at context S0 .. S0 + steps
                        for _ in range(steps):
                            cap(tok)
                    return go

                r = rounds_of({"default": stepper(False), "tall": stepper(True)}, rounds, 1)
                de = [t / steps for t in r["default"]]
                ta = [t / steps for t in r["tall"]]
                rat = [a / b for a, b in zip(ta, de)]
                say(f"B={B} context {S0}..{S0 + steps}: step captured {fmt(de)} /token   tall {fmt(ta)} /token  -> "
                    f"tall / default = {statistics.median(rat):.3f} ({min(rat):.3f}..{max(rat):.3f}); the default "
                    f"step's rounds spread {min(de) / statistics.median(de):.3f}..{max(de) / statistics.median(de):.3f} "
                    "of their median")
                del cache
        del model
    torch.cuda.empty_cache()


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
    if "6" in sec:
        section_fused_parts(dev, a.rounds)
    if "7" in sec:
        section_wide(dev, a.rounds)
    if "8" in sec:
        section_kv_fp8(dev, a.rounds)
    if "9" in sec:
        section_shared_prefix(dev, a.rounds)
    if "10" in sec:
        section_tall(dev, a.rounds)
    if "11" in sec:
        section_beam(dev, a.rounds)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
