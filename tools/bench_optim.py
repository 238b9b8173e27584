#!/usr/bin/env python
"""Cost of the layer-wise optimizers against the fused elementwise update they extend, on one parameter arena of
GPT-2-medium size (one variable per real tensor shape, about 355 M elements), in one process:

    AdamW (one dtf_optim_apply launch, 34 B/element)   vs  LAMB (pass 1 28 B + pass 2 18 B = 46 B/element)
    SGD with momentum (one launch, 26 B/element)       vs  LARS (pass 1  8 B + pass 2 26 B = 34 B/element)

Bytes per element count every f32 stream read and written once, the bf16 copy and the gradient zeroing. Each
update is timed with device events around Optimizer.apply_arena; baseline and layer-wise rule alternate inside one
loop; medians over --iters timed iterations after --warmup. The three launches of the layer-wise step are also
timed one by one (ops.optim.layerwise_*), so a slow pass can be named.

    python tools/bench_optim.py [--iters 30] [--warmup 5] [--out profiles/layerwise_optim.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distributed_tensorflow_amd import Variable  # noqa: E402
from distributed_tensorflow_amd.keras import optimizers  # noqa: E402
from distributed_tensorflow_amd.ops import optim as O  # noqa: E402

BYTES = {"adamw": 34, "lamb": 46, "sgdm": 26, "lars": 34}
PASS_BYTES = {"lamb": (28, 18), "lars": (8, 26)}


def gpt2_medium_shapes(layers=24, hidden=1024, vocab=50257, ctx=1024):
    s = [("wte", (vocab, hidden)), ("wpe", (ctx, hidden))]
    for i in range(layers):
        p = f"h{i}/"
        s += [(p + "ln_1/gamma", (hidden,)), (p + "ln_1/beta", (hidden,)),
              (p + "attn/c_attn/kernel", (hidden, 3 * hidden)), (p + "attn/c_attn/bias", (3 * hidden,)),
              (p + "attn/c_proj/kernel", (hidden, hidden)), (p + "attn/c_proj/bias", (hidden,)),
              (p + "ln_2/gamma", (hidden,)), (p + "ln_2/beta", (hidden,)),
              (p + "mlp/c_fc/kernel", (hidden, 4 * hidden)), (p + "mlp/c_fc/bias", (4 * hidden,)),
              (p + "mlp/c_proj/kernel", (4 * hidden, hidden)), (p + "mlp/c_proj/bias", (hidden,))]
    return s + [("ln_f/gamma", (hidden,)), ("ln_f/beta", (hidden,))]


def make(opt, shapes, dev):
    vs = [Variable(torch.empty(shape, device=dev).normal_(0, 0.02), name=nm) for nm, shape in shapes]
    opt.build(vs)
    return opt, vs[0]._dtf_arena


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_optim.py needs a GPU")
    dev = torch.device("cuda:0")
    shapes = gpt2_medium_shapes(args.layers)
    ex = ["bias", "gamma", "beta"]
    lines = []
    ratios = {}
    for base_name, new_name, mk_base, mk_new in [
            ("adamw", "lamb", lambda: optimizers.AdamW(1e-3, weight_decay=0.01),
             lambda: optimizers.LAMB(1e-3, weight_decay=0.01, exclude_from_weight_decay=ex)),
            ("sgdm", "lars", lambda: optimizers.SGD(0.1, momentum=0.9, weight_decay=1e-4),
             lambda: optimizers.LARS(0.1, momentum=0.9, weight_decay=1e-4, exclude_from_weight_decay=ex))]:
        (ob, ab), (on, an) = make(mk_base(), shapes, dev), make(mk_new(), shapes, dev)
        n = ab.numel
        evs = {base_name: [], new_name: []}
        for it in range(args.warmup + args.iters):
            for nm, o, a in ((base_name, ob, ab), (new_name, on, an)):
                a.grad.normal_()
                e = timed(lambda: o.apply_arena(a, zero_grad=True))
                if it >= args.warmup:
                    evs[nm].append(e)
        torch.cuda.synchronize()
        med = {k: statistics.median(x.elapsed_time(y) for x, y in v) for k, v in evs.items()}
        lo = {k: min(x.elapsed_time(y) for x, y in v) for k, v in evs.items()}
        hi = {k: max(x.elapsed_time(y) for x, y in v) for k, v in evs.items()}
        for k in (base_name, new_name):
            lines.append(f"{k:6s} {n / 1e6:7.1f} M elements  median {med[k] * 1e3:8.1f} us  (min {lo[k] * 1e3:.1f}, "
                         f"max {hi[k] * 1e3:.1f})  {BYTES[k]} B/element  {BYTES[k] * n / med[k] / 1e9:6.3f} TB/s")
        ratios[new_name] = med[new_name] / med[base_name]
        lines.append(f"{new_name}/{base_name} time ratio {ratios[new_name]:.3f}  (bytes ratio "
                     f"{BYTES[new_name] / BYTES[base_name]:.3f})")
        # the three launches one by one
        plan, kw = on._lw_plan(an), on._kernel_kwargs()
        hp = on._hp[id(an)]
        s = [an.slots[x] for x in on.get_slot_names()]
        lamb = new_name == "lamb"
        per = [[], [], []]
        for it in range(args.warmup + args.iters):
            an.grad.normal_()
            if lamb:
                e1 = timed(lambda: O.layerwise_pass1("lamb", plan, an.flat, an.grad, s[0], s[1], hp, b1=kw["b1"],
                                                     b2=kw["b2"], eps=kw["eps"], wd=kw["wd"]))
            else:
                e1 = timed(lambda: O.layerwise_pass1("lars", plan, an.flat, an.grad, None, None, hp))
            e2 = timed(lambda: O.layerwise_finalize(new_name, plan, wd=kw["wd"], eeta=kw.get("eeta", 0.0),
                                                    eps=kw["eps"]))
            e3 = timed(lambda: O.layerwise_pass2(new_name, plan, an.flat, an.grad, None if lamb else s[0], an.bf16,
                                                 hp, wd=kw["wd"], mom=kw.get("mom", 0.0)))
            if it >= args.warmup:
                for p, e in zip(per, (e1, e2, e3)):
                    p.append(e)
        torch.cuda.synchronize()
        m = [statistics.median(x.elapsed_time(y) for x, y in p) for p in per]
        b1, b2 = PASS_BYTES[new_name]
        lines.append(f"{new_name} pass 1   median {m[0] * 1e3:8.1f} us  {b1} B/element  {b1 * n / m[0] / 1e9:6.3f} TB/s")
        lines.append(f"{new_name} finalize median {m[1] * 1e3:8.1f} us  ({plan.ntiles} tiles, {plan.nvars} variables)")
        lines.append(f"{new_name} pass 2   median {m[2] * 1e3:8.1f} us  {b2} B/element  {b2 * n / m[2] / 1e9:6.3f} TB/s")
        lines.append("")
        del ob, ab, on, an, plan, s, hp
        torch.cuda.empty_cache()
    head = [f"tools/bench_optim.py on {torch.cuda.get_device_name(0)}: GPT-2-medium arena ({len(shapes)} variables), "
            f"{args.iters} timed iterations after {args.warmup} warm-up, device events, medians", ""]
    text = "\n".join(head + lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
