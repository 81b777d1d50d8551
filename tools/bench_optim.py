#!/usr/bin/env python
"""Time one optimizer step on a single GPU: ``FlatAdamW`` (with and without global-norm clipping)
against the foreign-optimizer path it replaces -- ``torch.optim.AdamW(fused=True)`` over the
per-parameter views plus ``clip_grad_norm_(foreach=True)``, followed by the bf16 and transposed
refresh that path pays at the next forward.  Sizes: the ViT-B/16 and the ResNet-50 flat buffers.

Method: warm up, then alternate the sides in one process; every measurement is a pair of device
events around ``--steps`` (>= 100) back-to-back steps.  Bytes are computed from the element count:
30 B per element for the update (p, m, v read and written, g read, bf16 written) plus 4 B for the
norm pass when clipping.

    python tools/bench_optim.py [--steps 200] [--rounds 5] [--out profiles/adamw_flat.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def bench_model(name, steps, rounds, warmup):
    from mi355x_dp.models import get_model
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    torch.manual_seed(0)
    eng = DataParallel(get_model(name).cuda())
    f = eng.flat
    f.grad.normal_(std=1e-2)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)
    flat_plain = FlatAdamW(eng, **hyper)
    flat_clip = FlatAdamW(eng, max_grad_norm=1.0, **hyper)
    decay = [p for p in f.params if p.ndim > 1]
    rest = [p for p in f.params if p.ndim <= 1]

    def stock_opt():
        return torch.optim.AdamW([dict(params=decay, weight_decay=hyper["weight_decay"]),
                                  dict(params=rest, weight_decay=0.0)], lr=hyper["lr"], betas=hyper["betas"],
                                 eps=hyper["eps"], fused=True)
    stock_a, stock_b = stock_opt(), stock_opt()

    def stock_plain():
        stock_a.step()
        f.refresh_bf16()  # bf16 shadow + transposed copies: what the "params dirty" hook triggers

    def stock_clip():
        torch.nn.utils.clip_grad_norm_(f.params, 1.0, foreach=True)
        stock_b.step()
        f.refresh_bf16()

    sides = {"flat_adamw": flat_plain.step, "flat_adamw_clip": flat_clip.step,
             "stock_fused": stock_plain, "stock_fused_clip": stock_clip}
    errors = {}
    for k, fn in list(sides.items()):
        try:
            for _ in range(warmup):
                fn()
        except RuntimeError as e:  # e.g. a fused stock path that refuses a layout: report, do not time
            errors[k] = str(e).splitlines()[0]
            del sides[k]
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(rounds):  # alternate the sides
        for k, fn in sides.items():
            ms[k].append(timed(fn, steps))
    n = f.numel
    rows = {}
    for k, v in ms.items():
        nbytes = n * (34 if k.endswith("clip") else 30)
        med = statistics.median(v)
        rows[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                   "bytes": nbytes, "TBps_at_median": round(nbytes / (med * 1e-3) / 1e12, 3)}
    return {"model": name, "flat_numel": n, "tensors": len(f.params), "steps_per_measurement": steps,
            "rounds": rounds, "results": rows, "errors": errors}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="vitb16,resnet50")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 100:
        ap.error("--steps must be at least 100")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "models": [bench_model(m, a.steps, a.rounds, a.warmup) for m in a.models.split(",")]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
