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

``--suite layerwise`` times ``FlatLARS`` and ``FlatLAMB`` instead, interleaved in the same process
with the optimizer each extends (``FlatSGD`` with momentum, ``FlatAdamW``) on the same engine, and
then every layer-wise kernel on its own over the whole flat buffer (device events around
``--steps`` back-to-back launches).  Bytes per element: SGD 22 (p, buf read and written, g read,
bf16 written), LARS 30 (+ the norm pass reading p and g), AdamW 30, LAMB 42 (moments: p, g, m, v
read, m, v written = 24; apply: p, m, v read, p and bf16 written = 18); the fp64 unit partials add
8 B per 64 elements and array.

    python tools/bench_optim.py --suite layerwise [--out profiles/layerwise_optim.json]
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


def _rows(ms, nbytes):
    rows = {}
    for k, v in ms.items():
        med = statistics.median(v)
        rows[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                   "bytes": nbytes[k], "TBps_at_median": round(nbytes[k] / (med * 1e-3) / 1e12, 3)}
    return rows


def bench_layerwise(name, steps, rounds, warmup):
    """FlatSGD / FlatLARS / FlatAdamW / FlatLAMB steps interleaved on one engine, then the
    layer-wise kernels one by one over the whole flat buffer"""
    from mi355x_dp import ops
    from mi355x_dp.models import get_model
    from mi355x_dp.parallel import DataParallel, FlatAdamW, FlatLAMB, FlatLARS, FlatSGD
    torch.manual_seed(0)
    eng = DataParallel(get_model(name).cuda())
    f = eng.flat
    f.grad.normal_(std=1e-2)
    sgd = FlatSGD(eng, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    lars = FlatLARS(eng, lr=1e-3, momentum=0.9, weight_decay=1e-4)
    adamw = FlatAdamW(eng, lr=1e-4, weight_decay=0.05)
    lamb = FlatLAMB(eng, lr=1e-4, weight_decay=0.01)
    lamb_clip = FlatLAMB(eng, lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
    sides = {"flat_sgd": sgd.step, "flat_lars": lars.step, "flat_adamw": adamw.step, "flat_lamb": lamb.step,
             "flat_lamb_clip": lamb_clip.step}
    n = f.numel
    units = n // 64
    per_elem = {"flat_sgd": 22, "flat_lars": 30, "flat_adamw": 30, "flat_lamb": 42, "flat_lamb_clip": 46}
    nbytes = {k: n * b + (16 * units if "lars" in k or "lamb" in k else 0) for k, b in per_elem.items()}
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(rounds):  # alternate the sides
        for k, fn in sides.items():
            ms[k].append(timed(fn, steps))

    # the kernels of one LARS / LAMB step, each alone over the whole buffer
    P = len(f.params)
    parts, sums, q = lamb._unit_parts, lamb._sums, lamb._q
    hl, hm = lars.param_groups[0], lamb.param_groups[0]
    b1, b2 = hm["betas"]
    kernels = {
        "seg_sqnorm_units (p, g)": (lambda: ops.seg_sqnorm_units_(f.data, parts[0], f.grad, parts[1]),
                                    8 * n + 16 * units),
        "seg_sqnorm_reduce (2 x P blocks)": (lambda: ops.seg_sqnorm_reduce_(parts, lamb.owned_units, sums),
                                             16 * units),
        "lars_trust": (lambda: ops.lars_trust_(sums, lars.excluded, q, lars.state, hl["trust_coefficient"],
                                               hl["weight_decay"], hl["eps"]), 21 * P),
        "lars_flat": (lambda: ops.lars_flat_(f.data, f.grad, lars.momentum_buf, f.bf16, lars.state, lars.unit_param,
                                             lars.excluded, q, 0, hl["momentum"], hl["weight_decay"]), 22 * n),
        "lamb_moments": (lambda: ops.lamb_moments_(f.data, f.grad, lamb.exp_avg, lamb.exp_avg_sq, lamb.state,
                                                   lamb.unit_param, lamb.excluded, 0, parts[0], parts[1], b1, b2,
                                                   hm["eps"], hm["weight_decay"]), 24 * n + 16 * units),
        "lamb_apply": (lambda: ops.lamb_apply_(f.data, lamb.exp_avg, lamb.exp_avg_sq, f.bf16, lamb.state,
                                               lamb.unit_param, lamb.excluded, q, 0, b1, b2, hm["eps"],
                                               hm["weight_decay"]), 18 * n),
        "refresh_transposed (step tail)": (f.refresh_transposed, 0),
    }
    for fn, _ in kernels.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    kms = {k: [] for k in kernels}
    for _ in range(rounds):
        for k, (fn, _) in kernels.items():
            kms[k].append(timed(fn, steps))
    units_of = [int(b - a) for a, b in lamb.owned_units.tolist()]
    return {"model": name, "flat_numel": n, "tensors": P, "units": units, "largest_parameter_units": max(units_of),
            "steps_per_measurement": steps, "rounds": rounds, "results": _rows(ms, nbytes),
            "kernels": _rows(kms, {k: b for k, (_, b) in kernels.items()})}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="vitb16,resnet50")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--suite", default="adamw", choices=["adamw", "layerwise"])
    a = ap.parse_args()
    if a.steps < 100:
        ap.error("--steps must be at least 100")
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "suite": a.suite,
           "models": [(bench_layerwise if a.suite == "layerwise" else bench_model)(m, a.steps, a.rounds, a.warmup)
                      for m in a.models.split(",")]}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
