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

``--suite ema`` times ``FlatEMA.update()`` against ``torch._foreach_lerp_`` over the parameters as
separate tensors (what ``AveragedModel`` runs), one ``lerp_`` over the whole flat buffer (the
bytes-equal floor of a library call), the enter + exit of ``FlatEMA.applied()`` and the two kernels
alone.  The update moves 12 B per element (p and ema read, ema written), the exchange 16.
``--ema-ab-lib`` names a kernel library built with the other cache policy of the update kernel
(``-DMI_EMA_NT=0/1``); its kernel is then timed in the same alternation.

    python tools/bench_optim.py --suite ema [--ema-ab-lib LIB] [--out profiles/raw/ema_flat.json]
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


def bench_ema(name, steps, rounds, warmup, ab_lib=None):
    """``FlatEMA.update()`` against ``torch._foreach_lerp_`` over the parameters as separate tensors
    (what ``AveragedModel`` runs) and one ``lerp_`` over the whole flat buffer, the exchange of
    ``applied()``, and the update kernel of this build against the one of ``ab_lib`` (a library
    built with the other cache policy), all interleaved in one process"""
    import ctypes
    from mi355x_dp import ops
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import _lib
    from mi355x_dp.parallel import DataParallel, FlatEMA
    torch.manual_seed(0)
    eng = DataParallel(get_model(name).cuda())
    f = eng.flat
    n = f.numel
    ema = FlatEMA(eng, decay=0.999)
    w = 1.0 - ema.decay
    live = [p.data for p in f.params]
    avg_list = [p.detach().clone() for p in live]  # separate allocations, as a deep copy of the module has
    avg_flat = f.data.clone()
    kernel_avg = f.data.clone()
    state = ema.state.clone()
    state[2] = w  # the kernels alone: no prep launch, a fixed weight

    def applied():
        with ema.applied():
            pass

    def policy(lib):
        return "nontemporal" if lib.mi_ema_nontemporal() else "plain"

    lib = _lib.load(True)
    kernels = {f"update_kernel_{policy(lib)} (this build)": lambda: ops.ema_update_(kernel_avg, f.data, state)}
    if ab_lib:
        alt = ctypes.CDLL(ab_lib)
        alt.mi_ema_update.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                      ctypes.c_void_p]
        alt.mi_ema_update.restype = ctypes.c_int
        assert policy(alt) != policy(lib), "--ema-ab-lib must be built with the other MI_EMA_NT"
        alt_avg = f.data.clone()

        def alt_update():
            rc = alt.mi_ema_update(_lib.ptr(alt_avg), _lib.ptr(f.data), n, _lib.ptr(state), _lib.stream_of(alt_avg))
            assert rc == 0, rc
        kernels[f"update_kernel_{policy(alt)} (A/B build)"] = alt_update
    sides = {"flat_ema_update (prep + 1 launch)": ema.update,
             "foreach_lerp (separate tensors)": lambda: torch._foreach_lerp_(avg_list, live, w),
             "lerp_ (whole flat buffer)": lambda: avg_flat.lerp_(f.data, w),
             **kernels,
             "swap_kernel": lambda: ops.ema_swap_(kernel_avg, avg_flat),
             "applied() enter + exit": applied}
    # update: p and ema read, ema written; swap: both read and written; applied(): two exchanges
    # (the two refreshes of the bf16 and transposed copies it also pays are not counted as bytes)
    payload = sum(p.numel() for p in f.params)
    nbytes = {k: 12 * n for k in sides}
    nbytes["foreach_lerp (separate tensors)"] = 12 * payload  # no alignment padding between tensors
    nbytes["swap_kernel"] = 16 * n
    nbytes["applied() enter + exit"] = 32 * n
    for fn in sides.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in sides}
    for _ in range(rounds):  # alternate the sides
        for k, fn in sides.items():
            ms[k].append(timed(fn, steps))

    # Back-to-back calls find their operands in the 256 MB last-level cache where they fit (the
    # ResNet-50 buffers do); in a training step a whole forward and backward run between two
    # updates.  Cold: 1 GiB written before every single call, one event pair per call.
    flush = torch.empty(1 << 28, dtype=torch.float32, device="cuda")
    cold = {k: fn for k, fn in sides.items() if k not in ("swap_kernel", "applied() enter + exit")}
    cms = {k: [] for k in cold}
    for _ in range(rounds):
        for k, fn in cold.items():
            pairs = []
            for _ in range(20):
                flush.zero_()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                pairs.append((a, b))
            torch.cuda.synchronize()
            cms[k].append(statistics.median(a.elapsed_time(b) for a, b in pairs))
    return {"model": name, "flat_numel": n, "payload_numel": payload, "tensors": len(f.params),
            "steps_per_measurement": steps, "rounds": rounds, "results": _rows(ms, nbytes),
            "cold_cache_single_calls": _rows(cms, nbytes)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="vitb16,resnet50")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--suite", default="adamw", choices=["adamw", "layerwise", "ema"])
    ap.add_argument("--ema-ab-lib", default=None,
                    help="--suite ema: a kernel library built with the other cache policy, e.g. "
                         "mi355x_dp.build.build_kernels(variant='emant', defines=('MI_EMA_NT=1',))")
    a = ap.parse_args()
    if a.steps < 100:
        ap.error("--steps must be at least 100")
    if a.suite == "ema":
        models = [bench_ema(m, a.steps, a.rounds, a.warmup, a.ema_ab_lib) for m in a.models.split(",")]
    else:
        models = [(bench_layerwise if a.suite == "layerwise" else bench_model)(m, a.steps, a.rounds, a.warmup)
                  for m in a.models.split(",")]
    out = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "hip": torch.version.hip,
           "suite": a.suite, "models": models}
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
