"""Time the soft-target loss kernels and the fused augmentation + Mixup / CutMix pass on one GPU.

    python tools/bench_loss_mix.py [--out profiles/loss_mix.md]

At the bench shape (256 x 224 x 224, 3 -> 8 channels, 1000 classes) it times

  mix   ``augment`` (the baseline pass), ``augment_mix`` with identity / Mixup / CutMix parameters,
        and ``augment`` followed by the ATen composition that mixes the bf16 batch afterwards
        (``roll`` + ``lerp`` for Mixup, ``roll`` + slice copy for CutMix);
  loss  forward + backward of the hard-label kernels, of the new pair / smoothed / dense kernels, and
        of ``F.cross_entropy`` with label smoothing on hard labels and on dense [N, 1000] targets.

Each group runs in a child process of its own under a time limit; a group that fails ends the run
(nothing more is started on the GPU after it).  Within a group the variants alternate round by
round and each round is timed with device events around ``--iters`` back-to-back calls; the table
gives the median round, and the spread, per call.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, H, W, C, COUT, NCLS = 256, 224, 224, 3, 8, 1000
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IN_MB = N * H * W * C / 1e6            # uint8 batch
OUT_MB = N * H * W * COUT * 2 / 1e6    # bf16 batch


def _time_group(variants, warmup, rounds, iters):
    """variants: {name: fn}.  Alternates them round by round; returns {name: [us per call per round]}."""
    import torch
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return times


def _graphed(fn):
    """fn captured in a HIP graph (after a warm-up on the capture stream): the replay is the GPU-side cost,
    as inside a GraphedStep, without the host's per-launch overhead."""
    import torch
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        fn()
    return graph.replay


def group_mix(a):
    import torch
    from mi355x_dp.data.mix import BatchMixer, MixParams, cutmix_box
    from mi355x_dp.ops import MixedTarget, _lib, augment, augment_mix
    _lib.load(True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    u8 = torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, device=dev, generator=g)
    labels = torch.randint(0, NCLS, (N,), device=dev, generator=g)
    x = torch.empty((N, COUT, H, W), dtype=torch.bfloat16, device=dev, memory_format=torch.channels_last)
    tgt = MixedTarget(torch.empty_like(labels), torch.empty_like(labels), torch.empty(N, device=dev))
    mixer = BatchMixer(device=dev)
    partner = (torch.arange(N) - 1) % N
    box, lam_cut = cutmix_box(0.5, H // 2, W // 2, H, W)
    y0, y1, x0, x1 = box

    def params(lam, bx):
        # one persistent buffer per batch size: clone, so that the three sets stay distinct
        p = mixer.upload(partner.numpy(), [lam] * N, [bx] * N)
        return MixParams(*(t.clone() for t in p))
    p_id, p_mixup, p_cut = params(1.0, (0, 0, 0, 0)), params(0.3, (0, 0, 0, 0)), params(0.5, box)

    def fused(p):
        return lambda: augment_mix(u8, labels, COUT, MEAN, STD, p, pad=4, flip=True, seed=1, out=x, target=tgt)

    def base():
        augment(u8, COUT, MEAN, STD, pad=4, flip=True, seed=1, out=x)

    def aten_mixup():
        base()
        mixed = torch.lerp(x.roll(1, 0), x, 0.3)
        yb = labels.roll(1)
        return mixed, yb

    def aten_cutmix():
        base()
        xb = x.roll(1, 0)
        x[:, :, y0:y1, x0:x1] = xb[:, :, y0:y1, x0:x1]
        return x, labels.roll(1)

    t = _time_group({"augment": base, "augment_mix identity": fused(p_id), "augment_mix mixup": fused(p_mixup),
                     "augment_mix cutmix": fused(p_cut), "augment + ATen mixup": aten_mixup,
                     "augment + ATen cutmix": aten_cutmix}, a.warmup, a.rounds, a.iters)
    frac = (y1 - y0) * (x1 - x0) / (H * W)
    nbytes = {"augment": (IN_MB, OUT_MB), "augment_mix identity": (IN_MB, OUT_MB),
              "augment_mix mixup": (2 * IN_MB, OUT_MB), "augment_mix cutmix": (IN_MB, OUT_MB),
              # roll: read + write the batch; lerp: read two, write one
              "augment + ATen mixup": (IN_MB + 3 * OUT_MB, OUT_MB + 2 * OUT_MB),
              # roll: read + write the batch; slice copy: read + write the box
              "augment + ATen cutmix": (IN_MB + OUT_MB + frac * OUT_MB, OUT_MB + OUT_MB + frac * OUT_MB)}
    return {"times": t, "bytes_mb": nbytes, "cut_box": list(box), "device": torch.cuda.get_device_name(0)}


def group_loss(a):
    import torch
    import torch.nn.functional as F
    from mi355x_dp.ops import MixedTarget, _lib, cross_entropy
    _lib.load(True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    lg = (torch.randn(N, NCLS, device=dev, generator=g) * 3).requires_grad_()
    ya = torch.randint(0, NCLS, (N,), device=dev, generator=g)
    yb = ya.roll(1)
    lam = torch.rand(N, device=dev, generator=g)
    pair = MixedTarget(ya, yb, lam)
    dense = pair.dense(NCLS).contiguous()
    dense16 = dense.bfloat16()

    def fb(loss_fn):
        def run():
            return torch.autograd.grad(loss_fn(), lg)
        return run

    variants = {
        "native hard labels (mi_ce_fwd/bwd)": fb(lambda: cross_entropy(lg, ya)),
        "native hard labels, eps 0.1": fb(lambda: cross_entropy(lg, ya, label_smoothing=0.1)),
        "native pair target, eps 0.1": fb(lambda: cross_entropy(lg, pair, label_smoothing=0.1)),
        "native dense fp32 target, eps 0.1": fb(lambda: cross_entropy(lg, dense, label_smoothing=0.1)),
        "native dense bf16 target, eps 0.1": fb(lambda: cross_entropy(lg, dense16, label_smoothing=0.1)),
        "ATen hard labels, eps 0.1": fb(lambda: F.cross_entropy(lg, ya, label_smoothing=0.1)),
        "ATen dense target, eps 0.1": fb(lambda: F.cross_entropy(lg, dense, label_smoothing=0.1)),
        "ATen dense target built per step, eps 0.1": fb(lambda: F.cross_entropy(lg, pair.dense(NCLS), label_smoothing=0.1)),
    }
    t = _time_group(variants, a.warmup, a.rounds, a.iters)
    tg = _time_group({k: _graphed(fn) for k, fn in variants.items()}, a.warmup, a.rounds, a.iters)
    return {"times": t, "times_graphed": tg, "device": torch.cuda.get_device_name(0)}


GROUPS = {"mix": group_mix, "loss": group_loss}


def _row(name, ts, extra=""):
    return (f"| {name} | {statistics.median(ts):.1f} | {min(ts):.1f} | {max(ts):.1f} |{extra}")


def report(res, a):
    rev = subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    out = [f"Measured by `tools/bench_loss_mix.py` on {res['mix']['device']}, tree at (or on top of) commit "
           f"`{rev or 'unknown'}`: {a.rounds} alternating rounds of {a.iters} back-to-back calls after {a.warmup} "
           "warm-up calls, device events around each round, microseconds per call.", ""]
    out += [f"### Input pass: {N} x {H} x {W}, {C} -> {COUT} channels", "",
            "| variant | median us | min | max | MB read (counted) | MB written (counted) | GB/s at the median |",
            "|---|---|---|---|---|---|---|"]
    for name, ts in res["mix"]["times"].items():
        r, w = res["mix"]["bytes_mb"][name]
        out.append(_row(name, ts, f" {r:.1f} | {w:.1f} | {(r + w) / statistics.median(ts) * 1e3:.0f} |"))
    out += ["", f"CutMix box (y0, y1, x0, x1) = {tuple(res['mix']['cut_box'])}; Mixup lam = 0.3; partner = batch rolled "
            "by one.  Byte counts are what the algorithm needs, from the shapes, not counters.", ""]
    for key, how in (("times", "eager (host launch overhead included)"), ("times_graphed", "replayed from a HIP graph")):
        out += [f"### Loss forward + backward, {how}: {N} x {NCLS} fp32 logits", "",
                "| variant | median us | min | max |", "|---|---|---|---|"]
        for name, ts in res["loss"][key].items():
            out.append(_row(name, ts))
        out.append("")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--group", choices=sorted(GROUPS))
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per group (child process)")
    ap.add_argument("--out", default=None, help="write the markdown tables here as well as to stdout")
    a = ap.parse_args()
    if a.group:  # child: one group, one JSON line
        print("RESULT " + json.dumps(GROUPS[a.group](a)), flush=True)
        return 0
    res = {}
    for name in ("mix", "loss"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--group", name,
               "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--iters", str(a.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
        if r.returncode != 0 or line is None:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.stderr.write(f"\ngroup {name} failed (exit {r.returncode}); nothing more is run\n")
            return 1
        res[name] = json.loads(line[len("RESULT "):])
    md = report(res, a)
    print(md)
    if a.out:
        with open(a.out, "w") as f:
            f.write(md)
    return 0


if __name__ == "__main__":
    sys.exit(main())
