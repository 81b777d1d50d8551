"""Time the fused crop-box + bilinear resample input pass (``ops.augment_resized``) on one GPU.

    python tools/bench_resized_crop.py [--out profiles/resized_crop.md] [--raw profiles/raw/resized_crop.json]

At batch 256 and a [256, 224, 224, 8] bf16 output (205.5 MB written) it times

  ``augment`` on a 224 x 224 source (the yardstick: the shift-crop kernel, same output bytes),
  ``augment_resized`` with RandomResizedCrop + RandomErasing parameters for 256^2 -> 224^2 and for
  32^2 -> 224^2, the 32^2 case with Mixup and with CutMix as well, and the evaluation transform
  (``center_params``, crop_pct 0.875) for both sources,
  and an ATen composition of the same math for both sources: ``F.affine_grid`` + ``F.grid_sample``
  on the per-image boxes (bilinear, half-pixel centres; it clamps to the image, not to the box, which
  costs the same), normalize, channel pad, bf16 ``channels_last``.  No erasing, no mixing.

The measurements run in one child process under a time limit.  The variants alternate round by round
and each round is timed with device events around ``--iters`` back-to-back calls; the table gives
the median round per call, and the spread.
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

N, S, C, COUT = 256, 224, 3, 8
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
OUT_MB = N * S * S * COUT * 2 / 1e6
SOURCES = (256, 32)


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


def measure(a):
    import torch
    import torch.nn.functional as F
    from mi355x_dp.data.crops import BatchCropper, GeoParams
    from mi355x_dp.data.mix import BatchMixer, MixParams, cutmix_box
    from mi355x_dp.ops import MixedTarget, _lib, augment, augment_resized
    _lib.load(True)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.empty((N, COUT, S, S), dtype=torch.bfloat16, device=dev, memory_format=torch.channels_last)
    labels = torch.randint(0, 1000, (N,), device=dev, generator=g)
    tgt = MixedTarget(torch.empty_like(labels), torch.empty_like(labels), torch.empty(N, device=dev))
    u224 = torch.randint(0, 256, (N, S, S, C), dtype=torch.uint8, device=dev, generator=g)
    cropper = BatchCropper(S, erase_prob=0.25, seed=1, device=dev)
    mixer = BatchMixer(device=dev)
    partner = ((torch.arange(N) - 1) % N).numpy()
    box, _ = cutmix_box(0.5, S // 2, S // 2, S, S)
    p_mixup = MixParams(*(t.clone() for t in mixer.upload(partner, [0.3] * N, [(0, 0, 0, 0)] * N)))
    p_cut = MixParams(*(t.clone() for t in mixer.upload(partner, [0.5] * N, [box] * N)))
    mean_t = torch.tensor(MEAN, device=dev).view(1, C, 1, 1)
    stdinv_t = (1.0 / torch.tensor(STD, device=dev)).view(1, C, 1, 1)

    variants = {"augment 224 (yardstick)": lambda: augment(u224, COUT, MEAN, STD, pad=4, flip=True, seed=1, out=x)}
    nbytes = {"augment 224 (yardstick)": N * S * S * C / 1e6}
    for src in SOURCES:
        u8 = torch.randint(0, 256, (N, src, src, C), dtype=torch.uint8, device=dev, generator=g)
        crop, flip, erase = cropper.host_params(0, N, src, src)
        # one persistent buffer per batch size: clone, so that the parameter sets stay distinct
        geo = GeoParams(*(t.clone() for t in cropper.upload(crop, flip, erase, src, src)))
        ev = cropper.center_params(N, src, src, crop_pct=0.875)
        in_mb = N * src * src * C / 1e6

        def fused(u8=u8, geo=geo, mix=None):
            if mix is None:
                return lambda: augment_resized(u8, S, COUT, MEAN, STD, geo, out=x)
            return lambda: augment_resized(u8, S, COUT, MEAN, STD, geo, mix=mix, labels=labels, out=x, target=tgt)

        # box -> affine map of normalized output coordinates into normalized source coordinates
        c = torch.from_numpy(crop).double()
        sx = c[:, 3] / src * (1 - 2 * torch.from_numpy(flip).double())
        theta = torch.zeros(N, 2, 3, dtype=torch.float64)
        theta[:, 0, 0], theta[:, 0, 2] = sx, (2 * c[:, 1] + c[:, 3]) / src - 1
        theta[:, 1, 1], theta[:, 1, 2] = c[:, 2] / src, (2 * c[:, 0] + c[:, 2]) / src - 1
        theta = theta.float().to(dev)

        def aten(u8=u8, theta=theta):
            f = u8.permute(0, 3, 1, 2).float()
            grid = F.affine_grid(theta, (N, C, S, S), align_corners=False)
            y = F.grid_sample(f, grid, mode="bilinear", padding_mode="border", align_corners=False)
            x[:, :C].copy_((y * (1.0 / 255.0) - mean_t) * stdinv_t)
            x[:, C:].zero_()

        variants[f"augment_resized {src} -> 224, RRC + erase"] = fused()
        variants[f"augment_resized {src} -> 224, centre crop 0.875"] = fused(geo=ev)
        variants[f"ATen grid_sample {src} -> 224"] = aten
        for k in (f"augment_resized {src} -> 224, RRC + erase", f"augment_resized {src} -> 224, centre crop 0.875",
                  f"ATen grid_sample {src} -> 224"):
            nbytes[k] = in_mb
        if src == 32:
            variants["augment_resized 32 -> 224, RRC + erase + Mixup"] = fused(mix=p_mixup)
            variants["augment_resized 32 -> 224, RRC + erase + CutMix"] = fused(mix=p_cut)
            nbytes["augment_resized 32 -> 224, RRC + erase + Mixup"] = 2 * in_mb
            nbytes["augment_resized 32 -> 224, RRC + erase + CutMix"] = in_mb
    t = _time_group(variants, a.warmup, a.rounds, a.iters)
    return {"times": t, "src_mb": nbytes, "out_mb": OUT_MB, "device": torch.cuda.get_device_name(0),
            "warmup": a.warmup, "rounds": a.rounds, "iters": a.iters}


def report(res):
    t = res["times"]
    base = statistics.median(t["augment 224 (yardstick)"])
    out = [f"Measured by `tools/bench_resized_crop.py` on {res['device']}: {res['rounds']} alternating rounds of "
           f"{res['iters']} back-to-back calls after {res['warmup']} warm-up calls, device events around each round, "
           f"microseconds per call.  Output [{N}, {S}, {S}, {COUT}] bf16 = {res['out_mb']:.1f} MB in every row.", "",
           "| variant | median us (min-max) | source MB (distinct bytes) | GB/s of output | time / `augment` | ATen / fused |",
           "|---|---:|---:|---:|---:|---:|"]
    for name, ts in t.items():
        med = statistics.median(ts)
        vs = ""
        if name.startswith("augment_resized") and name.endswith("RRC + erase"):
            src = name.split()[1]
            vs = f"{statistics.median(t[f'ATen grid_sample {src} -> 224']) / med:.1f}"
        out.append(f"| {name} | {med:.1f} ({min(ts):.1f}-{max(ts):.1f}) | {res['src_mb'][name]:.1f} | "
                   f"{res['out_mb'] / med * 1e3:.0f} | {med / base:.2f} | {vs} |")
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--timeout", type=int, default=240, help="seconds for the measuring child process")
    ap.add_argument("--out", default=None, help="write the markdown table here as well as to stdout")
    ap.add_argument("--raw", default=None, help="write every round's time here (JSON)")
    a = ap.parse_args()
    if a.child:
        print("RESULT " + json.dumps(measure(a)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child",
           "--warmup", str(a.warmup), "--rounds", str(a.rounds), "--iters", str(a.iters)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = next((ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")), None)
    if r.returncode != 0 or line is None:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        sys.stderr.write(f"\nmeasurement failed (exit {r.returncode})\n")
        return 1
    res = json.loads(line[len("RESULT "):])
    md = report(res)
    print(md)
    for path, text in ((a.out, md), (a.raw, json.dumps(res, indent=1) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
