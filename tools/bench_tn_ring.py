#!/usr/bin/env python
"""1x1 stride-1 conv weight gradients (ResNet bs256 shapes, as tools/bench_wgrad256.py) on the 128-tile
TN kernel: the one-stage k-loop against the slot ring (mi_set_tn_stages), one process, interleaved
rounds, medians.  The split-K block target is read once per process:
    MI355X_DP_TN_BLOCKS=768 python tools/bench_tn_ring.py [--rounds 5] [--iters 20]
    MI355X_DP_TN_BLOCKS=384 python tools/bench_tn_ring.py"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench_wgrad256 import SHAPES  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    a = ap.parse_args()
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops import kernels  # noqa: F401
    from mi355x_dp.ops._lib import ptr, stream_of
    lib = _lib.load(True)
    lib.mi_set_wgrad256(0)
    CL, BF = torch.channels_last, torch.bfloat16
    print(f"block target {os.environ.get('MI355X_DP_TN_BLOCKS', '768 (default)')}, batch {a.batch}")
    print("| H | C | K | one-stage us | ring us | ring / one-stage | TF/s (one-stage / ring) |")
    print("|---:|---:|---:|---:|---:|---:|---:|")
    try:
        for (H, C, K) in SHAPES:
            Nb = a.batch
            x = torch.randn(Nb, C, H, H, device="cuda").to(BF).contiguous(memory_format=CL)
            dy = torch.randn(Nb, K, H, H, device="cuda").to(BF).contiguous(memory_format=CL)
            dw = torch.zeros(K, C, device="cuda")
            st = stream_of(x)

            def timed(stages):
                lib.mi_set_tn_stages(stages)
                _lib.call("mi_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), Nb, H, H, C, K, 1, 1, 1, 0, H, H, st)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    _lib.call("mi_conv2d_wgrad", ptr(x), ptr(dy), ptr(dw), Nb, H, H, C, K, 1, 1, 1, 0, H, H, st)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.iters * 1e3
            ts = {1: [], 2: []}
            for _ in range(a.rounds):
                for s in (1, 2):
                    ts[s].append(timed(s))
            t1, t2 = statistics.median(ts[1]), statistics.median(ts[2])
            fl = 2.0 * Nb * H * H * C * K
            print(f"| {H} | {C} | {K} | {t1:.1f} | {t2:.1f} | {t2 / t1:.2f} | {fl / t1 / 1e6:.0f} / {fl / t2 / 1e6:.0f} |")
    finally:
        lib.mi_set_tn_stages(0)


if __name__ == "__main__":
    main()
