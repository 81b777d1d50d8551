#!/usr/bin/env python
"""What dropout and stochastic depth inside the fused ViT encoder layer cost (profiles/vit_drop.md).

    python tools/bench_vit_drop.py gemms [--batch 256] [--rounds 5]   # drop epilogues vs their undropped forms
    python tools/bench_vit_drop.py bwd   [--batch 256] [--rounds 5]   # mi_drop_bwd in GB/s
    python tools/bench_vit_drop.py step  [--batch 256] [--steps 20] [--warmup 5] [--rounds 3]
                                         [--configs zero,sd0.1,drop0.1]

``gemms``: each ViT-B/16 layer GEMM that can drop (proj, fc1, fc2 at M = batch x 197) with the
dropped epilogue against the epilogue it replaces, "cold" (a rotation over operand sets past the
Infinity Cache, as inside the model), interleaved rounds, medians.  ``step``: the ViT-B/16 training
step of bench.py (flat engine, FlatSGD, native cross entropy) for each configuration in one process,
the configurations interleaved round by round; one JSON line per configuration with every round's
img/s.  The ``step`` mode uses only constructor arguments, so the same file also runs against an
older tree (a configuration whose argument that tree lacks is reported as unsupported)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.environ.get("MI355X_DP_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

BF = torch.bfloat16
T_VIT, D, FF, LAYER = 197, 768, 3072, 5


def _timed(fn, sets, iters=12):
    for i in range(2):
        fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    s0, s1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s0.record()
    for i in range(iters):
        fn(sets[i % len(sets)])
    s1.record()
    torch.cuda.synchronize()
    return s0.elapsed_time(s1) / iters


def bench_gemms(a):
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops import transformer as Tm
    from mi355x_dp.ops._lib import ptr, stream_of
    _lib.load(True)
    M = a.batch * T_VIT
    blk = torch.tensor([1234, 7], dtype=torch.int64, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(0)

    def rnd(*shape):
        return (torch.rand(*shape, device="cuda", generator=g) * 2 - 1).to(BF)

    te, tr = Tm.drop_threshold(0.1), Tm.drop_threshold(0.1)
    # (name, N, K, undropped epi, drop kind, [(label, thr_e, site_e, thr_r, site_r)])
    res_masks = [("dropout 0.1", te, 8 * LAYER + 0, 0, 0), ("drop-path 0.1", 0, 0, tr, 8 * LAYER + 3),
                 ("both", te, 8 * LAYER + 0, tr, 8 * LAYER + 3)]
    cases = [("proj", D, D, Tm.EPI_RESIDUAL, Tm.DROP_RESIDUAL, res_masks),
             ("fc1", FF, D, Tm.EPI_GELU, Tm.DROP_GELU, [("dropout 0.1", te, 8 * LAYER + 1, 0, 0)]),
             ("fc2", D, FF, Tm.EPI_RESIDUAL, Tm.DROP_RESIDUAL, res_masks)]
    print("| GEMM | M N K | epilogue | ms (median) | rounds ms | vs undropped |")
    print("|---|---|---|---:|---|---:|")
    for name, N, K, epi, kind, masks in cases:
        sets = []
        for _ in range(a.sets):
            aux = rnd(M, N) if epi == Tm.EPI_RESIDUAL else torch.empty(M, N, dtype=BF, device="cuda")
            sets.append((rnd(M, K), rnd(N, K), torch.empty(M, N, dtype=BF, device="cuda"), aux,
                         torch.rand(N, device="cuda", generator=g)))

        def plain(s):
            A, W, out, aux, bias = s
            _lib.call("mi_gemm_nt_epi", ptr(A), ptr(W), ptr(out), ptr(bias), ptr(aux), epi, M, N, K, K, K, N,
                      stream_of(A))

        def dropped(mask):
            _, thr_e, site_e, thr_r, site_r = mask

            def fn(s):
                A, W, out, aux, bias = s
                _lib.call("mi_gemm_nt_epi_drop", ptr(A), ptr(W), ptr(out), ptr(bias), ptr(aux), kind, M, N, K, K, K, N,
                          ptr(blk), thr_e, site_e, thr_r, site_r, 0, T_VIT, stream_of(A))
            return fn

        fns = [("undropped (epi %d)" % epi, plain)] + [(m[0], dropped(m)) for m in masks]
        times = {label: [] for label, _ in fns}
        for _ in range(a.rounds):
            for label, fn in fns:
                times[label].append(_timed(fn, sets))
        base = statistics.median(times[fns[0][0]])
        for label, _ in fns:
            med = statistics.median(times[label])
            rounds = " ".join(f"{t:.3f}" for t in times[label])
            print(f"| {name} | {M} {N} {K} | {label} | {med:.3f} | {rounds} | {med / base:.3f}x |", flush=True)
        del sets
        torch.cuda.empty_cache()


def bench_bwd(a):
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops import transformer as Tm
    from mi355x_dp.ops._lib import ptr, stream_of
    _lib.load(True)
    M = a.batch * T_VIT
    blk = torch.tensor([1234, 7], dtype=torch.int64, device="cuda")
    sets = [((torch.randn(M, D, device="cuda")).to(BF), torch.empty(M, D, dtype=BF, device="cuda")) for _ in range(8)]
    te = Tm.drop_threshold(0.1)
    print("| mi_drop_bwd [%d][%d] | ms (median) | rounds ms | GB/s (read + write) |" % (M, D))
    print("|---|---:|---|---:|")
    for label, args in (("dropout 0.1", (te, 8 * LAYER, 0, 0)), ("drop-path 0.1", (0, 0, te, 8 * LAYER + 3)),
                        ("both", (te, 8 * LAYER, te, 8 * LAYER + 3))):
        def fn(s):
            _lib.call("mi_drop_bwd", ptr(s[0]), ptr(s[1]), M, D, ptr(blk), *args, 0, T_VIT, stream_of(s[0]))
        ts = [_timed(fn, sets, iters=40) for _ in range(a.rounds)]
        med = statistics.median(ts)
        print(f"| {label} | {med:.4f} | {' '.join(f'{t:.4f}' for t in ts)} | {2 * M * D * 2 / med / 1e6:.0f} |", flush=True)


CONFIGS = {"zero": {}, "sd0.1": {"stochastic_depth_prob": 0.1}, "drop0.1": {"dropout": 0.1},
           "both": {"dropout": 0.1, "stochastic_depth_prob": 0.1}}


def bench_step(a):
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import cross_entropy
    from mi355x_dp.parallel import DataParallel, FlatSGD
    dev = torch.device("cuda", 0)
    B, S = a.batch, 224
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn((B, 8, S, S), device=dev, generator=g).to(BF).contiguous(memory_format=torch.channels_last)
    x[:, 3:] = 0
    labels = torch.randint(0, 1000, (B,), dtype=torch.int64, device=dev, generator=g)
    runs = {}
    for name in a.configs.split(","):
        torch.manual_seed(1234)
        try:
            model = get_model("vit_b_16", num_classes=1000, **CONFIGS[name]).to(dev)
        except TypeError as e:
            print(json.dumps({"config": name, "unsupported": str(e)}), flush=True)
            continue
        engine = DataParallel(model, grad_comm="fp32", wgrad_stream="auto", shard_optimizer=False)
        opt = FlatSGD(engine, lr=0.01, momentum=0.9, weight_decay=1e-4)

        def core(engine=engine, opt=opt):
            engine.zero_grad()
            loss = cross_entropy(engine(x), labels)
            loss.backward()
            opt.step()
            return loss
        for _ in range(a.warmup):
            core()
        torch.cuda.synchronize()
        runs[name] = (core, [])
    for _ in range(a.rounds):
        for name, (core, out) in runs.items():
            core()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = core()
            torch.cuda.synchronize()
            out.append(B * a.steps / (time.perf_counter() - t0))
            assert torch.isfinite(loss.detach()).item()
    for name, (_, out) in runs.items():
        print(json.dumps({"config": name, "batch": B, "steps": a.steps, "img_s_rounds": [round(v, 1) for v in out],
                          "img_s_median": round(statistics.median(out), 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("gemms", "bwd", "step"))
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--sets", type=int, default=6)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--configs", default="zero,sd0.1,drop0.1")
    a = ap.parse_args()
    if a.rounds is None:
        a.rounds = 3 if a.mode == "step" else 5
    {"gemms": bench_gemms, "bwd": bench_bwd, "step": bench_step}[a.mode](a)


if __name__ == "__main__":
    main()
