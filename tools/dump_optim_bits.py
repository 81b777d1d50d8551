#!/usr/bin/env python
"""SHA-256 digests of everything the flat optimizers and their kernels compute, for comparing two
checkouts bit for bit (a refactor of ``parallel/optim.py``, ``csrc/kernels/optim.hip`` or the
optimizer section of ``ops/functional.py`` must leave every digest as it was).

    python tools/dump_optim_bits.py --device cpu|cuda > bits.json      # in each checkout; then diff

Only the public surface is used (``mi355x_dp.parallel``, ``mi355x_dp.ops``), so the same file runs
on both sides.  One JSON object is printed:

* engine level: ``FlatSGD`` / ``FlatAdamW`` / ``FlatLARS`` / ``FlatLAMB`` on the ResNet-18 and the
  small ViT engines, three steps on seeded gradients with ``lr`` changed before the third, then a
  checkpoint round trip (``state_dict`` -> ``torch.save`` -> fresh optimizer) and a fourth step; on
  ``cuda`` also balanced-shard mode at world 1 through a real process group;
* kernel level: every kernel family on a 16-byte aligned buffer and on one offset by an element
  (the scalar path), at sizes around the vector width, the unit size and one grid sweep.

The digests depend on the compiler and the torch build: compare runs of one machine only.
"""
import argparse
import hashlib
import io
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.append(os.path.join(ROOT, "compat"))

UNIT = 64
SQNORM_SWEEP = 1024 * 256 * 4  # one sweep of grad_sqnorm_'s capped grid
SWEEP = 8192 * 256 * 4         # one sweep of the elementwise kernels' capped grid
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)  # several buckets on the small ViT


def digest(t):
    if t is None or not torch.is_tensor(t):
        return repr(t)
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


# ------------------------------------------------------------------------------------ engines
def make_model(name, dev):
    torch.manual_seed(0)
    if name == "resnet18":
        from mi355x_dp.models import get_model
        return get_model("resnet18", num_classes=10).to(dev)
    from mi355x_dp.models.vit import VisionTransformer
    return VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=4, hidden_dim=64, mlp_dim=128,
                             num_classes=10).to(dev)


def make_optimizer(kind, eng):
    from mi355x_dp.parallel import FlatAdamW, FlatLAMB, FlatLARS, FlatSGD
    if kind == "sgd":
        return FlatSGD(eng, lr=0.05, momentum=0.9, weight_decay=1e-4)
    if kind == "adamw":
        return FlatAdamW(eng, lr=1e-3, weight_decay=0.05, max_grad_norm=0.5)
    if kind == "lars":
        return FlatLARS(eng, lr=0.05, momentum=0.9, weight_decay=1e-4)
    return FlatLAMB(eng, lr=1e-3, weight_decay=0.01, max_grad_norm=0.5)


def optimizer_digests(opt):
    f = opt.engine.flat
    out = {"flat.data": digest(f.data), "flat.bf16": digest(f.bf16), "steps": opt.steps}
    for name in ("momentum_buf", "exp_avg", "exp_avg_sq", "state", "last_grad_norm"):
        if getattr(opt, name, None) is not None:
            out[name] = digest(getattr(opt, name))
    if hasattr(opt, "last_trust_ratios"):
        out["trust_ratios"] = digest(opt.last_trust_ratios[0])
    return out


def engine_case(model, kind, dev, **engine_kw):
    from mi355x_dp.parallel import DataParallel

    def fresh():
        eng = DataParallel(make_model(model, dev), **engine_kw)
        return eng, make_optimizer(kind, eng)
    eng, opt = fresh()
    f = eng.flat
    mask = torch.zeros(f.numel, device=dev)  # alignment padding keeps a zero gradient
    for p, o in zip(f.params, f.offsets):
        mask[o:o + p.numel()] = 1
    gen = torch.Generator(device=dev).manual_seed(1)

    def step(e, o):
        e.flat.grad.copy_(torch.randn(f.numel, device=dev, generator=gen) * 1e-2 * mask)
        o.step()
        e.wait_param_sync()
    out = {}
    for i in range(3):
        if i == 2:
            opt.param_groups[0]["lr"] *= 0.5
        step(eng, opt)
        out[f"step{i + 1}"] = optimizer_digests(opt)
    sd = opt.state_dict()
    out["state_dict"] = {k: (digest(v) if torch.is_tensor(v) else repr(v)) for k, v in sd.items()}
    blob = io.BytesIO()
    torch.save(sd, blob)
    blob.seek(0)
    eng2, opt2 = fresh()
    eng2.flat.data.copy_(f.data)
    opt2.load_state_dict(torch.load(blob))
    step(eng2, opt2)
    out["resumed_step4"] = optimizer_digests(opt2)
    return out


# ------------------------------------------------------------------------------------ kernels
def buf(n, offset, dev, gen, dtype=torch.float32, scale=1.0):
    """n elements starting ``offset`` elements into an allocation (offset 1: no 16-byte alignment)"""
    whole = torch.randn(n + offset, device=dev, generator=gen) * scale
    return whole.to(dtype)[offset:]


def sqnorm_case(n, offset, dev):
    from mi355x_dp import ops
    gen = torch.Generator(device=dev).manual_seed(n)
    x = buf(n, offset, dev, gen)
    out = torch.zeros(1, dtype=torch.float64, device=dev)
    ops.grad_sqnorm_([x], out)
    res = {"one_segment": digest(out)}
    if n >= 255:  # three segments of the same buffer, the middle one starting unaligned
        a, b = n // 3 + 1, 2 * n // 3
        out3 = torch.zeros(1, dtype=torch.float64, device=dev)
        ops.grad_sqnorm_([x[:a], x[a:b], x[b:]], out3)
        res["three_segments"] = digest(out3)
    return res


def adamw_case(n, offset, dev):
    from mi355x_dp import ops
    gen = torch.Generator(device=dev).manual_seed(n)
    p, g = buf(n, offset, dev, gen), buf(n, offset, dev, gen, scale=0.1)
    m, v = buf(n, offset, dev, gen).zero_(), buf(n, offset, dev, gen).zero_()
    p16 = buf(n, offset, dev, gen, torch.bfloat16) if dev == "cuda" else None
    dmap = (torch.arange(2 + (n + 63) // 64, device=dev) % 2).to(torch.uint8)
    state = torch.zeros(8, dtype=torch.float64, device=dev)
    state[1] = 1e-3
    sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
    for _ in range(2):
        ops.grad_sqnorm_([g], sumsq)
        ops.adamw_prep_(state, sumsq, 0.9, 0.999, 0.05, 0.05, 0.5)
        ops.adamw_flat_(p, g, m, v, p16, state, 0.9, 0.999, 1e-8, dmap, 2)
    return {k: digest(t) for k, t in dict(p=p, m=m, v=v, p16=p16, state=state).items()}


def unit_case(kind, n, offset, dev):
    """P = 3 parameters over n / 64 units (the first excluded, one unit of padding), unit_base 3"""
    from mi355x_dp import ops
    gen = torch.Generator(device=dev).manual_seed(n)
    nu, P, base = n // UNIT, 3, 3
    pidx = torch.full((base + nu,), -1, dtype=torch.int32, device=dev)
    pidx[base:base + 2], pidx[base + 3:base + nu - 1], pidx[base + nu - 1] = 0, 1, 2
    excl = torch.tensor([1, 0, 0], dtype=torch.uint8, device=dev)
    table = torch.tensor([[0, 2], [3, nu - 1], [nu - 1, nu]], dtype=torch.int64, device=dev)
    p, g = buf(n, offset, dev, gen), buf(n, offset, dev, gen, scale=0.1)
    a, b = buf(n, offset, dev, gen).zero_(), buf(n, offset, dev, gen).zero_()
    p16 = buf(n, offset, dev, gen, torch.bfloat16) if dev == "cuda" else None
    parts = torch.zeros(2, nu, dtype=torch.float64, device=dev)
    sums = torch.zeros(2 * P, dtype=torch.float64, device=dev)
    q = torch.zeros(P, device=dev)
    state = torch.zeros(8, dtype=torch.float64, device=dev)
    state[1] = 0.05 if kind == "lars" else 1e-3
    sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
    for _ in range(2):
        if kind == "lars":
            ops.seg_sqnorm_units_(p, parts[0], g, parts[1])
            ops.seg_sqnorm_reduce_(parts, table, sums)
            ops.lars_trust_(sums, excl, q, state, 1e-3, 1e-4, 1e-8, 0.5)
            ops.lars_flat_(p, g, a, p16, state, pidx, excl, q, base, 0.9, 1e-4, 0.5)
        else:
            ops.grad_sqnorm_([g], sumsq)
            ops.lamb_prep_(state, sumsq, 0.9, 0.999, 0.05, 0.5)
            ops.lamb_moments_(p, g, a, b, state, pidx, excl, base, parts[0], parts[1], 0.9, 0.999, 1e-6, 0.01)
            ops.seg_sqnorm_reduce_(parts, table, sums)
            ops.lamb_trust_(sums, excl, q)
            ops.lamb_apply_(p, a, b, p16, state, pidx, excl, q, base, 0.9, 0.999, 1e-6, 0.01)
    return {k: digest(t) for k, t in dict(p=p, a=a, b=b, p16=p16, parts=parts, sums=sums, q=q, state=state).items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu", choices=["cpu", "cuda"])
    dev = ap.parse_args().device
    out = {}
    kinds = ("sgd", "adamw", "lars", "lamb")
    for model in ("resnet18", "vit"):
        for kind in kinds:
            out[f"engine/{model}/{kind}"] = engine_case(model, kind, dev)
    for offset in (0, 1):
        for n in (1, 63, 65, 100_003, SQNORM_SWEEP + 3):
            out[f"kernel/grad_sqnorm/n{n}/offset{offset}"] = sqnorm_case(n, offset, dev)
        for n in (1, 63, 65, 100_003):
            out[f"kernel/adamw/n{n}/offset{offset}"] = adamw_case(n, offset, dev)
        for kind in ("lars", "lamb"):
            for n in (5 * UNIT, SWEEP + 320):
                out[f"kernel/{kind}/n{n}/offset{offset}"] = unit_case(kind, n, offset, dev)
    if dev == "cuda":  # balanced shards at world 1: one launch per bucket shard, real collectives
        import torch.distributed as dist
        for k, v in dict(MASTER_ADDR="127.0.0.1", MASTER_PORT="29671", RANK="0", WORLD_SIZE="1",
                         LOCAL_RANK="0").items():
            os.environ.setdefault(k, v)
        torch.cuda.set_device(0)
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", 0))
        for kind in kinds:
            out[f"engine/vit-shard-world1/{kind}"] = engine_case("vit", kind, dev, shard_optimizer=True,
                                                                 force_comm=True, **PLAN)
        torch.cuda.synchronize()
        dist.destroy_process_group()
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
