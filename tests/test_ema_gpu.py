"""The weight-averaging kernels (csrc/kernels/ema.hip) and ``FlatEMA`` on the GPU: the update
kernel against the fp64 recursion (accuracy rule of ema_reference.py) over sizes, pointer phases
and launch cuts, the skipped call, the exact exchange, the prep kernel's scalars, whole engines
(ResNet-18, a small ViT), evaluation by in-place exchange, replay of a captured step with
device-resident counters, and balanced-shard mode at world 1."""
import os
import subprocess
import sys

import pytest
import torch

from ema_reference import RefEMA, check_rule, check_scalars

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 8  # guard elements on both sides of every kernel operand
SENTINEL = 7.0
# one sweep of the kernels' capped grid on the 16-byte path: 8192 blocks x 256 threads x 4 elements
# (the element-wise path sweeps a quarter of that, so the same n makes it loop too)
SWEEP = 8192 * 256 * 4
SIZES = [1, 3, 63, 65, 100_003]
PHASES = [(a, b) for a in range(4) for b in range(4)]  # element offsets of (ema, p): equal and different


def _i32(t):
    return t.detach().clone().view(torch.int32)


def _guarded(n, offset, fill):
    """n fp32 elements starting GUARD + offset elements into a fresh allocation filled with ``fill``"""
    whole = torch.full((GUARD + offset + n + GUARD,), fill, dtype=torch.float32, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + n]


def _guards_intact(whole, n, offset, fill):
    lo = GUARD + offset
    g = torch.cat([whole[:lo], whole[lo + n:]])
    want = torch.full_like(g, fill)
    return torch.equal(_i32(g), _i32(want))


def _state(decay, calls=0.0, updates=0.0):
    return torch.tensor([calls, updates, 0.0, decay, 0.0], dtype=torch.float64, device="cuda")


def _run_update_kernel(n, off_e=0, off_p=0, steps=4, decay=0.9, warmup=3):
    from mi355x_dp.ops import ema_prep_, ema_update_
    gen = torch.Generator(device="cuda").manual_seed(n % 9973 + 17 * off_e + 5 * off_p)
    whole_e, e = _guarded(n, off_e, SENTINEL)
    whole_p, p = _guarded(n, off_p, float("nan"))
    e.copy_(torch.randn(n, device="cuda", generator=gen))
    state = _state(decay)
    ref = RefEMA([e], decay, warmup=warmup)
    for step in range(steps):
        p.copy_(torch.randn(n, device="cuda", generator=gen) * (1.0 + step))
        ema_prep_(state, warmup, 1)
        ema_update_(e, p, state)
        ref.update([p])
        torch.cuda.synchronize()
        check_scalars(state, ref, f"n={n} offsets=({off_e},{off_p}) step {step}")
        check_rule(e, ref, f"n={n} offsets=({off_e},{off_p}) step {step}")
    assert _guards_intact(whole_e, n, off_e, SENTINEL), "ema: wrote outside its range"
    assert _guards_intact(whole_p, n, off_p, float("nan")), "p: written"
    return e


# --------------------------------------------------------------------------- 1. update kernel
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_matches_fp64(n):
    _run_update_kernel(n)


def test_update_kernel_empty_range():
    from mi355x_dp.ops import ema_update_
    whole_e, e = _guarded(0, 0, SENTINEL)
    whole_p, p = _guarded(0, 0, float("nan"))
    ema_update_(e, p, _state(0.9))
    torch.cuda.synchronize()
    assert _guards_intact(whole_e, 0, 0, SENTINEL)


@pytest.mark.parametrize("phase", [(0, 0), (1, 3)])
def test_update_kernel_second_grid_stride_trip(phase):
    """n beyond one sweep of the capped grid: the grid-stride loop takes a second trip.  Same
    reference and rule (k = 1), the fp64 side computed on the device: 8 M elements through the
    host would take seconds."""
    from ema_reference import host_scalars
    from mi355x_dp.ops import ema_prep_, ema_update_
    n, (off_e, off_p) = SWEEP + 323, phase
    gen = torch.Generator(device="cuda").manual_seed(7)
    whole_e, e = _guarded(n, off_e, SENTINEL)
    whole_p, p = _guarded(n, off_p, float("nan"))
    e.copy_(torch.randn(n, device="cuda", generator=gen))
    p.copy_(torch.randn(n, device="cuda", generator=gen))
    M = max(float(e.abs().max()), float(p.abs().max()))
    want = e.double()
    _c, _n, w, d = host_scalars(0, 0, 0.9, 3, 1)
    want.add_(w * (p.double() - want))
    state = _state(0.9)
    ema_prep_(state, 3, 1)
    ema_update_(e, p, state)
    torch.cuda.synchronize()
    assert abs(state.tolist()[2] - w) <= 2 * 2.0 ** -52 and w > 0.5
    err = float((e.double() - want).abs().max())
    print(f"n={n} offsets={phase}: max |fp32 - fp64| {err:.3e}, bound {8 * 2.0 ** -24 * M:.3e}")
    assert err <= 8 * 2.0 ** -24 * M
    assert _guards_intact(whole_e, n, off_e, SENTINEL) and _guards_intact(whole_p, n, off_p, float("nan"))


@pytest.mark.parametrize("n", [1, 3, 63, 65, 1003])
def test_update_kernel_unaligned_pointers(n):
    """operands 0-3 elements past a 16-byte boundary, the same and different for the two: guards
    of NaN around p and of a sentinel around ema stay, and the rule holds at every phase"""
    for off_e, off_p in PHASES:
        _run_update_kernel(n, off_e, off_p, steps=2)


def test_update_kernel_phase_does_not_change_the_bits():
    """the same values at every pointer phase give the same bits (one fmaf per element on either path)"""
    from mi355x_dp.ops import ema_prep_, ema_update_
    n = 1003
    gen = torch.Generator(device="cuda").manual_seed(11)
    e0, p0 = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)
    outs = []
    for off_e, off_p in PHASES:
        whole_e, e = _guarded(n, off_e, SENTINEL)
        whole_p, p = _guarded(n, off_p, float("nan"))
        e.copy_(e0), p.copy_(p0)
        state = _state(0.75)
        ema_prep_(state, None, 1)
        ema_update_(e, p, state)
        torch.cuda.synchronize()
        assert _guards_intact(whole_e, n, off_e, SENTINEL) and _guards_intact(whole_p, n, off_p, float("nan"))
        outs.append(_i32(e))
    assert all(torch.equal(o, outs[0]) for o in outs)
    want = e0.double() + 0.25 * (p0.double() - e0.double())
    M = max(float(e0.abs().max()), float(p0.abs().max()))
    assert float((outs[0].view(torch.float32).double() - want).abs().max()) <= 8 * 2.0 ** -24 * M  # the rule, k = 1


def test_update_kernel_launch_cuts():
    """one launch over [0, n) against the same range cut at arbitrary, unaligned points"""
    from mi355x_dp.ops import ema_prep_, ema_update_
    n = 100_003
    gen = torch.Generator(device="cuda").manual_seed(5)
    e0, p = torch.randn(n, device="cuda", generator=gen), torch.randn(n, device="cuda", generator=gen)
    state = _state(0.9)
    ema_prep_(state, 4, 1)
    one, cut = e0.clone(), e0.clone()
    ema_update_(one, p, state)
    cuts = [0, 1, 6, 70, 4099, 50_001, 99_999, n]
    for lo, hi in zip(cuts, cuts[1:]):
        ema_update_(cut[lo:hi], p[lo:hi], state)
    torch.cuda.synchronize()
    assert not torch.equal(one, e0)
    assert torch.equal(_i32(one), _i32(cut))


@pytest.mark.parametrize("phase", [(0, 0), (2, 1)])
def test_skipped_call_leaves_the_average_bit_identical(phase):
    from mi355x_dp.ops import ema_prep_, ema_update_
    n = 70_001
    whole_e, e = _guarded(n, phase[0], SENTINEL)
    whole_p, p = _guarded(n, phase[1], float("nan"))
    e.copy_(torch.randn(n, device="cuda"))
    ev = e.view(torch.int32)
    ev[0], ev[1], ev[2], ev[3] = 0x7FC12345, -0x80000000, 1, 0x7F800000  # NaN payload, -0, denormal, inf
    p.copy_(torch.randn(n, device="cuda"))
    before = _i32(e)
    state = _state(0.9)
    ema_prep_(state, None, 2)  # call 1 of every=2: skips
    torch.cuda.synchronize()
    assert state.tolist()[:3] == [1.0, 0.0, 0.0]
    ema_update_(e, p, state)
    torch.cuda.synchronize()
    assert torch.equal(_i32(e), before)
    ema_prep_(state, None, 2)  # call 2 updates
    ema_update_(e, p, state)
    torch.cuda.synchronize()
    assert state.tolist()[:2] == [2.0, 1.0] and not torch.equal(_i32(e)[4:], before[4:])
    assert _guards_intact(whole_e, n, phase[0], SENTINEL)


# ----------------------------------------------------------------------------- 2. swap kernel
def _special(n, seed):
    """random bit patterns: NaN payloads, infinities, signed zeros and denormals included"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    t = torch.randint(-2 ** 31, 2 ** 31, (n,), dtype=torch.int64, device="cuda", generator=gen).to(torch.int32)
    fixed = torch.tensor([0x7FC12345, -0x3EDCBB,0x7F800000, -0x800000, 0, -0x80000000, 1, -0x7FFFFFFF, 0x7FFFFF],
                         dtype=torch.int32, device="cuda")  # qNaN, NaN (sign set), +-inf, +-0, denormals
    k = min(n, fixed.numel())
    t[:k] = fixed[:k]
    return t


@pytest.mark.parametrize("n", SIZES + [SWEEP + 323])
def test_swap_kernel_exact(n):
    from mi355x_dp.ops import ema_swap_
    phases = PHASES if n < 100_000 else [(0, 0), (1, 3)]
    for off_a, off_b in phases:
        whole_a, a = _guarded(n, off_a, SENTINEL)
        whole_b, b = _guarded(n, off_b, float("nan"))
        a0, b0 = _special(n, 1), _special(n, 2).flip(0)
        a.view(torch.int32).copy_(a0), b.view(torch.int32).copy_(b0)
        ema_swap_(a, b)
        torch.cuda.synchronize()
        assert torch.equal(_i32(a), b0) and torch.equal(_i32(b), a0), (n, off_a, off_b)
        ema_swap_(a, b)
        torch.cuda.synchronize()
        assert torch.equal(_i32(a), a0) and torch.equal(_i32(b), b0), (n, off_a, off_b)
        assert _guards_intact(whole_a, n, off_a, SENTINEL) and _guards_intact(whole_b, n, off_b, float("nan"))


# ----------------------------------------------------------------------------- 3. prep kernel
def test_prep_kernel_matches_host_formula():
    from mi355x_dp.ops import ema_prep_
    state = _state(0.999)
    ref = RefEMA([], 0.999, warmup=10, every=3)
    seen = set()
    for call in range(25):
        ema_prep_(state, 10, 3)
        ref.update([])
        check_scalars(state, ref, f"call {call}")
        seen.add(ref.w == 0.0)
    assert seen == {True, False} and ref.c == 25 and ref.n == 8
    # no warm-up, every call: w = 1 - decay
    state = _state(0.75)
    ema_prep_(state, None, 1)
    assert state.tolist() == [1.0, 1.0, 0.25, 0.75, 0.75]


# --------------------------------------------------------------------------------- 4. engines
def _resnet18_engine():
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import augment, cross_entropy
    from mi355x_dp.parallel import DataParallel, FlatSGD
    torch.manual_seed(0)
    eng = DataParallel(get_model("resnet18", num_classes=10).cuda())
    opt = FlatSGD(eng, lr=0.05, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator(device="cuda").manual_seed(3)
    imgs = torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 10, (8,), device="cuda", generator=g)
    x = augment(imgs, 8, (0.49, 0.48, 0.45), (0.2, 0.2, 0.2), pad=4, flip=True, seed=0)

    def step():
        eng.train()
        eng.zero_grad()
        cross_entropy(eng(x), labels).backward()
        opt.step()
    return eng, opt, step, x


def _vit_engine(heads=4):
    from mi355x_dp.models.vit import VisionTransformer
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    torch.manual_seed(0)
    eng = DataParallel(VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=heads, hidden_dim=64,
                                         mlp_dim=128, num_classes=10).cuda())
    opt = FlatAdamW(eng, lr=1e-2, weight_decay=0.05)
    x = torch.randn(4, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
    labels = torch.arange(4, device="cuda")

    def step():
        eng.train()
        eng.zero_grad()
        torch.nn.functional.cross_entropy(eng(x).float(), labels).backward()
        opt.step()
    return eng, opt, step, x


_ENGINES = {"resnet18": _resnet18_engine, "vit": _vit_engine}


@pytest.mark.parametrize("model", ["resnet18", "vit"])
def test_engine_matches_fp64(model):
    """six steps; the reference gets fp64 copies of the engine's own master weights (and running
    statistics) after each step, which isolates the average from the training numerics"""
    from mi355x_dp.parallel import FlatEMA
    eng, opt, step, _x = _ENGINES[model]()
    mode = "average" if model == "resnet18" else "live"
    ema = FlatEMA(eng, decay=0.99, warmup=3, update_every=1, buffers=mode)
    assert len(ema.segments) == 1 and ema.avg.numel() == eng.flat.numel
    n_buf = sum(b.numel() for b in eng.buffers.buffers)
    assert (ema.avg_buffers is not None) == (model == "resnet18")
    live = lambda: [eng.flat.data] + ([eng.buffers.data[:n_buf]] if ema.avg_buffers is not None else [])  # noqa: E731
    ref = RefEMA(live(), 0.99, warmup=3)
    for k in range(6):
        step()
        ema.update()
        ref.update(live())
        torch.cuda.synchronize()
        check_scalars(ema.state, ref, f"{model} step {k}")
        check_rule(ema.avg, ref, f"{model} weights step {k}")
        if ema.avg_buffers is not None:
            check_rule(ema.avg_buffers, ref, f"{model} statistics step {k}", index=1)
    assert ema.num_updates == 6
    assert float((ema.avg - eng.flat.data).abs().max()) > 1e-5, "the average must lag the weights"


# ------------------------------------------------------------------------------- 5. applied()
@pytest.mark.parametrize("model", ["resnet18", "vit"])
def test_applied_on_the_device(model, monkeypatch):
    from mi355x_dp.parallel import FlatEMA
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    # one head of dimension 64: the attention kernels' head dimension (STRICT_NATIVE refuses any other)
    eng, opt, step, x = _resnet18_engine() if model == "resnet18" else _vit_engine(heads=1)
    ema = FlatEMA(eng, decay=0.9, buffers="average" if model == "resnet18" else "live")
    for _ in range(3):
        step()
        ema.update()
    f = eng.flat
    assert f.bf16 is not None and f.bf16_t is not None
    eng.eval()
    with torch.no_grad():
        live_out = eng(x).float().clone()
    state = [f.data, f.bf16, f.bf16_t, eng.buffers.data, ema.avg]
    snap = [t.clone() for t in state]
    avg16 = ema.avg.to(torch.bfloat16)
    kinds = set()
    with ema.applied():
        assert torch.equal(_i32(f.data), _i32(snap[4])), "flat.data must hold the average"
        assert torch.equal(f.bf16.view(torch.int16), avg16.view(torch.int16)), "bf16 copy != cast of the average"
        for p, o in zip(f.params, f.offsets):
            wt = getattr(p, "_mi_bf16_t", None)
            if wt is None:
                continue
            cast = avg16[o:o + p.numel()]
            if p.dim() == 4:
                K, C, R, S = p.shape
                want = cast.view(K, R, S, C).permute(3, 1, 2, 0).contiguous()  # [K][R][S][C] -> [C][R][S][K]
            else:
                want = cast.view(p.shape[0], p.shape[1]).t().contiguous()
            assert torch.equal(wt.view(torch.int16), want.view(torch.int16)), tuple(p.shape)
            kinds.add(p.dim())
        with torch.no_grad():
            avg_out = eng(x).float().clone()
        with pytest.raises(RuntimeError):
            ema.update()
    torch.cuda.synchronize()
    assert kinds >= ({4} if model == "resnet18" else {2}), kinds
    assert torch.isfinite(avg_out).all() and not torch.equal(avg_out, live_out)
    for t, s in zip(state, snap):
        view = torch.int32 if t.dtype == torch.float32 else torch.int16
        assert torch.equal(t.view(view), s.view(view)), "applied() did not restore bit for bit"


# --------------------------------------------------------------------------- 6. graph replay
def test_graphed_step_replays_device_counters():
    """Six replays of ONE captured step against six eager steps from the same start, with
    ``warmup=4, update_every=2``: calls 1, 3, 5 skip and calls 2, 4, 6 update with three different
    weights.  An average that bakes its weight (or its skip decision) on the host replays the
    captured call's behaviour six times and fails."""
    from mi355x_dp.graphs import GraphedStep
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import augment, cross_entropy
    from mi355x_dp.parallel import DataParallel, FlatEMA, FlatSGD
    torch.manual_seed(0)
    eng = DataParallel(get_model("resnet18", num_classes=10).cuda())
    opt = FlatSGD(eng, lr=0.01, momentum=0.9, weight_decay=1e-4)
    ema = FlatEMA(eng, decay=0.9, warmup=4, update_every=2, buffers="average")
    g = torch.Generator(device="cuda").manual_seed(3)
    imgs = torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 10, (8,), device="cuda", generator=g)
    mean, std = (0.49, 0.48, 0.45), (0.2, 0.2, 0.2)
    x = torch.empty((8, 8, 32, 32), dtype=torch.bfloat16, device="cuda", memory_format=torch.channels_last)

    def core():
        eng.zero_grad()
        loss = cross_entropy(eng(x), labels)
        loss.backward()
        opt.step()
        ema.update()
        return loss

    def load(seed):
        augment(imgs, 8, mean, std, pad=4, flip=True, seed=seed, out=x)

    load(0)
    core()                                   # eager first step (optimizer first-step semantics)
    gs = GraphedStep(core, warmup=1)         # one more eager step on a side stream, then capture
    state = [eng.flat.data, eng.flat.bf16, opt.momentum_buf, eng.buffers.data, ema.avg, ema.avg_buffers, ema.state]
    if eng.flat.bf16_t is not None:
        state.append(eng.flat.bf16_t)
    # a fresh start for both runs: counters at zero, the average equal to the weights
    ema.state[:3].zero_()
    ema.avg.copy_(eng.flat.data)
    ema.avg_buffers.copy_(eng.buffers.data[:ema.avg_buffers.numel()])
    snap = [t.clone() for t in state]

    def restore():
        for t, s in zip(state, snap):
            t.copy_(s)

    def run(fn, seeds, decay_at=None):
        restore()
        ref = RefEMA([eng.flat.data, eng.buffers.data[:ema.avg_buffers.numel()]], 0.9, warmup=4, every=2)
        for i, seed in enumerate(seeds):
            if i == decay_at:
                ema.decay = ref.decay = 0.2  # below the warm-up ramp, so it is what d_t becomes
                ema.sync_hyper()
            load(seed)
            fn()
            ref.update([eng.flat.data, eng.buffers.data[:ema.avg_buffers.numel()]])
        torch.cuda.synchronize()
        check_scalars(ema.state, ref, fn.__class__.__name__)
        check_rule(ema.avg, ref, "weights")
        check_rule(ema.avg_buffers, ref, "statistics", index=1)
        out = [t.clone() for t in (ema.avg, ema.avg_buffers, ema.state, eng.flat.data)]
        ema.decay = 0.9
        return out

    seeds = (7, 8, 9, 10, 11, 12)
    eager = run(core, seeds)
    graph = run(gs, seeds)
    assert gs.replays == 6
    assert graph[2].tolist()[:2] == [6.0, 3.0], "the device counters must advance on every replay"
    step_change = float((eager[3] - snap[0]).abs().max())
    print(f"training weights |graph - eager| {float((graph[3] - eager[3]).abs().max()):.3e} "
          f"(change over the six steps {step_change:.3e}); "
          f"average |graph - eager| {float((graph[0] - eager[0]).abs().max()):.3e}")
    assert torch.equal(graph[2], eager[2]), "state block differs"
    assert torch.equal(_i32(graph[0]), _i32(eager[0])), "averaged weights differ"
    assert torch.equal(_i32(graph[1]), _i32(eager[1])), "averaged statistics differ"

    # a new decay reaches a replay through sync_hyper()
    eager = run(core, seeds[:4], decay_at=2)
    graph = run(gs, seeds[:4], decay_at=2)
    assert graph[2].tolist()[3] == 0.2 and graph[2].tolist()[4] == 0.2, "the new decay did not reach the replay"
    assert torch.equal(graph[2], eager[2]) and torch.equal(_i32(graph[0]), _i32(eager[0]))


# ------------------------------------------------------------------- 7. shard mode at world 1
_SHARD_CHILD = r'''
import os, sys, torch, torch.distributed as dist
sys.path.insert(0, os.environ["ROOT"]); sys.path.append(os.path.join(os.environ["ROOT"], "compat"))
sys.path.insert(0, os.path.join(os.environ["ROOT"], "tests"))
backend = os.environ["BACKEND"]
torch.cuda.set_device(0)
if backend == "smddp":
    import smdistributed.dataparallel.torch.torch_smddp
    dist.init_process_group(backend="smddp")
else:
    dist.init_process_group(backend="nccl", device_id=torch.device("cuda", 0))
from mi355x_dp.models.vit import VisionTransformer
from mi355x_dp.parallel import DataParallel, FlatAdamW, FlatEMA
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)  # several buckets on a small model
x = torch.randn(4, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
labels = torch.arange(4, device="cuda")
def vit():
    torch.manual_seed(0)
    return VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=4, hidden_dim=64, mlp_dim=128,
                             num_classes=10).cuda()
def i32(t):
    return t.detach().clone().view(torch.int32)
a = DataParallel(vit(), shard_optimizer=True, force_comm=True, **PLAN)
b = DataParallel(vit(), **PLAN)
assert a.comm_on and a.sharded and not b.comm_on and len(a.buckets) > 1
oa, ob = FlatAdamW(a, **HYPER), FlatAdamW(b, **HYPER)
ea, eb = FlatEMA(a, decay=0.9, warmup=2), FlatEMA(b, decay=0.9, warmup=2)
assert len(ea.segments) == len(a.buckets) and len(eb.segments) == 1 and ea.avg.numel() == eb.avg.numel()
for step in range(3):
    a.zero_grad()
    torch.nn.functional.cross_entropy(a(x).float(), labels).backward()   # reduce-scatter per bucket
    a.finish_gradient_sync()
    torch.cuda.synchronize()
    b.flat.grad.copy_(a.flat.grad)           # the unsharded engine sees the same gradients
    oa.step(); ob.step()
    ea.update(); eb.update()                 # while the parameter all-gather of a is in flight
    a.wait_param_sync()
    torch.cuda.synchronize()
    assert torch.equal(a.flat.data, b.flat.data), f"step {step}: shard != unsharded"
    for lo, hi, off in ea.segments:
        assert torch.equal(i32(ea.avg[off:off + hi - lo]), i32(eb.avg[lo:hi])), f"step {step}: averages differ"
    assert torch.equal(ea.state, eb.state)
assert ea.num_updates == 3 and float((eb.avg - b.flat.data).abs().max()) > 1e-5
snap = [t.clone() for t in (a.flat.data, a.flat.bf16, a.flat.bf16_t, ea.avg)]
sa, sb = ea.module_state_dict(), eb.module_state_dict()
assert set(sa) == set(sb)
for k in sa:
    assert torch.equal(sa[k], sb[k]), k
with ea.applied():
    assert torch.equal(a.flat.bf16, a.flat.data.to(torch.bfloat16))
    for lo, hi, off in ea.segments:
        assert torch.equal(i32(a.flat.data[lo:hi]), i32(snap[3][off:off + hi - lo]))
    a.eval()
    with torch.no_grad():
        assert torch.isfinite(a(x).float()).all()
    a.train()
torch.cuda.synchronize()
for t, s in zip((a.flat.data, a.flat.bf16, a.flat.bf16_t, ea.avg), snap):
    v = torch.int32 if t.dtype == torch.float32 else torch.int16
    assert torch.equal(t.view(v), s.view(v)), "applied() did not restore"
print("SHARD_OK")
sys.stdout.flush()
os._exit(0)
'''


@pytest.mark.parametrize("backend", ["smddp", "nccl"])
def test_shard_mode_world1_matches_unsharded(backend):
    """Balanced-shard mode through a real process group at world 1 (``force_comm``): one update
    launch per bucket shard into the packed average, bit-identical to the unsharded ``FlatEMA``
    (same element-wise math, only the launch boundaries differ); ``applied()`` exchanges the
    shards, all-gathers and round-trips."""
    env = {**os.environ, "ROOT": ROOT, "BACKEND": backend, "MASTER_ADDR": "127.0.0.1",
           "MASTER_PORT": str(29660 + (backend == "nccl")), "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}
    r = subprocess.run([sys.executable, "-c", _SHARD_CHILD], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "SHARD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
