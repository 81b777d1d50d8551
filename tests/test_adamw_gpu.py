"""The flat AdamW kernels (csrc/kernels/optim.hip) and ``FlatAdamW`` on the GPU: the update kernel
against an fp64 reference (accuracy rule of adamw_reference.py), the deterministic squared-norm
reduction, the prep kernel's clip coefficient, whole engines (ResNet-18, a small ViT), replay of a
captured step with device-resident bias corrections, and balanced-shard mode at world 1."""
import os
import subprocess
import sys

import pytest
import torch

from adamw_reference import check_accuracy, decay_mask_of, ref_pair, ulp32

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
GUARD = 8  # sentinel elements on both sides of every kernel buffer
# one sweep of the update kernel's capped grid: 8192 blocks x 256 threads x 4 elements
SWEEP = 8192 * 256 * 4


def _guarded(n, offset, dtype, fill):
    """n elements starting ``offset`` elements into a fresh allocation, sentinels around them"""
    whole = torch.full((GUARD + offset + n + GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + n]


def _guards_intact(whole, n, offset, fill):
    lo = GUARD + offset
    return bool((whole[:lo] == fill).all()) and bool((whole[lo + n:] == fill).all())


def _run_update_kernel(n, mapped=False, offset=0, grad_scale=1.0, steps=5):
    from mi355x_dp.ops import adamw_flat_, adamw_prep_
    gen = torch.Generator(device="cuda").manual_seed(n % 9973 + 17 * offset)
    bufs = {k: _guarded(n, offset, torch.float32, 7.0) for k in "pgmv"}
    w16, p16 = _guarded(n, offset, torch.bfloat16, 7.0)
    p, g, m, v = (bufs[k][1] for k in "pgmv")
    p.copy_(torch.randn(n, device="cuda", generator=gen))
    m.zero_()
    v.zero_()
    unit_base, dmap, mask = 0, None, None
    if mapped:  # alternating decay / no-decay units, the segment starting at unit 3 of the map
        unit_base = 3
        dmap = (torch.arange(unit_base + (n + 63) // 64, device="cuda") % 2).to(torch.uint8)
        mask = dmap[unit_base:].bool().repeat_interleave(64)[:n]
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    state[1] = HYPER["lr"]
    ref64, ref32 = ref_pair(p, mask, **HYPER)
    b1, b2 = HYPER["betas"]
    for step in range(steps):
        g.copy_(torch.randn(n, device="cuda", generator=gen) * (0.1 / grad_scale))
        adamw_prep_(state, None, b1, b2, HYPER["weight_decay"], None, grad_scale)
        adamw_flat_(p, g, m, v, p16, state, b1, b2, HYPER["eps"], dmap, unit_base)
        ref64.step(g, grad_scale), ref32.step(g, grad_scale)
        torch.cuda.synchronize()
        check_accuracy(p, ref32.flat(), ref64.flat(), f"n={n} offset={offset} mapped={mapped} step {step}")
        assert torch.equal(p16, p.to(torch.bfloat16)), "bf16 shadow differs from the master"
    assert float(state[0]) == steps
    for k in "pgmv":
        assert _guards_intact(bufs[k][0], n, offset, 7.0), f"{k}: wrote outside its segment"
    assert _guards_intact(w16, n, offset, 7.0), "p16: wrote outside its segment"


# --------------------------------------------------------------------------- 1. update kernel
@pytest.mark.parametrize("n", [1, 3, 63, 65, 100_003])
def test_update_kernel_matches_fp64(n):
    _run_update_kernel(n)


def test_update_kernel_unaligned_pointers():
    """slices one element into their allocations (4-byte aligned only): the scalar path"""
    _run_update_kernel(100_003, offset=1)
    _run_update_kernel(192, mapped=True, offset=1)


@pytest.mark.parametrize("n", [64, 192, 64 * 4097])
def test_update_kernel_decay_map(n):
    _run_update_kernel(n, mapped=True)


def test_update_kernel_second_grid_stride_trip():
    _run_update_kernel(SWEEP + 320, mapped=True)


def test_update_kernel_grad_scale():
    """grad_scale = 0.5 on doubled gradients"""
    _run_update_kernel(100_003, grad_scale=0.5)


# ----------------------------------------------------------------------------- 2. norm kernel
@pytest.mark.parametrize("n,offset", [(1, 0), (255, 0), (257, 0), (257, 1), (1_048_576 + 3, 0), (3_000_001, 0),
                                      (3_000_001, 3)])
def test_sqnorm_deterministic_and_accurate(n, offset):
    from mi355x_dp.ops import grad_sqnorm_
    gen = torch.Generator(device="cuda").manual_seed(n)
    x = torch.randn(n + offset, device="cuda", generator=gen)[offset:]
    want = float((x.cpu().double() ** 2).sum())
    outs = []
    for _ in range(5):
        out = torch.zeros(1, dtype=torch.float64, device="cuda")
        grad_sqnorm_([x], out)
        outs.append(out)
    torch.cuda.synchronize()
    vals = [float(o) for o in outs]
    assert all(torch.equal(o, outs[0]) for o in outs), vals
    assert vals[0] == pytest.approx(want, rel=1e-9)
    if n >= 255:  # three segments of the same buffer, the middle one starting unaligned
        a, b = n // 3 + 1, 2 * n // 3
        out3 = torch.zeros(1, dtype=torch.float64, device="cuda")
        grad_sqnorm_([x[:a], x[a:b], x[b:]], out3)
        assert float(out3) == pytest.approx(want, rel=1e-9)
        assert float(out3) == pytest.approx(vals[0], rel=1e-9)


# --------------------------------------------------------------------------- 3. prep and clip
@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("above", [True, False])
def test_prep_clip_coefficient(above, grad_scale):
    from mi355x_dp.ops import adamw_flat_, adamw_prep_, grad_sqnorm_
    n = 70_001
    gen = torch.Generator(device="cuda").manual_seed(5)
    g = torch.randn(n, device="cuda", generator=gen) / grad_scale
    scaled = (g * grad_scale).clone().requires_grad_()
    scaled.grad = scaled.detach().clone()
    truth = float((g.cpu().double() * grad_scale).norm())
    max_norm = truth * (0.25 if above else 4.0)
    ref_norm = float(torch.nn.utils.clip_grad_norm_([scaled], max_norm))  # stock, fp32, on the device
    want_coef = min(1.0, max_norm / (truth + 1e-6))
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    state[1] = 1e-3
    sumsq = torch.zeros(1, dtype=torch.float64, device="cuda")
    grad_sqnorm_([g], sumsq)
    adamw_prep_(state, sumsq, 0.0, 0.999, 0.0, max_norm, grad_scale)
    p, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    adamw_flat_(p, g, m, v, None, state, 0.0, 0.999, 1e-8)  # beta1 = 0: exp_avg = grad_scale * coef * g
    torch.cuda.synchronize()
    st = state.tolist()
    assert st[0] == 1.0
    assert st[2] == pytest.approx(truth, rel=1e-9)
    # within the stock result's own fp32 rounding
    assert abs(st[2] - ref_norm) <= abs(ref_norm - truth) + ulp32(truth), (st[2], ref_norm, truth)
    assert st[3] == pytest.approx(want_coef, rel=1e-9) and (st[3] < 1.0) == above
    assert st[6] == pytest.approx(grad_scale * want_coef, rel=1e-9)
    applied = m.double() / g.double()
    assert float((applied - grad_scale * want_coef).abs().max()) <= 4 * ulp32(grad_scale * want_coef)
    # what stock clipping left in .grad is what the kernel applied
    assert torch.allclose(m, scaled.grad, rtol=1e-6, atol=0)


def test_prep_nonfinite_norm_propagates():
    from mi355x_dp.ops import adamw_prep_
    for bad, coef_ok in ((float("inf"), lambda c: c == 0.0), (float("nan"), lambda c: c != c)):
        state = torch.zeros(8, dtype=torch.float64, device="cuda")
        state[1] = 1e-3
        sumsq = torch.full((1,), bad, dtype=torch.float64, device="cuda")
        adamw_prep_(state, sumsq, 0.9, 0.999, 0.0, 1.0, 1.0)
        assert coef_ok(float(state[3])), (bad, float(state[3]))


# --------------------------------------------------------------------------------- 4. engine
def _resnet18_step():
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import augment, cross_entropy
    from mi355x_dp.parallel import DataParallel
    eng = DataParallel(get_model("resnet18", num_classes=10).cuda())
    g = torch.Generator(device="cuda").manual_seed(3)
    imgs = torch.randint(0, 256, (32, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 10, (32,), device="cuda", generator=g)
    x = augment(imgs, 8, (0.49, 0.48, 0.45), (0.2, 0.2, 0.2), pad=4, flip=True, seed=0)

    def backward():
        eng.zero_grad()
        cross_entropy(eng(x), labels).backward()
    return eng, backward


def _vit_step():
    from mi355x_dp.models.vit import VisionTransformer
    from mi355x_dp.parallel import DataParallel
    eng = DataParallel(VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=4, hidden_dim=64,
                                         mlp_dim=128, num_classes=10).cuda())
    x = torch.randn(4, 3, 32, 32, device="cuda")
    labels = torch.arange(4, device="cuda")

    def backward():
        eng.zero_grad()
        torch.nn.functional.cross_entropy(eng(x).float(), labels).backward()
    return eng, backward


def _check_compute_copies(eng):
    f = eng.flat
    assert torch.equal(f.bf16, f.data.to(torch.bfloat16)), "bf16 shadow differs from the master"
    n = 0
    for p in f.params:
        wt = getattr(p, "_mi_bf16_t", None)
        if wt is None:
            continue
        ref = p._mi_bf16.permute(1, 2, 3, 0) if p.dim() == 4 else p._mi_bf16.t()
        assert torch.equal(wt, ref.contiguous()), tuple(p.shape)
        n += 1
    assert n > 0


@pytest.mark.parametrize("model", ["resnet18", "vit"])
def test_engine_matches_fp64(model):
    """three steps with clipping; the references get the gradients the backward produced (copied
    from flat.grad), which isolates the optimizer from bf16 forward differences"""
    from mi355x_dp.parallel import FlatAdamW
    torch.manual_seed(0)
    eng, backward = _resnet18_step() if model == "resnet18" else _vit_step()
    backward()
    max_norm = 0.1 * float(eng.flat.grad.double().norm())
    opt = FlatAdamW(eng, max_grad_norm=max_norm, **HYPER)
    ref64, ref32 = ref_pair(eng.flat.data, decay_mask_of(opt), max_norm=max_norm, **HYPER)
    for step in range(3):
        backward()
        eng.finish_gradient_sync()
        g = eng.flat.grad.clone()
        opt.step()
        n64 = float(ref64.step(g))
        ref32.step(g)
        torch.cuda.synchronize()
        assert float(opt.last_grad_norm) == pytest.approx(n64, rel=1e-9)
        assert float(opt.last_grad_norm) > max_norm, "clipping is not active"
        check_accuracy(eng.flat.data, ref32.flat(), ref64.flat(), f"{model} step {step}")
        _check_compute_copies(eng)
    assert opt.steps == 3


# --------------------------------------------------------------------------- 5. graph replay
def test_graphed_step_replays_device_bias_corrections():
    """Three replays of ONE captured step must take steps t, t+1, t+2: the bias corrections and
    the step counter live on the device.  An optimizer that bakes them on the host replays step
    t's corrections three times (lr / bc1 differs by > 20 % between these steps) and fails."""
    from mi355x_dp.graphs import GraphedStep
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import augment, cross_entropy
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    torch.manual_seed(0)
    eng = DataParallel(get_model("resnet18", num_classes=10).cuda())
    opt = FlatAdamW(eng, lr=1e-3, weight_decay=0.05, max_grad_norm=1.0)
    g = torch.Generator(device="cuda").manual_seed(3)
    imgs = torch.randint(0, 256, (32, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 10, (32,), device="cuda", generator=g)
    mean, std = (0.49, 0.48, 0.45), (0.2, 0.2, 0.2)
    x = torch.empty((32, 8, 32, 32), dtype=torch.bfloat16, device="cuda", memory_format=torch.channels_last)

    def core():
        eng.zero_grad()
        loss = cross_entropy(eng(x), labels)
        loss.backward()
        opt.step()
        return loss

    def load(seed):
        augment(imgs, 8, mean, std, pad=4, flip=True, seed=seed, out=x)

    load(0)
    core()                                   # eager first step
    gs = GraphedStep(core, warmup=1)         # one more eager step on a side stream, then capture
    state = [eng.flat.data, eng.flat.bf16, opt.exp_avg, opt.exp_avg_sq, opt.state, eng.buffers.data]
    if eng.flat.bf16_t is not None:
        state.append(eng.flat.bf16_t)

    def snapshot():
        return [t.clone() for t in state]

    def restore(snap):
        for t, s in zip(state, snap):
            t.copy_(s)

    snap = snapshot()
    t0 = opt.steps
    assert t0 == 2
    eager, prev = [], snap[0]
    for seed in (7, 8, 9):
        load(seed)
        core()
        p = eng.flat.data.clone()
        eager.append((p, float((p - prev).abs().max())))
        prev = p
    assert opt.steps == t0 + 3
    restore(snap)
    for i, seed in enumerate((7, 8, 9)):
        load(seed)
        gs()
        torch.cuda.synchronize()
        p_eager, change = eager[i]
        diff = float((eng.flat.data - p_eager).abs().max())
        print(f"replay {i}: |graph - eager| {diff:.3e}, eager step change {change:.3e}")
        assert diff <= 1e-2 * change, (i, diff, change)
    assert gs.replays == 3 and opt.steps == t0 + 3, "the device step counter must advance on every replay"

    # a new learning rate reaches a replay through sync_hyper()
    snap = snapshot()
    opt.param_groups[0]["lr"] = 2.5e-4
    load(11)
    core()                                   # eager: step() uploads the new lr itself
    p_eager = eng.flat.data.clone()
    change = float((p_eager - snap[0]).abs().max())
    restore(snap)                            # puts the old lr back into the device state block
    assert float(opt.state[1]) == 1e-3
    opt.sync_hyper()
    load(11)
    gs()
    torch.cuda.synchronize()
    assert float(opt.state[1]) == 2.5e-4
    diff = float((eng.flat.data - p_eager).abs().max())
    print(f"replay at new lr: |graph - eager| {diff:.3e}, eager step change {change:.3e}")
    assert diff <= 1e-2 * change, (diff, change)


# ------------------------------------------------------------------- 6. shard mode at world 1
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
from adamw_reference import check_accuracy, decay_mask_of, ref_pair
from mi355x_dp.models.vit import VisionTransformer
from mi355x_dp.parallel import DataParallel, FlatAdamW
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)  # several buckets on a small model
x = torch.randn(4, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
labels = torch.arange(4, device="cuda")
def vit():
    torch.manual_seed(0)
    return VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=4, hidden_dim=64, mlp_dim=128,
                             num_classes=10).cuda()
for clip in (None, 0.05):
    a = DataParallel(vit(), shard_optimizer=True, force_comm=True, **PLAN)
    b = DataParallel(vit(), **PLAN)
    assert a.comm_on and a.sharded and not b.comm_on and len(a.buckets) > 1
    assert a.flat.numel == b.flat.numel and torch.equal(a.flat.data, b.flat.data)
    oa, ob = FlatAdamW(a, max_grad_norm=clip, **HYPER), FlatAdamW(b, max_grad_norm=clip, **HYPER)
    assert len(oa.segments) == len(a.buckets) and len(ob.segments) == 1
    ref64, ref32 = ref_pair(b.flat.data, decay_mask_of(ob), max_norm=clip, **HYPER)
    calls = a.comm_calls
    for step in range(3):
        a.zero_grad()
        torch.nn.functional.cross_entropy(a(x).float(), labels).backward()   # reduce-scatter per bucket
        a.finish_gradient_sync()
        torch.cuda.synchronize()
        b.flat.grad.copy_(a.flat.grad)           # the unsharded engine sees the same gradients
        oa.step(); ob.step()
        ref64.step(b.flat.grad), ref32.step(b.flat.grad)
        a.wait_param_sync()
        torch.cuda.synchronize()
        if clip is None:
            assert torch.equal(a.flat.data, b.flat.data), f"step {step}: shard != unsharded"
        else:
            assert float(oa.last_grad_norm) > clip
            assert abs(float(oa.last_grad_norm) / float(ob.last_grad_norm) - 1) < 1e-12
            check_accuracy(a.flat.data, ref32.flat(), ref64.flat(), f"shard clip step {step}")
            check_accuracy(b.flat.data, ref32.flat(), ref64.flat(), f"plain clip step {step}")
        assert torch.equal(a.flat.bf16, a.flat.data.to(torch.bfloat16))
    assert a.comm_calls - calls >= 3 * 2 * len(a.buckets)
print("SHARD_OK")
sys.stdout.flush()
os._exit(0)
'''


@pytest.mark.parametrize("backend", ["smddp", "nccl"])
def test_shard_mode_world1_matches_unsharded(backend):
    """Balanced-shard mode through a real process group at world 1 (``force_comm``): one update
    launch per bucket shard, the squared norm summed over the shard segments and all-reduced, the
    parameters all-gathered.  Without clipping the result is bit-identical to the unsharded engine
    (same element-wise math, only the launch boundaries differ).  With clipping it need not be:
    the squared norm is then the fixed-order sum of one set of block partials per segment instead
    of one set over the whole buffer, a different association of the same fp64 terms, so the
    coefficient can differ in its last fp64 bit and, after rounding to fp32, flip the last bit of
    some parameters.  That case uses the accuracy rule (and the norms agree to 1e-12)."""
    env = {**os.environ, "ROOT": ROOT, "BACKEND": backend, "MASTER_ADDR": "127.0.0.1",
           "MASTER_PORT": str(29640 + (backend == "nccl")), "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}
    r = subprocess.run([sys.executable, "-c", _SHARD_CHILD], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "SHARD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
