"""The layer-wise optimizer kernels (second half of csrc/kernels/optim.hip) and ``FlatLARS`` /
``FlatLAMB`` on the GPU: the segmented squared norms (accuracy, determinism, independence of the
launch cut, owned-range tables, the scalar path), the LARS and LAMB update kernels against the
fp64 per-tensor reference (accuracy rule of layerwise_reference.py), whole engines (ResNet-18, a
small ViT), replay of a captured LAMB step, and balanced-shard mode at world 1."""
import os
import subprocess
import sys

import pytest
import torch

from layerwise_reference import LAMB, LARS, check_accuracy, layout_of, ref_pair

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNIT = 64
GUARD = 8  # sentinel elements on both sides of every kernel buffer
# one sweep of the capped grid: 8192 blocks x 256 threads x 4 elements
SWEEP = 8192 * 256 * 4
SIZES = (1, 63, 64, 65, 4097, 100_003)
UNIT_BASE = 3  # the tested range starts at unit 3 of the unit -> parameter map


def _guarded(n, offset, dtype, fill):
    """n elements starting ``offset`` elements into a fresh allocation, sentinels around them"""
    whole = torch.full((GUARD + offset + n + GUARD,), fill, dtype=dtype, device="cuda")
    return whole, whole[GUARD + offset:GUARD + offset + n]


def _guards_intact(whole, n, offset, fill):
    lo = GUARD + offset
    return bool((whole[:lo] == fill).all()) and bool((whole[lo + n:] == fill).all())


class Layout:
    """parameters of ``sizes`` elements, each aligned to 64, one no-parameter unit before, between
    and after them"""

    def __init__(self, sizes, excluded=()):
        self.ranges, off = [], UNIT
        for n in sizes:
            self.ranges.append((off, off + n))
            off += (n + UNIT - 1) // UNIT * UNIT + UNIT
        self.numel, self.P = off, len(sizes)
        self.excluded = [i in excluded for i in range(self.P)]
        pidx = torch.full((UNIT_BASE + off // UNIT,), -1, dtype=torch.int32)
        for i, (lo, hi) in enumerate(self.ranges):
            pidx[UNIT_BASE + lo // UNIT:UNIT_BASE + (hi + UNIT - 1) // UNIT] = i
        self.pidx = pidx.cuda()
        self.excl = torch.tensor(self.excluded, dtype=torch.uint8).cuda()
        self.table = torch.tensor([[lo // UNIT, (hi + UNIT - 1) // UNIT] for lo, hi in self.ranges]).cuda()
        mask = torch.zeros(off, dtype=torch.bool)
        for lo, hi in self.ranges:
            mask[lo:hi] = True
        self.mask = mask.cuda()  # True inside a parameter

    def ref_layout(self):
        return [(lo, hi, ex) for (lo, hi), ex in zip(self.ranges, self.excluded)]

    def per_param_sumsq(self, x):
        xd = x.detach().cpu().double()
        return torch.stack([(xd[lo:hi] ** 2).sum() for lo, hi in self.ranges])


def _segmented(x, table, cuts=None):
    """unit partials in one launch (or one per range of ``cuts``, in units) + the reduce; returns
    (sums, guard report)"""
    from mi355x_dp.ops import seg_sqnorm_reduce_, seg_sqnorm_units_
    nu, P = x.numel() // UNIT, table.shape[0]
    wp, parts = _guarded(nu, 0, torch.float64, -3.0)
    wo, out = _guarded(P, 0, torch.float64, -3.0)
    cuts = cuts or [0, nu]
    for a, b in zip(cuts[:-1], cuts[1:]):
        seg_sqnorm_units_(x[a * UNIT:b * UNIT], parts[a:b])
    seg_sqnorm_reduce_(parts, table, out)
    torch.cuda.synchronize()
    return out.clone(), _guards_intact(wp, nu, 0, -3.0) and _guards_intact(wo, P, 0, -3.0)


def _layout_input(lay, offset=0, seed=0):
    """random everywhere (the no-parameter units too), zero in the padding of a parameter's last unit"""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    whole, x = _guarded(lay.numel, offset, torch.float32, 7.0)
    x.copy_(torch.randn(lay.numel, device="cuda", generator=gen))
    unit_of_param = lay.pidx[UNIT_BASE:].repeat_interleave(UNIT) >= 0
    x[unit_of_param & ~lay.mask] = 0.0
    return whole, x


# ------------------------------------------------------------------------ 1. segmented norms
def test_segnorm_accurate_and_deterministic():
    lay = Layout(SIZES)
    whole, x = _layout_input(lay)
    want = lay.per_param_sumsq(x)
    outs = [_segmented(x, lay.table) for _ in range(5)]
    assert all(ok for _, ok in outs), "wrote outside the partial / output buffers"
    assert all(torch.equal(o, outs[0][0]) for o, _ in outs), "not bit-identical from run to run"
    got = outs[0][0].cpu()
    for i, n in enumerate(SIZES):
        assert float(got[i]) == pytest.approx(float(want[i]), rel=1e-9), n
    assert _guards_intact(whole, lay.numel, 0, 7.0)


def test_segnorm_parameter_longer_than_a_grid_sweep():
    lay = Layout((65, SWEEP + 320, 64))
    _, x = _layout_input(lay, seed=1)
    want = lay.per_param_sumsq(x)
    (a, ok_a), (b, ok_b) = _segmented(x, lay.table), _segmented(x, lay.table)
    assert ok_a and ok_b and torch.equal(a, b)
    for i in range(lay.P):
        assert float(a[i]) == pytest.approx(float(want[i]), rel=1e-9), i


def test_segnorm_ignores_no_parameter_units():
    lay = Layout(SIZES)
    _, x = _layout_input(lay)
    before, _ = _segmented(x, lay.table)
    x[~(lay.pidx[UNIT_BASE:].repeat_interleave(UNIT) >= 0)] = 3.0e18  # large, and finite in fp64 when squared
    after, _ = _segmented(x, lay.table)
    assert torch.equal(before, after) and bool(torch.isfinite(after).all())


def test_segnorm_independent_of_the_launch_cut():
    lay = Layout(SIZES)
    _, x = _layout_input(lay)
    nu = lay.numel // UNIT
    one, _ = _segmented(x, lay.table)
    # cuts at unit boundaries: the second inside the 4097-element parameter, the third inside the largest
    u4097 = lay.ranges[4][0] // UNIT + 20
    ubig = lay.ranges[5][0] // UNIT + 777
    three, ok = _segmented(x, lay.table, cuts=[0, u4097, ubig, nu])
    assert ok and torch.equal(one, three)


def test_segnorm_owned_ranges_add_up():
    """two "ranks" each own a slice of every parameter (one slice may be empty)"""
    lay = Layout(SIZES)
    _, x = _layout_input(lay)
    whole, _ = _segmented(x, lay.table)
    t = lay.table.cpu()
    mid = (t[:, 0] + (t[:, 1] - t[:, 0]) // 2).clamp(max=t[:, 1])
    ta = torch.stack([t[:, 0], mid], 1).contiguous().cuda()
    tb = torch.stack([mid, t[:, 1]], 1).contiguous().cuda()
    assert bool((ta[:, 0] == ta[:, 1]).any()), "expected an empty owned range (the one-unit parameters)"
    (a, _), (b, _) = _segmented(x, ta), _segmented(x, tb)
    assert torch.allclose(a + b, whole, rtol=1e-13, atol=0)
    assert bool((a[ta[:, 0] == ta[:, 1]] == 0).all())
    assert bool((a[:4] + b[:4] == whole[:4]).all())  # one-unit parameters: exact


def test_segnorm_unaligned_pointer_scalar_path():
    """a range one element into its allocation (4-byte aligned only): the same bits as the vector path"""
    lay = Layout(SIZES)
    w0, x0 = _layout_input(lay, offset=0)
    w1, x1 = _layout_input(lay, offset=1)
    assert x0.data_ptr() % 16 == 0 and x1.data_ptr() % 16 == 4 and torch.equal(x0, x1)
    (a, ok_a), (b, ok_b) = _segmented(x0, lay.table), _segmented(x1, lay.table)
    assert ok_a and ok_b and torch.equal(a, b)
    want = lay.per_param_sumsq(x1)
    for i in range(lay.P):
        assert float(b[i]) == pytest.approx(float(want[i]), rel=1e-9), i
    assert _guards_intact(w1, lay.numel, 1, 7.0)


# ------------------------------------------------------------------------- 2. update kernels
ZERO_W, ZERO_G = 2, 4     # the all-zero adapted parameter (64 elements); the all-zero gradient (4097)
EXCLUDED = (1, 3)         # the 63- and 65-element parameters


def _run_update(kind, offset=0, grad_scale=1.0, steps=5):
    from mi355x_dp import ops
    hyper = LARS if kind == "lars" else LAMB
    lay = Layout(SIZES, excluded=EXCLUDED)
    n, nu, P = lay.numel, lay.numel // UNIT, lay.P
    gen = torch.Generator(device="cuda").manual_seed(11 + offset)
    names = "pgb" if kind == "lars" else "pgmv"
    bufs = {k: _guarded(n, offset, torch.float32, 7.0) for k in names}
    w16, p16 = _guarded(n, offset, torch.bfloat16, 7.0)
    wparts, parts = _guarded(2 * nu, 0, torch.float64, -3.0)
    wsums, sums = _guarded(2 * P, 0, torch.float64, -3.0)
    wq, q = _guarded(P, 0, torch.float32, -3.0)
    parts = parts.view(2, nu)
    p, g = bufs["p"][1], bufs["g"][1]
    p.copy_(torch.randn(n, device="cuda", generator=gen) * lay.mask)
    zlo, zhi = lay.ranges[ZERO_W]
    p[zlo:zhi] = 0.0
    for k in names[2:]:
        bufs[k][1].zero_()
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    state[1] = hyper["lr"]
    ref64, ref32 = ref_pair(kind, p, lay.ref_layout(), **hyper)
    start = p.clone()
    for step in range(steps):
        g.copy_(torch.randn(n, device="cuda", generator=gen) * lay.mask * (0.1 / grad_scale))
        glo, ghi = lay.ranges[ZERO_G]
        g[glo:ghi] = 0.0
        if kind == "lars":
            b = bufs["b"][1]
            ops.seg_sqnorm_units_(p, parts[0], g, parts[1])
            ops.seg_sqnorm_reduce_(parts, lay.table, sums)
            ops.lars_trust_(sums, lay.excl, q, state, hyper["trust_coefficient"], hyper["weight_decay"],
                            hyper["eps"], grad_scale)
            ops.lars_flat_(p, g, b, p16, state, lay.pidx, lay.excl, q, UNIT_BASE, hyper["momentum"],
                           hyper["weight_decay"], grad_scale)
        else:
            m, v = bufs["m"][1], bufs["v"][1]
            b1, b2 = hyper["betas"]
            ops.lamb_prep_(state, None, b1, b2, None, grad_scale)
            ops.lamb_moments_(p, g, m, v, state, lay.pidx, lay.excl, UNIT_BASE, parts[0], parts[1], b1, b2,
                              hyper["eps"], hyper["weight_decay"])
            ops.seg_sqnorm_reduce_(parts, lay.table, sums)
            ops.lamb_trust_(sums, lay.excl, q)
            ops.lamb_apply_(p, m, v, p16, state, lay.pidx, lay.excl, q, UNIT_BASE, b1, b2, hyper["eps"],
                            hyper["weight_decay"])
        ref64.step(g, grad_scale), ref32.step(g, grad_scale)
        torch.cuda.synchronize()
        what = f"{kind} offset={offset} grad_scale={grad_scale} step {step}"
        check_accuracy(p, ref32.flat(), ref64.flat(), what)
        assert torch.equal(p16, p.to(torch.bfloat16)), "bf16 shadow differs from the master"
        assert torch.allclose(q.cpu().double(), torch.tensor(ref64.q, dtype=torch.float64), rtol=1e-5, atol=0), what
        qs = q.tolist()
        assert all(qs[i] == 1.0 for i in EXCLUDED)
        if step == 0:
            assert qs[ZERO_W] == 1.0, "an all-zero adapted parameter must get q = 1"
            assert bool((p[zlo:zhi] != 0).any()), "... and still move"
        if kind == "lars":
            assert qs[ZERO_G] == 1.0  # |g'| = 0
    assert float(state[0]) == steps
    glo, ghi = lay.ranges[ZERO_G]
    assert bool((p[glo:ghi] != start[glo:ghi]).any()), "the zero-gradient parameter still decays"
    assert bool((p[~lay.mask] == 0).all()), "padding must stay zero"
    for k in names:
        assert _guards_intact(bufs[k][0], n, offset, 7.0), f"{k}: wrote outside its segment"
    assert _guards_intact(w16, n, offset, 7.0), "p16: wrote outside its segment"
    assert _guards_intact(wparts, 2 * nu, 0, -3.0) and _guards_intact(wsums, 2 * P, 0, -3.0)
    assert _guards_intact(wq, P, 0, -3.0)
    return p.clone()


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_update_kernels_match_fp64(kind):
    _run_update(kind)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_update_kernels_unaligned_pointers(kind):
    """slices one element into their allocations (4-byte aligned only): the scalar path"""
    _run_update(kind, offset=1)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_update_kernels_grad_scale(kind):
    """grad_scale = 0.5 on doubled gradients"""
    _run_update(kind, grad_scale=0.5)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_update_kernels_second_grid_stride_trip(kind):
    """a parameter longer than one sweep of the capped grid, one step"""
    from mi355x_dp import ops
    hyper = LARS if kind == "lars" else LAMB
    lay = Layout((65, SWEEP + 320), excluded=(0,))
    n, nu, P = lay.numel, lay.numel // UNIT, lay.P
    gen = torch.Generator(device="cuda").manual_seed(5)
    p = torch.randn(n, device="cuda", generator=gen) * lay.mask
    g = torch.randn(n, device="cuda", generator=gen) * lay.mask * 0.1
    p16 = torch.zeros(n, dtype=torch.bfloat16, device="cuda")
    parts = torch.zeros(2, nu, dtype=torch.float64, device="cuda")
    sums = torch.zeros(2 * P, dtype=torch.float64, device="cuda")
    q = torch.zeros(P, device="cuda")
    state = torch.zeros(8, dtype=torch.float64, device="cuda")
    state[1] = hyper["lr"]
    ref64, ref32 = ref_pair(kind, p, lay.ref_layout(), **hyper)
    if kind == "lars":
        b = torch.zeros(n, device="cuda")
        ops.seg_sqnorm_units_(p, parts[0], g, parts[1])
        ops.seg_sqnorm_reduce_(parts, lay.table, sums)
        ops.lars_trust_(sums, lay.excl, q, state, hyper["trust_coefficient"], hyper["weight_decay"], hyper["eps"])
        ops.lars_flat_(p, g, b, p16, state, lay.pidx, lay.excl, q, UNIT_BASE, hyper["momentum"],
                       hyper["weight_decay"])
    else:
        m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        b1, b2 = hyper["betas"]
        ops.lamb_prep_(state, None, b1, b2)
        ops.lamb_moments_(p, g, m, v, state, lay.pidx, lay.excl, UNIT_BASE, parts[0], parts[1], b1, b2, hyper["eps"],
                          hyper["weight_decay"])
        ops.seg_sqnorm_reduce_(parts, lay.table, sums)
        ops.lamb_trust_(sums, lay.excl, q)
        ops.lamb_apply_(p, m, v, p16, state, lay.pidx, lay.excl, q, UNIT_BASE, b1, b2, hyper["eps"],
                        hyper["weight_decay"])
    ref64.step(g), ref32.step(g)
    torch.cuda.synchronize()
    check_accuracy(p, ref32.flat(), ref64.flat(), f"{kind} sweep")
    assert torch.equal(p16, p.to(torch.bfloat16))
    assert q.tolist()[1] == pytest.approx(ref64.q[1], rel=1e-5)


# --------------------------------------------------------------------------------- 3. engine
def _resnet18_step():
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import augment, cross_entropy
    from mi355x_dp.parallel import DataParallel
    eng = DataParallel(get_model("resnet18", num_classes=10).cuda())
    g = torch.Generator(device="cuda").manual_seed(3)
    imgs = torch.randint(0, 256, (8, 32, 32, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.randint(0, 10, (8,), device="cuda", generator=g)
    x = augment(imgs, 8, (0.49, 0.48, 0.45), (0.2, 0.2, 0.2), pad=4, flip=True, seed=0)

    def backward():
        eng.zero_grad()
        cross_entropy(eng(x), labels).backward()
    return eng, backward


def _vit():
    from mi355x_dp.models.vit import VisionTransformer
    return VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=4, hidden_dim=64, mlp_dim=128,
                             num_classes=10).cuda()


def _vit_step():
    from mi355x_dp.parallel import DataParallel
    eng = DataParallel(_vit())
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


@pytest.mark.parametrize("case", ["resnet18-lars", "vit-lamb", "vit-lamb-clip"])
def test_engine_matches_fp64(case):
    """three steps; the references get the gradients the backward produced (copied from
    flat.grad), which isolates the optimizer from bf16 forward differences"""
    from mi355x_dp.parallel import FlatLAMB, FlatLARS
    torch.manual_seed(0)
    kind = "lars" if case.endswith("lars") else "lamb"
    eng, backward = _resnet18_step() if kind == "lars" else _vit_step()
    extra = {}
    if case.endswith("clip"):
        backward()
        extra = dict(max_grad_norm=0.1 * float(eng.flat.grad.double().norm()))
    opt = FlatLARS(eng, **LARS) if kind == "lars" else FlatLAMB(eng, **LAMB, **extra)
    lay = layout_of(opt)
    rkw = dict(LARS) if kind == "lars" else dict(LAMB, **({"max_norm": extra["max_grad_norm"]} if extra else {}))
    ref64, ref32 = ref_pair(kind, eng.flat.data, lay, **rkw)
    zero_w = [i for i, (lo, hi, ex) in enumerate(lay) if not ex and bool((eng.flat.data[lo:hi] == 0).all())]
    if kind == "lamb":
        assert zero_w, "the ViT's zero-initialised head weight should exercise the |w| = 0 branch"
    start = eng.flat.data.clone()
    for step in range(3):
        backward()
        eng.finish_gradient_sync()
        g = eng.flat.grad.clone()
        opt.step()
        n64 = ref64.step(g)
        ref32.step(g)
        torch.cuda.synchronize()
        if extra:
            assert float(opt.last_grad_norm) == pytest.approx(float(n64), rel=1e-9)
            assert float(opt.last_grad_norm) > extra["max_grad_norm"], "clipping is not active"
        check_accuracy(eng.flat.data, ref32.flat(), ref64.flat(), f"{case} step {step}")
        q, names = opt.last_trust_ratios
        assert len(names) == q.numel() == len(lay)
        assert torch.allclose(q.cpu().double(), torch.tensor(ref64.q, dtype=torch.float64), rtol=1e-5, atol=0)
        if step == 0:
            moved = []
            for i in zero_w:  # |w| = 0 -> q = 1; the parameter moves where it has a gradient (u = r)
                lo, hi, _ = lay[i]
                assert float(q[i]) == 1.0, names[i]
                assert bool((eng.flat.data[lo:hi] != 0).any()) == bool((g[lo:hi] != 0).any()), names[i]
                moved.append(bool((eng.flat.data[lo:hi] != 0).any()))
            assert any(moved) or not zero_w, "the zero-initialised head weight has a gradient and must move"
        _check_compute_copies(eng)
    assert opt.steps == 3
    assert float((eng.flat.data - start).abs().max()) > 1e-3


# --------------------------------------------------------------------------- 4. graph replay
def test_graphed_lamb_step_replays_device_state():
    """Three replays of ONE captured FlatLAMB step must take steps t, t+1, t+2 (step counter and
    bias corrections on the device), and a new lr reaches a replay through sync_hyper()."""
    from mi355x_dp.graphs import GraphedStep
    from mi355x_dp.models import get_model
    from mi355x_dp.ops import augment, cross_entropy
    from mi355x_dp.parallel import DataParallel, FlatLAMB
    torch.manual_seed(0)
    eng = DataParallel(get_model("resnet18", num_classes=10).cuda())
    opt = FlatLAMB(eng, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0)
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


# ------------------------------------------------------------------- 5. shard mode at world 1
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
from layerwise_reference import LAMB, LARS, check_accuracy, layout_of, ref_pair
from mi355x_dp.models.vit import VisionTransformer
from mi355x_dp.parallel import DataParallel, FlatLAMB, FlatLARS
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)  # several buckets on a small model
x = torch.randn(4, 3, 32, 32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3))
labels = torch.arange(4, device="cuda")
def vit():
    torch.manual_seed(0)
    return VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=4, hidden_dim=64, mlp_dim=128,
                             num_classes=10).cuda()
for kind, clip in (("lars", None), ("lamb", None), ("lamb", 0.05)):
    a = DataParallel(vit(), shard_optimizer=True, force_comm=True, **PLAN)
    b = DataParallel(vit(), **PLAN)
    assert a.comm_on and a.sharded and not b.comm_on and len(a.buckets) > 1
    assert a.flat.numel == b.flat.numel and torch.equal(a.flat.data, b.flat.data)
    if kind == "lars":
        oa, ob, rkw = FlatLARS(a, **LARS), FlatLARS(b, **LARS), dict(LARS)
    else:
        oa, ob = FlatLAMB(a, max_grad_norm=clip, **LAMB), FlatLAMB(b, max_grad_norm=clip, **LAMB)
        rkw = dict(LAMB, max_norm=clip)
    assert len(oa.segments) == len(a.buckets) and len(ob.segments) == 1
    ref64, ref32 = ref_pair(kind, b.flat.data, layout_of(ob), **rkw)
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
            assert torch.equal(oa.last_trust_ratios[0], ob.last_trust_ratios[0]), f"{kind} step {step}: q differs"
            assert torch.equal(a.flat.data, b.flat.data), f"{kind} step {step}: shard != unsharded"
        else:
            assert float(oa.last_grad_norm) > clip
            assert abs(float(oa.last_grad_norm) / float(ob.last_grad_norm) - 1) < 1e-12
            check_accuracy(a.flat.data, ref32.flat(), ref64.flat(), f"shard clip step {step}")
        check_accuracy(b.flat.data, ref32.flat(), ref64.flat(), f"{kind} plain step {step}")
        assert torch.equal(a.flat.bf16, a.flat.data.to(torch.bfloat16))
print("SHARD_OK")
sys.stdout.flush()
os._exit(0)
'''


@pytest.mark.parametrize("backend", ["smddp", "nccl"])
def test_shard_mode_world1_matches_unsharded(backend):
    """Balanced-shard mode through a real process group at world 1 (``force_comm``): one launch per
    bucket shard, the per-parameter sums all-reduced, the parameters all-gathered.  Without
    clipping the result is bit-identical to the unsharded engine: a unit's partial depends on its
    64 values alone and a parameter's sum on its owned range alone, not on the launch boundaries.
    With LAMB's clipping it need not be (the GLOBAL norm is one set of block partials per segment,
    as for FlatAdamW): that case uses the accuracy rule and the norms agree to 1e-12."""
    env = {**os.environ, "ROOT": ROOT, "BACKEND": backend, "MASTER_ADDR": "127.0.0.1",
           "MASTER_PORT": str(29650 + (backend == "nccl")), "RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}
    r = subprocess.run([sys.executable, "-c", _SHARD_CHILD], capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0 and "SHARD_OK" in r.stdout, r.stdout[-3000:] + r.stderr[-4000:]
