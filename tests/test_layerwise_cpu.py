"""FlatLARS and FlatLAMB on the host implementations (same math as the HIP kernels), single process
and gloo world 2: accuracy against the fp64 per-tensor reference with its fp32 run as the yardstick
(layerwise_reference.py), the exclude predicate, replica identity with and without balanced
shards, checkpoints through utils/checkpoint.py, and a learning-rate change between steps."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from layerwise_reference import LAMB, LARS, check_accuracy, layout_of, ref_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)
HYPER = {"lars": LARS, "lamb": LAMB}


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dist.init_process_group("gloo", rank=rank, world_size=world)


def _model():
    from mi355x_dp.models import Net
    torch.manual_seed(0)
    return Net()


def _data():
    g = torch.Generator().manual_seed(1)
    return torch.randn(16, 3, 32, 32, generator=g), torch.randint(0, 10, (16,), generator=g)


def _backward(m, x, y):
    m.zero_grad()
    F.cross_entropy(m(x), y).backward()


def _make(kind, engine, **kw):
    from mi355x_dp.parallel import FlatLAMB, FlatLARS
    return (FlatLARS if kind == "lars" else FlatLAMB)(engine, **{**HYPER[kind], **kw})


def _first_norm():
    from mi355x_dp.parallel import DataParallel
    m = DataParallel(_model(), **PLAN)
    _backward(m, *_data())
    return float(m.flat.grad.double().norm())


def _state_tensors(opt):
    return [opt.momentum_buf] if hasattr(opt, "momentum_buf") else [opt.exp_avg, opt.exp_avg_sq]


# ------------------------------------------------------------------ 1. single process vs fp64
@pytest.mark.parametrize("kind,clip", [("lars", False), ("lamb", False), ("lamb", True)])
def test_single_process_matches_fp64(kind, clip):
    """five steps; the references get the gradients the engine produced, so the comparison is of
    the optimizer alone"""
    from mi355x_dp.parallel import DataParallel
    m = DataParallel(_model(), **PLAN)
    extra = dict(max_grad_norm=0.1 * _first_norm()) if clip else {}
    opt = _make(kind, m, **extra)
    assert len(opt.segments) == 1 and all(t.numel() == m.flat.numel for t in _state_tensors(opt))
    rkw = dict(HYPER[kind], **({"max_norm": extra["max_grad_norm"]} if clip else {}))
    ref64, ref32 = ref_pair(kind, m.flat.data, layout_of(opt), **rkw)
    start = m.flat.data.clone()
    x, y = _data()
    for step in range(5):
        _backward(m, x, y)
        g = m.flat.grad.clone()
        opt.step()
        n64 = ref64.step(g)
        ref32.step(g)
        if clip:
            assert float(opt.last_grad_norm) > extra["max_grad_norm"], "clipping is not active"
            assert float(opt.last_grad_norm) == pytest.approx(float(n64), rel=1e-9)
        elif kind == "lamb":
            assert opt.last_grad_norm is None
        check_accuracy(m.flat.data, ref32.flat(), ref64.flat(), f"{kind} step {step}")
        q, names = opt.last_trust_ratios
        assert len(names) == q.numel() == len(ref64.q) and "conv1.weight" in names
        assert torch.allclose(q.double(), torch.tensor(ref64.q, dtype=torch.float64), rtol=1e-5, atol=0)
    assert opt.steps == 5
    moved = float((m.flat.data - start).abs().max())
    assert moved > 1e-3, moved  # far above the accuracy bound: a wrong trust ratio cannot hide


# --------------------------------------------------------------------------- 2. exclude map
def _zero_grad_step(kind, exclude=None):
    from mi355x_dp.parallel import DataParallel
    m = DataParallel(_model(), **PLAN)
    opt = _make(kind, m, lr=0.1, weight_decay=0.25, exclude=exclude)
    before = {n: p.detach().clone() for n, p in m.module.named_parameters()}
    m.zero_grad()
    opt.step()
    return m, opt, before


def _check_zero_grad_step(kind, m, opt, before, excluded):
    """all-zero gradients: an excluded parameter stays; an adapted one sees only its decay --
    LARS: |g'| = 0 -> q = 1 -> w -= lr * wd * w;  LAMB: u = wd * w, q = 1 / wd -> w -= lr * w"""
    factor = 1 - 0.1 * 0.25 if kind == "lars" else 1 - 0.1
    n_ex = 0
    for n, p in m.module.named_parameters():
        if excluded(n, p):
            n_ex += 1
            assert torch.equal(p.detach(), before[n]), n
        else:
            assert torch.allclose(p.detach(), before[n] * factor, rtol=1e-5, atol=1e-8), n
            assert not torch.equal(p.detach(), before[n]), n
    assert 0 < n_ex < len(before)
    q, names = opt.last_trust_ratios
    flags = opt.excluded.tolist()
    for qi, n, ex in zip(q.tolist(), names, flags):
        assert ex == excluded(n, dict(m.module.named_parameters())[n])
        want = 1.0 if (ex or kind == "lars") else 1 / 0.25
        assert qi == pytest.approx(want, rel=1e-5), n
    pad = torch.ones(m.flat.numel, dtype=torch.bool)
    for i in range(len(m.flat.params)):
        lo, hi = m.flat.param_range(i)
        pad[lo:hi] = False
    assert pad.any() and (m.flat.data[pad] == 0).all()
    for t in _state_tensors(opt):
        assert (t[pad] == 0).all()


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_exclude_default(kind):
    m, opt, before = _zero_grad_step(kind)
    _check_zero_grad_step(kind, m, opt, before, lambda n, p: p.ndim <= 1)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_exclude_custom_predicate(kind):
    pred = lambda name, p: name.startswith("conv1") or name == "fc3.bias"  # noqa: E731
    m, opt, before = _zero_grad_step(kind, exclude=pred)
    _check_zero_grad_step(kind, m, opt, before, pred)


def test_unaligned_layout_is_rejected():
    from mi355x_dp.parallel import DataParallel, FlatLAMB, FlatLARS
    for cls in (FlatLARS, FlatLAMB):
        m = DataParallel(_model(), **PLAN)
        m.flat.offsets[1] += 1
        with pytest.raises(ValueError, match="multiples of 64"):
            cls(m, lr=0.1)


# ------------------------------------------------------------------------- 3. world 2, gloo
def _worker_world2(rank, world, port, q, kind, shard, steps):
    try:
        _init(rank, world, port)
        from mi355x_dp.parallel import DataParallel
        m = DataParallel(_model(), shard_optimizer=shard, **PLAN)
        opt = _make(kind, m)
        x, y = _data()
        part = slice(rank * 8, (rank + 1) * 8)
        for _ in range(steps):
            _backward(m, x[part], y[part])
            opt.step()
        sd = {k: v.clone().numpy() for k, v in m.state_dict().items()}  # joins the parameter all-gathers
        q.put((rank, sd, opt.last_trust_ratios[0].tolist(), [t.numel() for t in _state_tensors(opt)], m.flat.numel,
               len(m.buckets)))
        dist.destroy_process_group()
    except Exception as e:  # surface worker failures instead of timing out
        q.put((rank, e, None, None, None, None))
        raise


def _spawn(target, args, world=2):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    ps = [ctx.Process(target=target, args=(r, world, port, q) + tuple(args)) for r in range(world)]
    for p in ps:
        p.start()
    res = {}
    for _ in ps:
        r, *rest = q.get(timeout=180)
        res[r] = rest
    for p in ps:
        p.join(60)
    for r, v in res.items():
        assert not isinstance(v[0], Exception), f"rank {r}: {v[0]!r}"
    return res


def _full_batch_reference(kind, dtype, steps):
    """one process, full batch (mean of the two shard losses == average of the shard gradients),
    the per-tensor reference over the model's own tensors"""
    m = _model().to(dtype)
    params = list(m.parameters())
    layout, off = [], 0
    for p in params:
        layout.append((off, off + p.numel(), p.ndim <= 1))
        off += p.numel()
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])  # noqa: E731
    ref = ref_pair(kind, cat(params), layout, **HYPER[kind])[0 if dtype == torch.float64 else 1]
    x, y = _data()
    x = x.to(dtype)
    for _ in range(steps):
        m.zero_grad()
        (0.5 * (F.cross_entropy(m(x[:8]), y[:8]) + F.cross_entropy(m(x[8:]), y[8:]))).backward()
        ref.step(cat([p.grad for p in params]))
        new = ref.flat()
        with torch.no_grad():
            for p, (lo, hi, _) in zip(params, layout):
                p.copy_(new[lo:hi].reshape(p.shape))
    return {"module." + k: v.detach() for k, v in m.state_dict().items()}


def _cat(sd, keys):
    return torch.cat([torch.as_tensor(sd[k]).reshape(-1).double() for k in keys])


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_world2_matches_full_batch_and_shards_agree(kind):
    steps = 3
    ar = _spawn(_worker_world2, (kind, False, steps))
    sh = _spawn(_worker_world2, (kind, True, steps))
    keys = sorted(ar[0][0])
    for res in (ar, sh):
        for k in keys:
            assert (res[0][0][k] == res[1][0][k]).all(), f"replicas diverged at {k}"
        assert res[0][1] == res[1][1], "ranks hold different trust ratios"
    assert ar[0][4] > 1, "expected several buckets"
    ref64, ref32 = _full_batch_reference(kind, torch.float64, steps), _full_batch_reference(kind, torch.float32, steps)
    r64, r32 = _cat(ref64, keys), _cat(ref32, keys)
    check_accuracy(_cat(ar[0][0], keys), r32, r64, f"{kind} all-reduce engine vs full batch")
    check_accuracy(_cat(sh[0][0], keys), r32, r64, f"{kind} shard engine vs full batch")
    for r in range(2):
        assert all(n * 2 == sh[r][3] for n in sh[r][2]), "state must hold 1/world of the flat buffer"
        assert all(n == ar[r][3] for n in ar[r][2])


# ---------------------------------------------------------------------------- 4. checkpoints
def _resume_run(engine, x, y, ckpt):
    from mi355x_dp.utils import load_checkpoint, save_checkpoint
    m, opt = engine()
    for _ in range(3):
        _backward(m, x, y)
        opt.step()
    save_checkpoint(ckpt, m, opt, step=3)
    for _ in range(2):
        _backward(m, x, y)
        opt.step()
    a = {k: v.clone() for k, v in m.state_dict().items()}
    m2, opt2 = engine()
    for p in m2.module.parameters():  # resume must not depend on the fresh init
        p.data.add_(1.0)
    info = load_checkpoint(ckpt, m2, opt2)
    assert opt2.steps == 3
    for _ in range(2):
        _backward(m2, x, y)
        opt2.step()
    b = m2.state_dict()
    same = all(torch.equal(a[k], b[k]) for k in a) and opt2.steps == 5 and \
        all(torch.equal(s, t) for s, t in zip(_state_tensors(opt), _state_tensors(opt2)))
    return same, info["step"]


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_checkpoint_resume_plain(kind, tmp_path):
    from mi355x_dp.parallel import DataParallel

    def engine():
        m = DataParallel(_model(), **PLAN)
        return m, _make(kind, m, **({"max_grad_norm": 0.5} if kind == "lamb" else {}))
    same, step = _resume_run(engine, *_data(), str(tmp_path / "ckpt.pt"))
    assert same and step == 3


def _worker_resume(rank, world, port, q, kind, ckpt):
    try:
        _init(rank, world, port)
        from mi355x_dp.parallel import DataParallel
        x, y = _data()
        part = slice(rank * 8, (rank + 1) * 8)

        def engine():
            m = DataParallel(_model(), shard_optimizer=True, **PLAN)
            return m, _make(kind, m)
        same, step = _resume_run(engine, x[part], y[part], ckpt)
        q.put((rank, same, step, os.path.exists(f"{ckpt}.optim-rank{rank}-of-{world}")))
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, e, None, None))
        raise


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_checkpoint_resume_shard_world2(kind, tmp_path):
    """utils/checkpoint.py keys on "shard" in the state dict: every rank writes its own state"""
    res = _spawn(_worker_resume, (kind, str(tmp_path / "ckpt.pt")))
    for r, (same, step, exists) in res.items():
        assert same is True and step == 3 and exists, (r, same, step, exists)


@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_shard_state_rejects_a_different_bucket_plan(kind):
    from mi355x_dp.parallel import DataParallel
    e1 = DataParallel(_model(), shard_optimizer=True, **PLAN)
    o1 = _make(kind, e1)
    _backward(e1, *_data())
    o1.step()
    sd = o1.state_dict()
    assert sd["steps"] == 1 and sd["shard"]["bucket_ranges"] == [list(r) for r in e1.bucket_ranges]
    same = DataParallel(_model(), shard_optimizer=True, **PLAN)
    o_same = _make(kind, same)
    o_same.load_state_dict(sd)
    assert all(torch.equal(s, t) for s, t in zip(_state_tensors(o_same), _state_tensors(o1))) and o_same.steps == 1
    other = DataParallel(_model(), shard_optimizer=True, bucket_cap_mb=0.2, first_bucket_mb=0.05, min_bucket_mb=0)
    assert len(other.buckets) != len(e1.buckets)
    with pytest.raises(ValueError, match="bucket plan"):
        _make(kind, other).load_state_dict(sd)


# ------------------------------------------------------------------------------ 5. lr change
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_lr_change_takes_effect_on_the_next_step(kind):
    from mi355x_dp.parallel import DataParallel
    m = DataParallel(_model(), **PLAN)
    opt = _make(kind, m)
    ref64, ref32 = ref_pair(kind, m.flat.data, layout_of(opt), **HYPER[kind])
    frozen64, _ = ref_pair(kind, m.flat.data, layout_of(opt), **HYPER[kind])  # never told about the change
    lr0 = HYPER[kind]["lr"]
    x, y = _data()
    for step, lr in enumerate([lr0, lr0, 0.3 * lr0, 0.3 * lr0]):
        opt.param_groups[0]["lr"] = lr
        ref64.set_lr(lr)
        ref32.set_lr(lr)
        _backward(m, x, y)
        g = m.flat.grad.clone()
        opt.step()
        ref64.step(g), ref32.step(g), frozen64.step(g)
        check_accuracy(m.flat.data, ref32.flat(), ref64.flat(), f"{kind} step {step} lr {lr}")
    apart = float((ref64.flat() - frozen64.flat()).abs().max())
    assert float((m.flat.data.double() - frozen64.flat()).abs().max()) > 0.5 * apart > 1e-4
