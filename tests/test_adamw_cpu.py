"""FlatAdamW on the host fallback (same math as the HIP kernels), single process and gloo world 2:
accuracy against an fp64 reference with stock fp32 AdamW as the yardstick (adamw_reference.py),
the per-unit decay map, replica identity with and without balanced shards, checkpoints, and a
learning-rate change between steps."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from adamw_reference import check_accuracy, decay_mask_of, ref_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)
HYPER = dict(lr=1e-2, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _init(rank, world, port):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    sys.path.insert(0, ROOT)
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


def _first_norm():
    """gradient norm of the first step (what sizes max_grad_norm in the clipping cases)"""
    from mi355x_dp.parallel import DataParallel
    m = DataParallel(_model(), **PLAN)
    _backward(m, *_data())
    return float(m.flat.grad.double().norm())


# ------------------------------------------------------------------ 1. single process vs fp64
@pytest.mark.parametrize("clip", [False, True])
def test_single_process_matches_fp64(clip):
    """five steps; the references get the gradients the engine produced, so the comparison is of
    the optimizer alone"""
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    max_norm = 0.1 * _first_norm() if clip else None
    m = DataParallel(_model(), **PLAN)
    opt = FlatAdamW(m, max_grad_norm=max_norm, **HYPER)
    assert len(opt.segments) == 1 and opt.exp_avg.numel() == m.flat.numel
    ref64, ref32 = ref_pair(m.flat.data, decay_mask_of(opt), max_norm=max_norm, **HYPER)
    x, y = _data()
    for step in range(5):
        _backward(m, x, y)
        g = m.flat.grad.clone()
        opt.step()
        n64 = ref64.step(g)
        n32 = ref32.step(g)
        if clip:
            assert float(opt.last_grad_norm) > max_norm, "clipping is not active"
            assert float(opt.last_grad_norm) == pytest.approx(float(n64), rel=1e-6)
            assert abs(float(opt.last_grad_norm) - float(n64)) <= 2 * abs(float(n32) - float(n64)) + 1e-7 * float(n64)
        else:
            assert opt.last_grad_norm is None
        check_accuracy(m.flat.data, ref32.flat(), ref64.flat(), f"step {step}")
    assert opt.steps == 5


# ------------------------------------------------------------------------------ 2. decay map
def _zero_grad_step(no_decay=None):
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    m = DataParallel(_model(), **PLAN)
    opt = FlatAdamW(m, lr=0.1, weight_decay=0.25, eps=1e-8, no_decay=no_decay)
    before = {n: p.detach().clone() for n, p in m.module.named_parameters()}
    m.zero_grad()
    opt.step()
    return m, opt, before


def _padding_mask(flat):
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for i in range(len(flat.params)):
        lo, hi = flat.param_range(i)
        pad[lo:hi] = False
    return pad


def test_decay_map_default():
    m, opt, before = _zero_grad_step()
    factor = 1 - 0.1 * 0.25
    seen = set()
    for n, p in m.module.named_parameters():
        seen.add(p.ndim > 1)
        want = before[n] * factor if p.ndim > 1 else before[n]
        assert torch.equal(p.detach(), want), n
    assert seen == {True, False}
    pad = _padding_mask(m.flat)
    assert pad.any()
    for buf in (m.flat.data, opt.exp_avg, opt.exp_avg_sq):
        assert (buf[pad] == 0).all()
    assert (opt.exp_avg == 0).all() and (opt.exp_avg_sq == 0).all()


def test_decay_map_custom_predicate():
    m, opt, before = _zero_grad_step(no_decay=lambda name, p: name.startswith("conv1") or name == "fc3.bias")
    factor = 1 - 0.1 * 0.25
    kept = 0
    for n, p in m.module.named_parameters():
        keep = n.startswith("conv1") or n == "fc3.bias"
        kept += keep
        assert torch.equal(p.detach(), before[n] if keep else before[n] * factor), n
    assert 0 < kept < len(before)
    assert (m.flat.data[_padding_mask(m.flat)] == 0).all()


# ------------------------------------------------------------------------- 3. world 2, gloo
def _worker_world2(rank, world, port, q, shard, max_norm, steps):
    try:
        _init(rank, world, port)
        from mi355x_dp.parallel import DataParallel, FlatAdamW
        m = DataParallel(_model(), shard_optimizer=shard, **PLAN)
        opt = FlatAdamW(m, max_grad_norm=max_norm, **HYPER)
        x, y = _data()
        part = slice(rank * 8, (rank + 1) * 8)
        norms = []
        for _ in range(steps):
            _backward(m, x[part], y[part])
            opt.step()
            norms.append(float(opt.last_grad_norm))
        sd = {k: v.clone().numpy() for k, v in m.state_dict().items()}  # joins the parameter all-gathers
        q.put((rank, sd, norms, opt.exp_avg.numel(), opt.exp_avg_sq.numel(), m.flat.numel, len(m.buckets)))
        dist.destroy_process_group()
    except Exception as e:  # surface worker failures instead of timing out
        q.put((rank, e, None, None, None, None, None))
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


def _full_batch_reference(dtype, max_norm, steps):
    """one process, full batch (mean of the two shard losses == average of the shard gradients),
    torch.optim.AdamW with decay / no-decay groups and clip_grad_norm_"""
    m = _model().to(dtype)
    decay = [p for p in m.parameters() if p.ndim > 1]
    rest = [p for p in m.parameters() if p.ndim <= 1]
    hyper = {k: v for k, v in HYPER.items() if k != "weight_decay"}
    opt = torch.optim.AdamW([dict(params=decay, weight_decay=HYPER["weight_decay"]),
                             dict(params=rest, weight_decay=0.0)], **hyper)
    x, y = _data()
    x = x.to(dtype)
    for _ in range(steps):
        opt.zero_grad()
        (0.5 * (F.cross_entropy(m(x[:8]), y[:8]) + F.cross_entropy(m(x[8:]), y[8:]))).backward()
        torch.nn.utils.clip_grad_norm_(list(m.parameters()), max_norm)
        opt.step()
    return {"module." + k: v.detach() for k, v in m.state_dict().items()}


def _cat(sd, keys):
    return torch.cat([torch.as_tensor(sd[k]).reshape(-1).double() for k in keys])


def test_world2_matches_full_batch_and_shards_agree():
    steps = 3
    max_norm = 0.1 * _first_norm()
    ar = _spawn(_worker_world2, (False, max_norm, steps))
    sh = _spawn(_worker_world2, (True, max_norm, steps))
    keys = sorted(ar[0][0])
    for res in (ar, sh):
        for k in keys:
            assert (res[0][0][k] == res[1][0][k]).all(), f"replicas diverged at {k}"
        assert res[0][1] == res[1][1], "ranks saw different gradient norms"
        assert all(n > max_norm for n in res[0][1]), "clipping is not active"
    assert ar[0][5] > 1, "expected several buckets"
    ref64, ref32 = _full_batch_reference(torch.float64, max_norm, steps), \
        _full_batch_reference(torch.float32, max_norm, steps)
    r64, r32 = _cat(ref64, keys), _cat(ref32, keys)
    check_accuracy(_cat(ar[0][0], keys), r32, r64, "all-reduce engine vs full batch")
    _, e_stock = check_accuracy(_cat(sh[0][0], keys), r32, r64, "shard engine vs full batch")
    # shard vs all-reduce engine: the same rule, with the all-reduce engine in the reference's place
    check_accuracy(_cat(sh[0][0], keys), _cat(ar[0][0], keys) + (r32 - r64), _cat(ar[0][0], keys),
                   "shard engine vs all-reduce engine")
    for r in range(2):
        assert sh[r][2] * 2 == sh[r][3] * 2 == sh[r][4], "moments must hold 1/world of the flat buffer"
        assert ar[r][2] == ar[r][3] == ar[r][4]


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
    same = all(torch.equal(a[k], b[k]) for k in a) and torch.equal(opt.exp_avg, opt2.exp_avg) and \
        torch.equal(opt.exp_avg_sq, opt2.exp_avg_sq) and opt2.steps == 5
    return same, info["step"]


def test_checkpoint_resume_plain(tmp_path):
    from mi355x_dp.parallel import DataParallel, FlatAdamW

    def engine():
        m = DataParallel(_model(), **PLAN)
        return m, FlatAdamW(m, max_grad_norm=0.5, **HYPER)
    same, step = _resume_run(engine, *_data(), str(tmp_path / "ckpt.pt"))
    assert same and step == 3


def _worker_resume(rank, world, port, q, ckpt):
    try:
        _init(rank, world, port)
        from mi355x_dp.parallel import DataParallel, FlatAdamW
        x, y = _data()
        part = slice(rank * 8, (rank + 1) * 8)

        def engine():
            m = DataParallel(_model(), shard_optimizer=True, **PLAN)
            return m, FlatAdamW(m, max_grad_norm=0.5, **HYPER)
        same, step = _resume_run(engine, x[part], y[part], ckpt)
        q.put((rank, same, step, os.path.exists(f"{ckpt}.optim-rank{rank}-of-{world}")))
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, e, None, None))
        raise


def test_checkpoint_resume_shard_world2(tmp_path):
    """utils/checkpoint.py keys on "shard" in the state dict: every rank writes its own moments"""
    res = _spawn(_worker_resume, (str(tmp_path / "ckpt.pt"),))
    for r, (same, step, exists) in res.items():
        assert same is True and step == 3 and exists, (r, same, step, exists)


def test_shard_state_rejects_a_different_bucket_plan():
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    e1 = DataParallel(_model(), shard_optimizer=True, **PLAN)
    o1 = FlatAdamW(e1, **HYPER)
    _backward(e1, *_data())
    o1.step()
    sd = o1.state_dict()
    assert sd["steps"] == 1 and sd["shard"]["bucket_ranges"] == [list(r) for r in e1.bucket_ranges]
    same = DataParallel(_model(), shard_optimizer=True, **PLAN)
    o_same = FlatAdamW(same, **HYPER)
    o_same.load_state_dict(sd)
    assert torch.equal(o_same.exp_avg, o1.exp_avg) and torch.equal(o_same.exp_avg_sq, o1.exp_avg_sq)
    assert o_same.steps == 1
    other = DataParallel(_model(), shard_optimizer=True, bucket_cap_mb=0.2, first_bucket_mb=0.05, min_bucket_mb=0)
    assert len(other.buckets) != len(e1.buckets)
    with pytest.raises(ValueError, match="bucket plan"):
        FlatAdamW(other, **HYPER).load_state_dict(sd)


# ------------------------------------------------------------------------------ 5. lr change
def test_lr_change_takes_effect_on_the_next_step():
    from mi355x_dp.parallel import DataParallel, FlatAdamW
    m = DataParallel(_model(), **PLAN)
    opt = FlatAdamW(m, **HYPER)
    ref64, ref32 = ref_pair(m.flat.data, decay_mask_of(opt), **HYPER)
    frozen64, _ = ref_pair(m.flat.data, decay_mask_of(opt), **HYPER)  # never told about the change
    x, y = _data()
    for step, lr in enumerate([HYPER["lr"], HYPER["lr"], 3e-3, 3e-3]):
        opt.param_groups[0]["lr"] = lr
        ref64.set_lr(lr)
        ref32.set_lr(lr)
        _backward(m, x, y)
        g = m.flat.grad.clone()
        opt.step()
        ref64.step(g), ref32.step(g), frozen64.step(g)
        check_accuracy(m.flat.data, ref32.flat(), ref64.flat(), f"step {step} lr {lr}")
    apart = float((ref64.flat() - frozen64.flat()).abs().max())
    assert float((m.flat.data.double() - frozen64.flat()).abs().max()) > 0.5 * apart > 1e-4
