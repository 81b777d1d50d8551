"""FlatEMA on the host fallback (same math as the HIP kernels, product and sum rounded separately),
single process and gloo world 2: the averaged weights against the fp64 recursion of
ema_reference.py, evaluation by in-place exchange (``applied()``), live against averaged
BatchNorm statistics, replica identity with and without balanced shards, checkpoints, a decay
change between updates and argument validation."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from ema_reference import RefEMA, check_rule, check_scalars

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN = dict(bucket_cap_mb=0.05, first_bucket_mb=0.01, min_bucket_mb=0)


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


class BNNet(torch.nn.Module):
    """conv + BatchNorm + linear: float buffers of odd total length (2 x 12 + the integer counter)"""

    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 12, 3, padding=1)
        self.bn = torch.nn.BatchNorm2d(12)
        self.fc = torch.nn.Linear(12, 10)

    def forward(self, x):
        return self.fc(F.relu(self.bn(self.conv(x))).mean((2, 3)))


def _model(bn=False):
    from mi355x_dp.models import Net
    torch.manual_seed(0)
    return BNNet() if bn else Net()


def _data():
    g = torch.Generator().manual_seed(1)
    return torch.randn(16, 3, 32, 32, generator=g), torch.randint(0, 10, (16,), generator=g)


def _engine(bn=False, **kw):
    from mi355x_dp.parallel import DataParallel, FlatSGD
    m = DataParallel(_model(bn), **PLAN, **kw)
    return m, FlatSGD(m, lr=0.05, momentum=0.9)


def _step(m, opt, x, y):
    m.train()
    m.zero_grad()
    F.cross_entropy(m(x), y).backward()
    opt.step()


def _bits(t):
    return t.detach().clone().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


# ------------------------------------------------------------------ 1. single process vs fp64
def test_single_process_matches_fp64():
    from mi355x_dp.parallel import FlatEMA
    m, opt = _engine()
    ema = FlatEMA(m, decay=0.99, warmup=10, update_every=2)
    assert len(ema.segments) == 1 and ema.avg.numel() == m.flat.numel and torch.equal(ema.avg, m.flat.data)
    assert ema.num_updates == 0 and ema.num_calls == 0
    ref = RefEMA([m.flat.data], 0.99, warmup=10, every=2)
    x, y = _data()
    for step in range(12):
        _step(m, opt, x, y)
        before = ema.avg.clone()
        ema.update()
        ref.update([m.flat.data])
        check_scalars(ema.state, ref, f"step {step}")
        check_rule(ema.avg, ref, f"step {step}")
        assert (step % 2 == 0) == torch.equal(before, ema.avg), "odd calls skip, even calls update"
    assert ema.num_calls == 12 and ema.num_updates == 6
    assert float((ema.avg - m.flat.data).abs().max()) > 1e-4, "the average must lag the weights"


# ------------------------------------------------------------------------------ 2. applied()
@pytest.mark.parametrize("bn", [False, True])
def test_applied_exchanges_and_restores(bn):
    from mi355x_dp.parallel import FlatEMA
    m, opt = _engine(bn)
    ema = FlatEMA(m, decay=0.9, buffers="average" if bn else "live")
    x, y = _data()
    for _ in range(3):
        _step(m, opt, x, y)
        ema.update()
    m.eval()
    snap = [_bits(m.flat.data), _bits(m.buffers.data)] + ([_bits(m.flat.bf16)] if m.flat.bf16 is not None else [])
    avg_before = _bits(ema.avg)
    live_out = m(x).detach().clone()
    want = ema.module_state_dict()
    assert torch.equal(_bits(m.flat.data), snap[0]), "module_state_dict() must restore"

    def current():
        return [_bits(m.flat.data), _bits(m.buffers.data)] + ([_bits(m.flat.bf16)] if m.flat.bf16 is not None else [])

    with ema.applied():
        got = m.module.state_dict()
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k
        assert torch.equal(_bits(m.flat.data), avg_before)
        if m.flat.bf16 is not None:
            assert torch.equal(m.flat.bf16, m.flat.data.to(torch.bfloat16))
        stock = _model(bn)
        stock.load_state_dict(want)
        stock.eval()
        out = m(x).detach()
        assert torch.equal(out, stock(x).detach())
        assert not torch.equal(out, live_out)
        with pytest.raises(RuntimeError, match="already active"):
            with ema.applied():
                pass
        with pytest.raises(RuntimeError, match="inside applied"):
            ema.update()
    for a, b in zip(current(), snap):
        assert torch.equal(a, b)
    assert torch.equal(_bits(ema.avg), avg_before)
    assert torch.equal(m(x).detach(), live_out)

    with pytest.raises(KeyError):
        with ema.applied():
            raise KeyError("body")
    for a, b in zip(current(), snap):
        assert torch.equal(a, b)
    assert torch.equal(_bits(ema.avg), avg_before)
    ema.update()  # usable again after the block


# ------------------------------------------------------------------- 3. live vs averaged buffers
@pytest.mark.parametrize("mode", ["live", "average"])
def test_buffers_live_and_average(mode):
    from mi355x_dp.parallel import FlatEMA
    m, opt = _engine(bn=True)
    plain, plain_opt = _engine(bn=True)  # the same run without an EMA: what the live statistics must be
    ema = FlatEMA(m, decay=0.9, warmup=2, buffers=mode)
    n_buf = sum(b.numel() for b in m.buffers.buffers)
    assert n_buf == 24 and (ema.avg_buffers is not None) == (mode == "average")
    ref = RefEMA([m.flat.data, m.buffers.data[:n_buf]], 0.9, warmup=2)
    x, y = _data()
    for step in range(4):
        _step(m, opt, x, y)
        _step(plain, plain_opt, x, y)
        ema.update()
        ref.update([m.flat.data, m.buffers.data[:n_buf]])
        assert torch.equal(m.buffers.data, plain.buffers.data), "live statistics changed"
        assert int(m.module.bn.num_batches_tracked) == step + 1
    check_rule(ema.avg, ref, "weights")
    tracked = m.module.bn.num_batches_tracked.clone()
    live_mean = m.module.bn.running_mean.clone()
    sd = ema.module_state_dict()
    assert torch.equal(sd["bn.num_batches_tracked"], tracked) and torch.equal(m.module.bn.num_batches_tracked, tracked)
    if mode == "average":
        assert ema.avg_buffers.numel() == n_buf
        check_rule(ema.avg_buffers, ref, "statistics", index=1)
        assert torch.equal(sd["bn.running_mean"], ema.avg_buffers[:12])
        assert not torch.equal(sd["bn.running_mean"], live_mean)
    else:
        assert torch.equal(sd["bn.running_mean"], live_mean)
    assert torch.equal(m.module.bn.running_mean, live_mean)


# ------------------------------------------------------------------------- 4. world 2, gloo
def _worker_world2(rank, world, port, q, shard, steps):
    try:
        _init(rank, world, port)
        from mi355x_dp.parallel import FlatEMA
        m, opt = _engine(shard_optimizer=shard)
        ema = FlatEMA(m, decay=0.9, warmup=3)
        x, y = _data()
        part = slice(rank * 8, (rank + 1) * 8)
        for _ in range(steps):
            _step(m, opt, x[part], y[part])
            ema.update()
        live = {k: v.clone().numpy() for k, v in m.state_dict().items()}  # joins the parameter all-gathers
        bf16 = m.flat.bf16.clone() if m.flat.bf16 is not None else None
        avg = {k: v.numpy() for k, v in ema.module_state_dict().items()}
        after = {k: v.clone().numpy() for k, v in m.state_dict().items()}
        restored = all((live[k] == after[k]).all() for k in live) and \
            (bf16 is None or torch.equal(bf16, m.flat.bf16))
        with ema.applied():
            inside = {k: v.clone().numpy() for k, v in m.module.state_dict().items()}
        applied_ok = all((inside[k] == avg[k]).all() for k in avg)
        q.put((rank, avg, restored and applied_ok, ema.avg.numel(), m.flat.numel, len(m.buckets), ema.num_updates))
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


def test_world2_replicas_identical_and_shards_packed():
    steps = 4
    ar = _spawn(_worker_world2, (False, steps))
    sh = _spawn(_worker_world2, (True, steps))
    keys = sorted(ar[0][0])
    for res in (ar, sh):
        for k in keys:
            assert (res[0][0][k] == res[1][0][k]).all(), f"replicas' averaged weights diverged at {k}"
        for r in range(2):
            assert res[r][1] is True, f"rank {r}: applied() did not restore / publish"
            assert res[r][5] == steps
    for k in keys:
        assert (ar[0][0][k] == sh[0][0][k]).all(), f"shard engine's average differs from the unsharded one at {k}"
    assert sh[0][4] > 1, "expected several buckets"
    for r in range(2):
        assert sh[r][2] * 2 == sh[r][3], "shard mode: avg must hold 1/world of the flat buffer"
        assert ar[r][2] == ar[r][3]


# ---------------------------------------------------------------------------- 5. checkpoints
def _resume_run(engine, x, y, ckpt):
    from mi355x_dp.utils import load_checkpoint, save_checkpoint
    m, opt, ema = engine()
    for _ in range(3):
        _step(m, opt, x, y)
        ema.update()
    save_checkpoint(ckpt, m, opt, step=3, ema=ema)
    for _ in range(3):
        _step(m, opt, x, y)
        ema.update()
    m2, opt2, ema2 = engine()
    for p in m2.module.parameters():  # resume must not depend on the fresh init
        p.data.add_(1.0)
    ema2.avg.add_(1.0)
    ema2.decay = 0.5
    info = load_checkpoint(ckpt, m2, opt2, ema=ema2)
    assert ema2.num_calls == 3 and ema2.num_updates == 1 and ema2.decay == ema.decay
    for _ in range(3):
        _step(m2, opt2, x, y)
        ema2.update()
    m.wait_param_sync(), m2.wait_param_sync()  # shard mode: join the parameter all-gathers
    same =torch.equal(_bits(ema.avg), _bits(ema2.avg)) and torch.equal(ema.state, ema2.state) and \
        torch.equal(m.flat.data, m2.flat.data) and (ema2.num_calls, ema2.num_updates) == (6, 3)
    if ema.avg_buffers is not None:
        same = same and torch.equal(_bits(ema.avg_buffers), _bits(ema2.avg_buffers))
    return same, info["step"]


def test_checkpoint_resume_plain(tmp_path):
    from mi355x_dp.parallel import FlatEMA
    from mi355x_dp.utils import load_checkpoint, save_checkpoint

    def engine():
        m, opt = _engine(bn=True)
        return m, opt, FlatEMA(m, decay=0.95, warmup=2, update_every=2, buffers="average")
    ckpt = str(tmp_path / "ckpt.pt")
    same, step = _resume_run(engine, *_data(), ckpt)
    assert same and step == 3
    state = torch.load(ckpt, weights_only=True)
    assert set(state["ema"]) >= {"avg", "avg_buffers", "calls", "updates", "decay", "warmup", "update_every", "buffers"}

    # a call without ema= behaves as before: no "ema" entry, and such a file loads without one
    m, opt, ema = engine()
    plain = str(tmp_path / "plain.pt")
    save_checkpoint(plain, m, opt, step=1)
    assert "ema" not in torch.load(plain, weights_only=True)
    assert load_checkpoint(plain, m, opt)["step"] == 1
    assert load_checkpoint(ckpt, m, opt)["step"] == 3  # an EMA checkpoint loads without ema= too
    with pytest.raises(ValueError, match="no averaged weights"):
        load_checkpoint(plain, m, opt, ema=ema)


def _worker_resume(rank, world, port, q, ckpt):
    try:
        _init(rank, world, port)
        from mi355x_dp.parallel import FlatEMA
        x, y = _data()
        part = slice(rank * 8, (rank + 1) * 8)

        def engine():
            m, opt = _engine(shard_optimizer=True)
            return m, opt, FlatEMA(m, decay=0.95, warmup=2, update_every=2)
        same, step = _resume_run(engine, x[part], y[part], ckpt)
        q.put((rank, same, step, os.path.exists(f"{ckpt}.ema-rank{rank}-of-{world}")))
        dist.destroy_process_group()
    except Exception as e:
        q.put((rank, e, None, None))
        raise


def test_checkpoint_resume_shard_world2(tmp_path):
    ckpt = str(tmp_path / "ckpt.pt")
    res = _spawn(_worker_resume, (ckpt,))
    for r, (same, step, exists) in res.items():
        assert same is True and step == 3 and exists, (r, same, step, exists)
    assert torch.load(ckpt, weights_only=True)["ema"] == {"sharded_over": 2}


def test_shard_state_rejects_a_different_bucket_plan():
    from mi355x_dp.parallel import DataParallel, FlatEMA
    e1 = DataParallel(_model(), shard_optimizer=True, **PLAN)
    a = FlatEMA(e1, decay=0.9)
    a.update()
    sd = a.state_dict()
    assert sd["updates"] == 1 and sd["shard"]["bucket_ranges"] == [list(r) for r in e1.bucket_ranges]
    b = FlatEMA(DataParallel(_model(), shard_optimizer=True, **PLAN), decay=0.5)
    b.load_state_dict(sd)
    assert torch.equal(a.avg, b.avg) and b.num_updates == 1 and b.decay == 0.9 and float(b.state[3]) == 0.9
    other = DataParallel(_model(), shard_optimizer=True, bucket_cap_mb=0.2, first_bucket_mb=0.05, min_bucket_mb=0)
    assert len(other.buckets) != len(e1.buckets)
    with pytest.raises(ValueError, match="bucket plan"):
        FlatEMA(other, decay=0.9).load_state_dict(sd)


# --------------------------------------------------------------- 6. decay change, validation
def test_decay_change_takes_effect_on_the_next_update():
    from mi355x_dp.parallel import FlatEMA
    m, opt = _engine()
    ema = FlatEMA(m, decay=0.9)
    ref = RefEMA([m.flat.data], 0.9)
    frozen = RefEMA([m.flat.data], 0.9)  # never told about the change
    x, y = _data()
    for step, decay in enumerate([0.9, 0.9, 0.5, 0.5]):
        ema.decay = ref.decay = decay
        _step(m, opt, x, y)
        ema.update()
        ref.update([m.flat.data]), frozen.update([m.flat.data])
        check_scalars(ema.state, ref, f"step {step}")
        check_rule(ema.avg, ref, f"step {step} decay {decay}")
    apart = float((ref.ema[0] - frozen.ema[0]).abs().max())
    assert float((ema.avg.double() - frozen.ema[0]).abs().max()) > 0.5 * apart > 1e-5


@pytest.mark.parametrize("kw", [dict(decay=1.0), dict(decay=-0.1), dict(decay=float("nan")), dict(warmup=0),
                                dict(warmup=0.5), dict(update_every=0), dict(update_every=2.0),
                                dict(update_every=True), dict(buffers="both")])
def test_argument_validation(kw):
    from mi355x_dp.parallel import FlatEMA
    m, _ = _engine()
    with pytest.raises(ValueError, match="FlatEMA"):
        FlatEMA(m, **kw)


def test_host_ops_without_the_library():
    """the three flat ops on host tensors: any length, unaligned slices, exact exchange"""
    from mi355x_dp.ops import ema_prep_, ema_swap_, ema_update_
    from mi355x_dp.ops.functional import EMA_STATE_LEN
    assert EMA_STATE_LEN == 5
    state = torch.zeros(5, dtype=torch.float64)
    state[3] = 0.75
    g = torch.Generator().manual_seed(2)
    whole_e, whole_p = torch.randn(40, generator=g), torch.randn(40, generator=g)
    e, p = whole_e[3:30], whole_p[1:28]
    e0, guard = e.clone(), whole_e.clone()
    ema_prep_(state, None, 2)
    assert state.tolist() == [1.0, 0.0, 0.0, 0.75, 0.0]
    ema_update_(e, p, state)
    assert torch.equal(e, e0), "a skipped call must leave the average alone"
    ema_prep_(state, None, 2)
    assert state.tolist() == [2.0, 1.0, 0.25, 0.75, 0.75]
    ema_update_(e, p, state)
    assert torch.allclose(e, e0 + 0.25 * (p - e0), rtol=0, atol=1e-6) and not torch.equal(e, e0)
    assert torch.equal(whole_e[:3], guard[:3]) and torch.equal(whole_e[30:], guard[30:])
    ema_update_(e[:0], p[:0], state)  # n == 0
    a = torch.tensor([float("nan"), -0.0, 1e-42, float("inf"), 1.0])
    a.view(torch.int32)[0] = 0x7FC12345  # a NaN payload
    b = torch.arange(5, dtype=torch.float32)
    a0, b0 = _bits(a), _bits(b)
    ema_swap_(a, b)
    assert torch.equal(_bits(a), b0) and torch.equal(_bits(b), a0)
    ema_swap_(a, b)
    assert torch.equal(_bits(a), a0) and torch.equal(_bits(b), b0)
