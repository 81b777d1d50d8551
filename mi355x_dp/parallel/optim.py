"""``FlatAdamW``: torch.optim.AdamW semantics over the engine's flat buffers, with global-norm
gradient clipping computed on the device -- the way a ViT is normally trained (AdamW, no weight
decay on biases / norms / tokens, ``clip_grad_norm_``) without leaving the flat-buffer design.

One step is: squared-norm pass (only when clipping) -> in shard mode a one-element all-reduce ->
a one-thread prep kernel -> one fused update launch per segment (csrc/kernels/optim.hip).
Everything that changes per step -- the step count, ``lr``, the bias corrections, the clip
coefficient -- lives in a small device state block that the prep kernel advances, so a captured
step (``GraphedStep``, the graphed engine) replays with the right corrections; nothing in
``step()`` reads the device.

``FlatLARS`` and ``FlatLAMB``: the layer-wise optimizers of large-batch training on the same flat
buffers.  Every parameter gets its own trust ratio ``q`` from L2 norms taken per parameter over the
flat buffer (segmented norms: one fp64 partial per 64-element unit, then one block per parameter
sums its units in a fixed order -- deterministic, device-resident, independent of how the owned
range is cut into launches).  torch ships neither optimizer, so these formulas are the
specification.  Norms are the fp64 square roots of fp64 sums of squares;
``g' = grad_scale * clip * g`` (``clip`` = 1 for LARS); ``exclude(name, param)`` (default
``ndim <= 1``) picks the parameters without decay and without adaptation; the ``> 0`` tests are
plain comparisons, so a NaN norm gives ``q = 1`` and the NaN reaches the weights through the
update itself.

LARS (``lr``, ``momentum=0.9``, ``weight_decay``, ``trust_coefficient=1e-3``, ``eps=1e-8``)::

    adapted:   q = trust_coefficient * |w| / (|g'| + wd * |w| + eps)  if |w| > 0 and |g'| > 0 else 1
               d = q * (g' + wd * w)
    excluded:  d = g'
    buf = momentum * buf + d          (buf starts at zero: no first-step special case)
    w  -= lr * buf

LAMB (``lr``, ``betas``, ``eps=1e-6``, ``weight_decay``, ``max_grad_norm=None``)::

    t += 1
    m = beta1 * m + (1 - beta1) * g'
    v = beta2 * v + (1 - beta2) * g'^2
    r = (m / bc1) / (sqrt(v / bc2) + eps)          bc = 1 - beta^t
    adapted:   u = r + wd * w,  q = |w| / |u|  if |w| > 0 and |u| > 0 else 1
    excluded:  u = r,           q = 1
    w -= lr * q * u

One step is: finish the gradient sync -> unit partials over this rank's segments (LARS: a norm
pass over w and g; LAMB: fused into the moments launch, where u exists only in registers) -> one
block per parameter reduces them -> in shard mode ONE all-reduce of the ``[2 P]`` fp64 vector, so
every rank holds the same ``q`` -> the trust kernel -> one update launch per segment (LAMB: the
apply launch recomputes u from the stored m, v and the still unchanged w) -> the same tail as
``FlatAdamW.step``.  With ``max_grad_norm`` LAMB first takes the global norm like ``FlatAdamW``
(in shard mode one more one-element all-reduce: the moments need the coefficient).
"""
from __future__ import annotations

from typing import Callable, Optional

import torch
import torch.distributed as dist

from .ddp import DataParallel, _FlatOptimizer

UNIT = 64  # elements per decay-map byte (= the flat buffer's parameter alignment)


def default_no_decay(name: str, param: torch.Tensor) -> bool:
    """biases, BatchNorm / LayerNorm weights: every parameter with at most one dimension"""
    return param.ndim <= 1


class FlatAdamW(_FlatOptimizer):
    """AdamW (no amsgrad, no maximize) over the flat buffer: one fused launch per segment with
    weight decay chosen per parameter, 1/world scaling, clipping and the bf16 copy refresh.

    ``no_decay(name, param) -> bool`` picks the parameters without weight decay (default:
    ``ndim <= 1``).  ``max_grad_norm`` clips the global gradient norm like
    ``torch.nn.utils.clip_grad_norm_``; the norm it would have returned is ``last_grad_norm`` (a
    one-element device tensor; ``float('inf')`` measures without clipping, None skips the pass).

    ``param_groups[0]["lr"]`` may be changed between steps: ``step()`` uploads it -- except while
    the stream is capturing, where a baked fill would reset it on every replay; before a replay
    push a new value with ``sync_hyper()``."""

    def __init__(self, engine: DataParallel, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None,
                 no_decay: Optional[Callable[[str, torch.Tensor], bool]] = None):
        from mi355x_dp.ops.functional import ADAMW_STATE_LEN, grad_sqnorm_slots
        f = engine.flat
        dev = f.data.device
        if f.numel % UNIT or any(o % UNIT for o in f.offsets):
            raise ValueError("FlatAdamW: flat offsets must be multiples of 64 elements")
        packed = self._init_segments(engine)
        if any(lo % UNIT for lo, _hi, _off in self.segments):
            raise ValueError("FlatAdamW: shard boundaries must be multiples of 64 elements")
        self.exp_avg = torch.zeros(packed, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(packed, dtype=torch.float32, device=dev)
        self.max_grad_norm = max_grad_norm
        self.param_groups = [dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps,
                                  weight_decay=weight_decay)]
        # one byte per 64-element unit: 1 = decays.  A unit never straddles two parameters;
        # alignment padding (zero in p, g, m, v) stays zero either way
        names = {id(p): n for n, p in engine.module.named_parameters()}
        pred = no_decay if no_decay is not None else default_no_decay
        dmap = torch.zeros(f.numel // UNIT, dtype=torch.uint8)
        for p, o in zip(f.params, f.offsets):
            if not pred(names.get(id(p), ""), p):
                dmap[o // UNIT:(o + p.numel() + UNIT - 1) // UNIT] = 1
        self.decay_map = dmap.to(dev)
        state = [0.0] * ADAMW_STATE_LEN
        state[1] = float(lr)
        self.state = torch.tensor(state, dtype=torch.float64, device=dev)
        self._lr_uploaded = float(lr)
        self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        n_slots = grad_sqnorm_slots(hi - lo for lo, hi, _ in self.segments) if dev.type == "cuda" else 0
        self._partials = torch.zeros(max(n_slots, 1), dtype=torch.float64, device=dev)

    # ------------------------------------------------------------------ device-resident scalars
    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """total gradient norm of the last step (what ``clip_grad_norm_`` returns), on the device"""
        return self.state[2:3] if self.max_grad_norm is not None else None

    @property
    def steps(self) -> int:
        """the device step counter (a host read: not for use inside a step)"""
        return int(self.state[0].item())

    def sync_hyper(self):
        """Upload ``param_groups[0]["lr"]`` to the device state block (one fill, no host sync).
        Call it before replaying a captured step after changing ``lr``."""
        lr = float(self.param_groups[0]["lr"])
        self.state[1:2].fill_(lr)
        self._lr_uploaded = lr

    def _capturing(self) -> bool:
        return self.state.is_cuda and torch.cuda.is_current_stream_capturing()

    # ---------------------------------------------------------------------------------- step
    def step(self):
        from mi355x_dp.ops.functional import adamw_flat_, adamw_prep_, grad_sqnorm_
        e = self.engine
        e.finish_gradient_sync(average=False)
        g = self.param_groups[0]
        f = e.flat
        if float(g["lr"]) != self._lr_uploaded and not self._capturing():
            self.sync_hyper()
        clip = self.max_grad_norm is not None
        if clip:
            grad_sqnorm_([f.grad[lo:hi] for lo, hi, _ in self.segments], self._sumsq, self._partials)
            if e.sharded and e.comm_on:
                # every rank then holds the same norm, hence the same coefficient: replicas stay identical
                dist.all_reduce(self._sumsq, op=dist.ReduceOp.SUM, group=e.process_group)
        b1, b2 = g["betas"]
        adamw_prep_(self.state, self._sumsq, b1, b2, g["weight_decay"], self.max_grad_norm if clip else None,
                    e.grad_scale)
        for lo, hi, so in self.segments:
            adamw_flat_(f.data[lo:hi], f.grad[lo:hi], self.exp_avg[so:so + hi - lo],
                        self.exp_avg_sq[so:so + hi - lo], f.bf16[lo:hi] if f.bf16 is not None else None, self.state,
                        b1, b2, g["eps"], self.decay_map, lo // UNIT)
        if e.sharded and e.comm_on:
            e.gather_params()  # bf16 copy + transposed operands refreshed after the gather
        else:
            f.refresh_transposed()  # dgrad operands of every conv, one launch

    # --------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        """In shard mode the moments are this rank's packed shards (a per-rank optimizer
        checkpoint, tagged with ``shard``)."""
        sd = {"steps": self.steps, "param_groups": self.param_groups,
              "exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(),
              "max_grad_norm": self.max_grad_norm}
        if self.engine.sharded:
            sd["shard"] = self._shard_meta()
        return sd

    def load_state_dict(self, sd):
        self._check_shard_meta(sd)
        self.param_groups = [dict(g, betas=tuple(g["betas"])) for g in sd["param_groups"]]
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.state[0:1].fill_(float(sd["steps"]))
        self.sync_hyper()


class _LayerwiseOptimizer(_FlatOptimizer):
    """What FlatLARS and FlatLAMB share: the unit -> parameter map, the excluded flags, this rank's
    owned-unit table (all built once on the host), the norm buffers and the lr upload."""

    def _init_layerwise(self, engine: DataParallel, exclude, lr: float, state_len: int) -> int:
        f = engine.flat
        dev = f.data.device
        who = type(self).__name__
        if f.numel % UNIT or any(o % UNIT for o in f.offsets):
            raise ValueError(f"{who}: flat offsets must be multiples of 64 elements")
        packed = self._init_segments(engine)
        if any(lo % UNIT or hi % UNIT for lo, hi, _off in self.segments):
            raise ValueError(f"{who}: shard boundaries must be multiples of 64 elements")
        names = {id(p): n for n, p in engine.module.named_parameters()}
        pred = exclude if exclude is not None else default_no_decay
        P = len(f.params)
        self.param_names = [names.get(id(p), "") for p in f.params]
        pidx = torch.full((f.numel // UNIT,), -1, dtype=torch.int32)  # -1: alignment padding, no parameter
        excl = torch.zeros(P, dtype=torch.uint8)
        table = torch.zeros(P, 2, dtype=torch.int64)  # owned units of every parameter, packed-state indices
        for i, (p, o) in enumerate(zip(f.params, f.offsets)):
            a, b = o, o + (p.numel() + UNIT - 1) // UNIT * UNIT
            pidx[a // UNIT:b // UNIT] = i
            excl[i] = 1 if pred(self.param_names[i], p) else 0
            owned = [(max(a, lo), min(b, hi), lo, so) for lo, hi, so in self.segments if max(a, lo) < min(b, hi)]
            if len(owned) > 1:
                raise ValueError(f"{who}: parameter {self.param_names[i]!r} lies in more than one segment")
            for x, y, lo, so in owned:
                table[i, 0], table[i, 1] = (so + x - lo) // UNIT, (so + y - lo) // UNIT
        self.unit_param = pidx.to(dev)
        self.excluded = excl.to(dev)
        self.owned_units = table.to(dev)
        self._unit_parts = torch.zeros(2, max(packed // UNIT, 1), dtype=torch.float64, device=dev)
        self._sums = torch.zeros(2 * P, dtype=torch.float64, device=dev)
        self._q = torch.ones(P, dtype=torch.float32, device=dev)
        state = [0.0] * state_len
        state[1] = float(lr)
        self.state = torch.tensor(state, dtype=torch.float64, device=dev)
        self._lr_uploaded = float(lr)
        return packed

    @property
    def last_trust_ratios(self):
        """(device fp32 vector ``q``, one per parameter of the flat buffer; the parameter names)"""
        return self._q, self.param_names

    @property
    def steps(self) -> int:
        """the device step counter (a host read: not for use inside a step)"""
        return int(self.state[0].item())

    def sync_hyper(self):
        """Upload ``param_groups[0]["lr"]`` to the device state block (one fill, no host sync).
        Call it before replaying a captured step after changing ``lr``."""
        lr = float(self.param_groups[0]["lr"])
        self.state[1:2].fill_(lr)
        self._lr_uploaded = lr

    def _upload_lr(self):
        capturing = self.state.is_cuda and torch.cuda.is_current_stream_capturing()
        if float(self.param_groups[0]["lr"]) != self._lr_uploaded and not capturing:
            self.sync_hyper()

    def _parts(self, which: int, lo: int, hi: int, so: int):
        return self._unit_parts[which, so // UNIT:(so + hi - lo) // UNIT]

    def _reduce_norms(self):
        """unit partials -> per-parameter sums -> (shard mode) the one all-reduce"""
        from mi355x_dp.ops.functional import seg_sqnorm_reduce_
        e = self.engine
        seg_sqnorm_reduce_(self._unit_parts, self.owned_units, self._sums)
        if e.sharded and e.comm_on:
            # every rank then holds the same norms, hence the same q: replicas stay identical
            dist.all_reduce(self._sums, op=dist.ReduceOp.SUM, group=e.process_group)

    def _finish(self):
        e = self.engine
        if e.sharded and e.comm_on:
            e.gather_params()  # bf16 copy + transposed operands refreshed after the gather
        else:
            e.flat.refresh_transposed()  # dgrad operands of every conv, one launch


class FlatLARS(_LayerwiseOptimizer):
    """LARS (formulas in the module docstring) over the flat buffer: a norm pass, one block per
    parameter, a trust kernel and one fused update launch per segment with momentum, 1/world
    scaling and the bf16 copy refresh.  ``exclude(name, param) -> bool`` picks the parameters that
    get plain momentum SGD without weight decay (default: ``ndim <= 1``).

    ``param_groups[0]["lr"]`` may be changed between steps, under the same contract as
    ``FlatAdamW`` (``step()`` uploads it except while capturing; ``sync_hyper()`` before a replay)."""

    def __init__(self, engine: DataParallel, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                 trust_coefficient: float = 1e-3, eps: float = 1e-8,
                 exclude: Optional[Callable[[str, torch.Tensor], bool]] = None):
        from mi355x_dp.ops.functional import LARS_STATE_LEN
        packed = self._init_layerwise(engine, exclude, lr, LARS_STATE_LEN)
        self.momentum_buf = torch.zeros(packed, dtype=torch.float32, device=engine.flat.data.device)
        self.param_groups = [dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                                  trust_coefficient=trust_coefficient, eps=eps)]

    def step(self):
        from mi355x_dp.ops.functional import lars_flat_, lars_trust_, seg_sqnorm_units_
        e = self.engine
        e.finish_gradient_sync(average=False)
        g = self.param_groups[0]
        f = e.flat
        self._upload_lr()
        for lo, hi, so in self.segments:
            seg_sqnorm_units_(f.data[lo:hi], self._parts(0, lo, hi, so), f.grad[lo:hi], self._parts(1, lo, hi, so))
        self._reduce_norms()
        lars_trust_(self._sums, self.excluded, self._q, self.state, g["trust_coefficient"], g["weight_decay"],
                    g["eps"], e.grad_scale)
        for lo, hi, so in self.segments:
            lars_flat_(f.data[lo:hi], f.grad[lo:hi], self.momentum_buf[so:so + hi - lo],
                       f.bf16[lo:hi] if f.bf16 is not None else None, self.state, self.unit_param, self.excluded,
                       self._q, lo // UNIT, g["momentum"], g["weight_decay"], e.grad_scale)
        self._finish()

    def state_dict(self):
        """In shard mode ``momentum_buf`` is this rank's packed shards (a per-rank optimizer
        checkpoint, tagged with ``shard``)."""
        sd = {"steps": self.steps, "param_groups": self.param_groups,
              "momentum_buf": self.momentum_buf.detach().cpu()}
        if self.engine.sharded:
            sd["shard"] = self._shard_meta()
        return sd

    def load_state_dict(self, sd):
        self._check_shard_meta(sd)
        self.param_groups = [dict(g) for g in sd["param_groups"]]
        self.momentum_buf.copy_(sd["momentum_buf"])
        self.state[0:1].fill_(float(sd["steps"]))
        self.sync_hyper()


class FlatLAMB(_LayerwiseOptimizer):
    """LAMB (formulas in the module docstring) over the flat buffer: a one-thread prep kernel, a
    moments launch per segment that also produces the unit partials of ``w^2`` and ``u^2``, one
    block per parameter, a trust kernel and an apply launch per segment that recomputes ``u`` and
    refreshes the bf16 copy.  ``exclude(name, param) -> bool`` picks the parameters without weight
    decay and with ``q = 1`` (default: ``ndim <= 1``).  ``max_grad_norm`` clips the global gradient
    norm first, as in ``FlatAdamW``; ``last_grad_norm`` is the norm it measured.

    ``param_groups[0]["lr"]`` may be changed between steps, under the same contract as
    ``FlatAdamW``."""

    def __init__(self, engine: DataParallel, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None,
                 exclude: Optional[Callable[[str, torch.Tensor], bool]] = None):
        from mi355x_dp.ops.functional import LAMB_STATE_LEN, grad_sqnorm_slots
        packed = self._init_layerwise(engine, exclude, lr, LAMB_STATE_LEN)
        dev = engine.flat.data.device
        self.exp_avg = torch.zeros(packed, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(packed, dtype=torch.float32, device=dev)
        self.max_grad_norm = max_grad_norm
        self.param_groups = [dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps,
                                  weight_decay=weight_decay)]
        self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
        n_slots = grad_sqnorm_slots(hi - lo for lo, hi, _ in self.segments) if dev.type == "cuda" else 0
        self._partials = torch.zeros(max(n_slots, 1), dtype=torch.float64, device=dev)

    @property
    def last_grad_norm(self) -> Optional[torch.Tensor]:
        """total gradient norm of the last step (what ``clip_grad_norm_`` returns), on the device"""
        return self.state[2:3] if self.max_grad_norm is not None else None

    def step(self):
        from mi355x_dp.ops.functional import grad_sqnorm_, lamb_apply_, lamb_moments_, lamb_prep_, lamb_trust_
        e = self.engine
        e.finish_gradient_sync(average=False)
        g = self.param_groups[0]
        f = e.flat
        self._upload_lr()
        clip = self.max_grad_norm is not None
        if clip:
            grad_sqnorm_([f.grad[lo:hi] for lo, hi, _ in self.segments], self._sumsq, self._partials)
            if e.sharded and e.comm_on:
                dist.all_reduce(self._sumsq, op=dist.ReduceOp.SUM, group=e.process_group)
        b1, b2 = g["betas"]
        lamb_prep_(self.state, self._sumsq, b1, b2, self.max_grad_norm if clip else None, e.grad_scale)
        for lo, hi, so in self.segments:
            lamb_moments_(f.data[lo:hi], f.grad[lo:hi], self.exp_avg[so:so + hi - lo],
                          self.exp_avg_sq[so:so + hi - lo], self.state, self.unit_param, self.excluded, lo // UNIT,
                          self._parts(0, lo, hi, so), self._parts(1, lo, hi, so), b1, b2, g["eps"],
                          g["weight_decay"])
        self._reduce_norms()
        lamb_trust_(self._sums, self.excluded, self._q)
        for lo, hi, so in self.segments:
            lamb_apply_(f.data[lo:hi], self.exp_avg[so:so + hi - lo], self.exp_avg_sq[so:so + hi - lo],
                        f.bf16[lo:hi] if f.bf16 is not None else None, self.state, self.unit_param, self.excluded,
                        self._q, lo // UNIT, b1, b2, g["eps"], g["weight_decay"])
        self._finish()

    def state_dict(self):
        """In shard mode the moments are this rank's packed shards (a per-rank optimizer
        checkpoint, tagged with ``shard``)."""
        sd = {"steps": self.steps, "param_groups": self.param_groups,
              "exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(),
              "max_grad_norm": self.max_grad_norm}
        if self.engine.sharded:
            sd["shard"] = self._shard_meta()
        return sd

    def load_state_dict(self, sd):
        self._check_shard_meta(sd)
        self.param_groups = [dict(g, betas=tuple(g["betas"])) for g in sd["param_groups"]]
        self.exp_avg.copy_(sd["exp_avg"])
        self.exp_avg_sq.copy_(sd["exp_avg_sq"])
        self.state[0:1].fill_(float(sd["steps"]))
        self.sync_hyper()
