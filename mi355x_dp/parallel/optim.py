"""The flat optimizers: ``FlatSGD``, ``FlatAdamW``, ``FlatLARS`` and ``FlatLAMB`` update the engine's
flat fp32 master buffer with fused launches per segment and refresh the bf16 copy in the same pass.
``_FlatSegments`` holds the packed segments, their layout checks and the shard metadata (shared
with ``FlatEMA``), ``_FlatOptimizer`` what all four add (flat slices, the step tail),
``_DeviceStateOptimizer`` what the three with a device state block share (``lr`` upload,
the global-norm pass, checkpoints), ``_LayerwiseOptimizer`` the segmented norms of LARS and LAMB.

``FlatAdamW``: torch.optim.AdamW semantics over the engine's flat buffers, with global-norm
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

from .ddp import DataParallel

UNIT = 64  # elements per decay-map byte (= the flat buffer's parameter alignment)


def default_no_decay(name: str, param: torch.Tensor) -> bool:
    """biases, BatchNorm / LayerNorm weights: every parameter with at most one dimension"""
    return param.ndim <= 1


class _FlatSegments:
    """Per-element state packed to the ranges of the flat buffer this rank updates -- what the flat
    optimizers and ``FlatEMA`` (ema.py) share: the segments with their layout checks and slices,
    and the shard metadata of their per-rank checkpoints."""

    # which segment ends must be multiples of 64 elements (with every flat offset): None = no
    # requirement, "lo" = the starts, "lo_hi" = starts and ends
    unit_aligned: Optional[str] = None

    def _init_segments(self, engine: DataParallel) -> int:
        """``self.segments`` = (flat lo, flat hi, packed-state offset) per range this rank updates
        (shard mode: its shard of every bucket, packed -- 1/world of the optimizer state; otherwise
        the whole flat buffer).  Returns the packed size."""
        who, f, ends = type(self).__name__, engine.flat, self.unit_aligned
        if ends and (f.numel % UNIT or any(o % UNIT for o in f.offsets)):
            raise ValueError(f"{who}: flat offsets must be multiples of 64 elements")
        self.engine = engine
        self.segments = []
        off = 0
        for lo, hi in engine.shard_ranges if engine.sharded else [(0, f.numel)]:
            self.segments.append((lo, hi, off))
            off += hi - lo
        if ends and any(lo % UNIT or (ends == "lo_hi" and hi % UNIT) for lo, hi, _off in self.segments):
            raise ValueError(f"{who}: shard boundaries must be multiples of 64 elements")
        return off

    @staticmethod
    def _packed(t, seg):
        """one segment's slice of a packed state tensor"""
        lo, hi, off = seg
        return t[off:off + hi - lo]

    def _shard_meta(self):
        """Which slice of the packed momentum belongs to which flat range: the bucket plan (flat
        [lo, hi) of every bucket and of this rank's shard of it) depends on the planner settings
        and, with calibrate=True, on timing -- a resume must see the same plan."""
        e = self.engine
        return {"rank": e.rank, "world": e.world_size, "numel": int(e.flat.numel),
                "bucket_ranges": [[int(lo), int(hi)] for lo, hi in e.bucket_ranges],
                "shard_ranges": [[int(lo), int(hi)] for lo, hi in e.shard_ranges]}

    def _check_shard_meta(self, sd):
        if not self.engine.sharded:
            return
        want, got = self._shard_meta(), sd.get("shard") or {}
        if {k: got.get(k) for k in ("rank", "world")} != {"rank": want["rank"], "world": want["world"]}:
            raise ValueError(f"optimizer shard (rank {got.get('rank')} of {got.get('world')}) does not match "
                             f"this rank ({want['rank']} of {want['world']})")
        for k in ("numel", "bucket_ranges", "shard_ranges"):
            if got.get(k) != want[k]:
                raise ValueError(f"optimizer shard checkpoint was written with a different bucket plan ({k} "
                                 "differs): its packed momentum would pair with the wrong parameters; resume "
                                 "with the same bucket_cap_mb / first / last / min bucket settings and without "
                                 "calibrate=True")


class _FlatOptimizer(_FlatSegments):
    """What the flat optimizers share beyond ``_FlatSegments``: the parameter names, the flat
    slices of a segment and the step tail."""

    def _names(self):
        """the module's name of every parameter of the flat buffer ("" where it has none)"""
        names = {id(p): n for n, p in self.engine.module.named_parameters()}
        return [names.get(id(p), "") for p in self.engine.flat.params]

    def _flat(self, seg):
        """(master, gradient, bf16 copy or None) slices of one segment"""
        lo, hi, _off = seg
        f = self.engine.flat
        return f.data[lo:hi], f.grad[lo:hi], f.bf16[lo:hi] if f.bf16 is not None else None

    def zero_grad(self, set_to_none: bool = False):
        self.engine.zero_grad()

    def _finish(self):
        """the step tail: publish the updated parameters to the compute copies"""
        e = self.engine
        if e.sharded and e.comm_on:
            e.gather_params()  # bf16 copy + transposed operands refreshed after the gather
        else:
            e.flat.refresh_transposed()  # dgrad operands of every conv, one launch


class FlatSGD(_FlatOptimizer):
    """torch.optim.SGD semantics over the flat buffer in ONE fused kernel launch
    (momentum + weight decay + 1/world + bf16 copy refresh)."""

    def __init__(self, engine: DataParallel, lr: float, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False):
        self.lr, self.momentum, self.dampening = lr, momentum, dampening
        self.weight_decay, self.nesterov = weight_decay, nesterov
        # shard mode: momentum only for this rank's shards, packed (1/world of the optimizer state)
        off = self._init_segments(engine)
        self.momentum_buf = torch.zeros(off, dtype=torch.float32, device=engine.flat.data.device) if momentum else None
        self.steps = 0
        self.param_groups = [dict(lr=lr, momentum=momentum, weight_decay=weight_decay, nesterov=nesterov,
                                  dampening=dampening)]

    def step(self):
        from mi355x_dp.ops.functional import sgd_flat_
        self.engine.finish_gradient_sync(average=False)
        g = self.param_groups[0]
        for seg in self.segments:
            p, grad, p16 = self._flat(seg)
            mom = self._packed(self.momentum_buf, seg) if self.momentum_buf is not None else None
            sgd_flat_(p, grad, mom, p16, g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"],
                      first_step=(self.steps == 0), grad_scale=self.engine.grad_scale)
        self._finish()
        self.steps += 1

    def state_dict(self):
        """In shard mode ``momentum_buf`` is this rank's packed shards (a per-rank optimizer
        checkpoint, tagged with ``shard``)."""
        sd = {"steps": self.steps, "param_groups": self.param_groups,
              "momentum_buf": self.momentum_buf.detach().cpu() if self.momentum_buf is not None else None}
        if self.engine.sharded:
            sd["shard"] = self._shard_meta()
        return sd

    def load_state_dict(self, sd):
        self._check_shard_meta(sd)
        self.steps = sd["steps"]
        self.param_groups = sd["param_groups"]
        if sd.get("momentum_buf") is not None and self.momentum_buf is not None:
            self.momentum_buf.copy_(sd["momentum_buf"])


class _DeviceStateOptimizer(_FlatOptimizer):
    """What FlatAdamW, FlatLARS and FlatLAMB share: the device state block (``state[0]`` the step
    count, ``state[1]`` ``lr``; the rest per optimizer, ops/functional.py), the ``lr`` upload, the
    global gradient norm of the clipping optimizers and the checkpoints.

    A subclass names its packed per-element state tensors in ``state_tensors`` and sets ``clips``
    when it takes ``max_grad_norm``."""

    state_tensors = ()
    clips = False
    max_grad_norm = None

    def _init_state(self, engine: DataParallel, lr: float, state_len: int,
                    max_grad_norm: Optional[float] = None) -> int:
        """segments, the zeroed state tensors, the state block and (``clips``) the norm buffers;
        returns the packed size"""
        from mi355x_dp.ops.functional import grad_sqnorm_slots
        packed = self._init_segments(engine)
        dev = engine.flat.data.device
        for name in self.state_tensors:
            setattr(self, name, torch.zeros(packed, dtype=torch.float32, device=dev))
        state = [0.0] * state_len
        state[1] = float(lr)
        self.state = torch.tensor(state, dtype=torch.float64, device=dev)
        self._lr_uploaded = float(lr)
        if self.clips:
            self.max_grad_norm = max_grad_norm
            self._sumsq = torch.zeros(1, dtype=torch.float64, device=dev)
            n_slots = grad_sqnorm_slots(hi - lo for lo, hi, _ in self.segments) if dev.type == "cuda" else 0
            self._partials = torch.zeros(max(n_slots, 1), dtype=torch.float64, device=dev)
        return packed

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

    def _begin(self):
        """finish the gradient sync and upload a changed ``lr`` -- except while the stream is
        capturing, where a baked fill would reset it on every replay; returns the hyper-parameters"""
        self.engine.finish_gradient_sync(average=False)
        capturing = self.state.is_cuda and torch.cuda.is_current_stream_capturing()
        if float(self.param_groups[0]["lr"]) != self._lr_uploaded and not capturing:
            self.sync_hyper()
        return self.param_groups[0]

    def _grad_sqnorm(self):
        """with ``max_grad_norm``: ``_sumsq`` = the squared gradient norm over all ranks' segments"""
        from mi355x_dp.ops.functional import grad_sqnorm_
        if self.max_grad_norm is None:
            return
        e = self.engine
        grad_sqnorm_([e.flat.grad[lo:hi] for lo, hi, _ in self.segments], self._sumsq, self._partials)
        if e.sharded and e.comm_on:
            # every rank then holds the same norm, hence the same coefficient: replicas stay identical
            dist.all_reduce(self._sumsq, op=dist.ReduceOp.SUM, group=e.process_group)

    # --------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        """In shard mode the state tensors are this rank's packed shards (a per-rank optimizer
        checkpoint, tagged with ``shard``)."""
        sd = {"steps": self.steps, "param_groups": self.param_groups}
        for name in self.state_tensors:
            sd[name] = getattr(self, name).detach().cpu()
        if self.clips:
            sd["max_grad_norm"] = self.max_grad_norm
        if self.engine.sharded:
            sd["shard"] = self._shard_meta()
        return sd

    def load_state_dict(self, sd):
        self._check_shard_meta(sd)
        self.param_groups = [dict(g, betas=tuple(g["betas"])) if "betas" in g else dict(g)
                             for g in sd["param_groups"]]
        for name in self.state_tensors:
            getattr(self, name).copy_(sd[name])
        self.state[0:1].fill_(float(sd["steps"]))
        self.sync_hyper()


class FlatAdamW(_DeviceStateOptimizer):
    """AdamW (no amsgrad, no maximize) over the flat buffer: one fused launch per segment with
    weight decay chosen per parameter, 1/world scaling, clipping and the bf16 copy refresh.

    ``no_decay(name, param) -> bool`` picks the parameters without weight decay (default:
    ``ndim <= 1``).  ``max_grad_norm`` clips the global gradient norm like
    ``torch.nn.utils.clip_grad_norm_``; the norm it would have returned is ``last_grad_norm`` (a
    one-element device tensor; ``float('inf')`` measures without clipping, None skips the pass).

    ``param_groups[0]["lr"]`` may be changed between steps: ``step()`` uploads it -- except while
    the stream is capturing, where a baked fill would reset it on every replay; before a replay
    push a new value with ``sync_hyper()``."""

    state_tensors = ("exp_avg", "exp_avg_sq")
    clips = True
    unit_aligned = "lo"

    def __init__(self, engine: DataParallel, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None,
                 no_decay: Optional[Callable[[str, torch.Tensor], bool]] = None):
        from mi355x_dp.ops.functional import ADAMW_STATE_LEN
        self._init_state(engine, lr, ADAMW_STATE_LEN, max_grad_norm)
        self.param_groups = [dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps,
                                  weight_decay=weight_decay)]
        # one byte per 64-element unit: 1 = decays.  A unit never straddles two parameters;
        # alignment padding (zero in p, g, m, v) stays zero either way
        f = engine.flat
        pred = no_decay if no_decay is not None else default_no_decay
        dmap = torch.zeros(f.numel // UNIT, dtype=torch.uint8)
        for name, p, o in zip(self._names(), f.params, f.offsets):
            if not pred(name, p):
                dmap[o // UNIT:(o + p.numel() + UNIT - 1) // UNIT] = 1
        self.decay_map = dmap.to(f.data.device)

    def step(self):
        from mi355x_dp.ops.functional import adamw_flat_, adamw_prep_
        g = self._begin()
        b1, b2 = g["betas"]
        self._grad_sqnorm()
        adamw_prep_(self.state, self._sumsq, b1, b2, g["weight_decay"], self.max_grad_norm, self.engine.grad_scale)
        for seg in self.segments:
            p, grad, p16 = self._flat(seg)
            adamw_flat_(p, grad, self._packed(self.exp_avg, seg), self._packed(self.exp_avg_sq, seg), p16, self.state,
                        b1, b2, g["eps"], self.decay_map, seg[0] // UNIT)
        self._finish()


class _LayerwiseOptimizer(_DeviceStateOptimizer):
    """What FlatLARS and FlatLAMB share: the unit -> parameter map, the excluded flags, this rank's
    owned-unit table (all built once on the host) and the norm buffers."""

    unit_aligned = "lo_hi"

    def _init_layerwise(self, engine: DataParallel, exclude, lr: float, state_len: int, max_grad_norm=None):
        packed = self._init_state(engine, lr, state_len, max_grad_norm)
        f = engine.flat
        dev = f.data.device
        pred = exclude if exclude is not None else default_no_decay
        P = len(f.params)
        self.param_names = self._names()
        pidx = torch.full((f.numel // UNIT,), -1, dtype=torch.int32)  # -1: alignment padding, no parameter
        excl = torch.zeros(P, dtype=torch.uint8)
        table = torch.zeros(P, 2, dtype=torch.int64)  # owned units of every parameter, packed-state indices
        for i, (p, o) in enumerate(zip(f.params, f.offsets)):
            a, b = o, o + (p.numel() + UNIT - 1) // UNIT * UNIT
            pidx[a // UNIT:b // UNIT] = i
            excl[i] = 1 if pred(self.param_names[i], p) else 0
            owned = [(max(a, lo), min(b, hi), lo, so) for lo, hi, so in self.segments if max(a, lo) < min(b, hi)]
            if len(owned) > 1:
                raise ValueError(f"{type(self).__name__}: parameter {self.param_names[i]!r} lies in more than "
                                 "one segment")
            for x, y, lo, so in owned:
                table[i, 0], table[i, 1] = (so + x - lo) // UNIT, (so + y - lo) // UNIT
        self.unit_param = pidx.to(dev)
        self.excluded = excl.to(dev)
        self.owned_units = table.to(dev)
        self._unit_parts = torch.zeros(2, max(packed // UNIT, 1), dtype=torch.float64, device=dev)
        self._sums = torch.zeros(2 * P, dtype=torch.float64, device=dev)
        self._q = torch.ones(P, dtype=torch.float32, device=dev)

    @property
    def last_trust_ratios(self):
        """(device fp32 vector ``q``, one per parameter of the flat buffer; the parameter names)"""
        return self._q, self.param_names

    def _parts(self, seg):
        """one segment's slices of the two rows of unit partials"""
        lo, hi, so = seg
        return self._unit_parts[:, so // UNIT:(so + hi - lo) // UNIT]

    def _reduce_norms(self):
        """unit partials -> per-parameter sums -> (shard mode) the one all-reduce"""
        from mi355x_dp.ops.functional import seg_sqnorm_reduce_
        e = self.engine
        seg_sqnorm_reduce_(self._unit_parts, self.owned_units, self._sums)
        if e.sharded and e.comm_on:
            # every rank then holds the same norms, hence the same q: replicas stay identical
            dist.all_reduce(self._sums, op=dist.ReduceOp.SUM, group=e.process_group)


class FlatLARS(_LayerwiseOptimizer):
    """LARS (formulas in the module docstring) over the flat buffer: a norm pass, one block per
    parameter, a trust kernel and one fused update launch per segment with momentum, 1/world
    scaling and the bf16 copy refresh.  ``exclude(name, param) -> bool`` picks the parameters that
    get plain momentum SGD without weight decay (default: ``ndim <= 1``).

    ``param_groups[0]["lr"]`` may be changed between steps, under the same contract as
    ``FlatAdamW`` (``step()`` uploads it except while capturing; ``sync_hyper()`` before a replay)."""

    state_tensors = ("momentum_buf",)

    def __init__(self, engine: DataParallel, lr: float, momentum: float = 0.9, weight_decay: float = 0.0,
                 trust_coefficient: float = 1e-3, eps: float = 1e-8,
                 exclude: Optional[Callable[[str, torch.Tensor], bool]] = None):
        from mi355x_dp.ops.functional import LARS_STATE_LEN
        self._init_layerwise(engine, exclude, lr, LARS_STATE_LEN)
        self.param_groups = [dict(lr=lr, momentum=momentum, weight_decay=weight_decay,
                                  trust_coefficient=trust_coefficient, eps=eps)]

    def step(self):
        from mi355x_dp.ops.functional import lars_flat_, lars_trust_, seg_sqnorm_units_
        g = self._begin()
        scale = self.engine.grad_scale
        for seg in self.segments:
            p, grad, _p16 = self._flat(seg)
            part_w, part_g = self._parts(seg)
            seg_sqnorm_units_(p, part_w, grad, part_g)
        self._reduce_norms()
        lars_trust_(self._sums, self.excluded, self._q, self.state, g["trust_coefficient"], g["weight_decay"],
                    g["eps"], scale)
        for seg in self.segments:
            p, grad, p16 = self._flat(seg)
            lars_flat_(p, grad, self._packed(self.momentum_buf, seg), p16, self.state, self.unit_param, self.excluded,
                       self._q, seg[0] // UNIT, g["momentum"], g["weight_decay"], scale)
        self._finish()


class FlatLAMB(_LayerwiseOptimizer):
    """LAMB (formulas in the module docstring) over the flat buffer: a one-thread prep kernel, a
    moments launch per segment that also produces the unit partials of ``w^2`` and ``u^2``, one
    block per parameter, a trust kernel and an apply launch per segment that recomputes ``u`` and
    refreshes the bf16 copy.  ``exclude(name, param) -> bool`` picks the parameters without weight
    decay and with ``q = 1`` (default: ``ndim <= 1``).  ``max_grad_norm`` clips the global gradient
    norm first, as in ``FlatAdamW``; ``last_grad_norm`` is the norm it measured.

    ``param_groups[0]["lr"]`` may be changed between steps, under the same contract as
    ``FlatAdamW``."""

    state_tensors = ("exp_avg", "exp_avg_sq")
    clips = True

    def __init__(self, engine: DataParallel, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-6,
                 weight_decay: float = 1e-2, max_grad_norm: Optional[float] = None,
                 exclude: Optional[Callable[[str, torch.Tensor], bool]] = None):
        from mi355x_dp.ops.functional import LAMB_STATE_LEN
        self._init_layerwise(engine, exclude, lr, LAMB_STATE_LEN, max_grad_norm)
        self.param_groups = [dict(lr=lr, betas=(float(betas[0]), float(betas[1])), eps=eps,
                                  weight_decay=weight_decay)]

    def step(self):
        from mi355x_dp.ops.functional import lamb_apply_, lamb_moments_, lamb_prep_, lamb_trust_
        g = self._begin()
        b1, b2 = g["betas"]
        self._grad_sqnorm()
        lamb_prep_(self.state, self._sumsq, b1, b2, self.max_grad_norm, self.engine.grad_scale)
        for seg in self.segments:
            p, grad, _p16 = self._flat(seg)
            part_w, part_u = self._parts(seg)
            lamb_moments_(p, grad, self._packed(self.exp_avg, seg), self._packed(self.exp_avg_sq, seg), self.state,
                          self.unit_param, self.excluded, seg[0] // UNIT, part_w, part_u, b1, b2, g["eps"],
                          g["weight_decay"])
        self._reduce_norms()
        lamb_trust_(self._sums, self.excluded, self._q)
        for seg in self.segments:
            p, _grad, p16 = self._flat(seg)
            lamb_apply_(p, self._packed(self.exp_avg, seg), self._packed(self.exp_avg_sq, seg), p16, self.state,
                        self.unit_param, self.excluded, self._q, seg[0] // UNIT, b1, b2, g["eps"], g["weight_decay"])
        self._finish()
