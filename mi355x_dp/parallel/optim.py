"""``FlatAdamW``: torch.optim.AdamW semantics over the engine's flat buffers, with global-norm
gradient clipping computed on the device -- the way a ViT is normally trained (AdamW, no weight
decay on biases / norms / tokens, ``clip_grad_norm_``) without leaving the flat-buffer design.

One step is: squared-norm pass (only when clipping) -> in shard mode a one-element all-reduce ->
a one-thread prep kernel -> one fused update launch per segment (csrc/kernels/optim.hip).
Everything that changes per step -- the step count, ``lr``, the bias corrections, the clip
coefficient -- lives in a small device state block that the prep kernel advances, so a captured
step (``GraphedStep``, the graphed engine) replays with the right corrections; nothing in
``step()`` reads the device.
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
