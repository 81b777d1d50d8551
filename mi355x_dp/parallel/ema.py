"""``FlatEMA``: an exponential moving average of the weights on the flat buffer, and evaluation
with the averaged weights by an in-place exchange.

The averaged weights are one more fp32 buffer with the flat buffer's layout (in shard mode packed
to this rank's shards, like ``exp_avg``: 1/world of the flat buffer).  One call of ``update()`` is
a one-thread prep kernel and one fused launch per segment (csrc/kernels/ema.hip).  What changes
per call lives in a device state block that the prep kernel advances, so a step captured by
``GraphedStep`` averages correctly on every replay; nothing in ``update()`` reads the device.

State block (float64): ``[0]`` calls ``c``, ``[1]`` updates ``n``, ``[2]`` ``w`` of this call,
``[3]`` ``decay``, ``[4]`` ``d_t``.  One call, the scalars in fp64::

    c += 1
    if c % update_every != 0:   skip (w = 0, the average is not touched)
    else:  d_t = decay                                    without warm-up
               = min(decay, (1 + n) / (warmup + n))       with warm-up
           w = 1 - d_t ;  n += 1
           ema = fma(float(w), p - ema, ema)              per element, fp32

``applied()`` evaluates with the averaged weights without a third buffer: the average and the
master weights are exchanged in place (32-bit moves: the exchange is its own inverse bit for
bit), the compute copies (bf16, transposed operands) are refreshed the way the optimizers' step
tail does it, and on exit the same sequence puts the training weights back.  Evaluation therefore
runs on the same native kernels as training.
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch

from .ddp import DataParallel
from .optim import _FlatSegments


class FlatEMA(_FlatSegments):
    """Exponential moving average of an engine's weights (``torch.optim.swa_utils.AveragedModel``
    with ``get_ema_multi_avg_fn``, timm's ``ModelEma``) over the flat buffer.

    Construct it after loading a checkpoint into the model: the average starts as a copy of the
    master weights.  Call ``update()`` after ``optimizer.step()``.

    ``warmup``: None, or ``>= 1`` for ``d_t = min(decay, (1 + n) / (warmup + n))``.
    ``update_every``: average on every ``update_every``-th call only.
    ``buffers``: ``"live"`` (``AveragedModel(use_buffers=False)``): BatchNorm running statistics
    are never averaged and evaluation uses the live ones; ``"average"`` (``use_buffers=True``): the
    floating-point buffers are averaged with the same weight.  Integer buffers
    (``num_batches_tracked``) are never touched.

    ``decay`` may be changed between calls: ``update()`` uploads it -- except while the stream is
    capturing, where a baked fill would reset it on every replay; before a replay push a new value
    with ``sync_hyper()``."""

    unit_aligned = "lo_hi"

    def __init__(self, engine: DataParallel, decay: float = 0.9999, warmup: Optional[float] = None,
                 update_every: int = 1, buffers: str = "live"):
        from mi355x_dp.ops.functional import EMA_STATE_LEN
        self._check_decay(decay)
        if warmup is not None and not warmup >= 1:
            raise ValueError(f"FlatEMA: warmup must be None or >= 1, not {warmup!r}")
        if isinstance(update_every, bool) or not isinstance(update_every, int) or update_every < 1:
            raise ValueError(f"FlatEMA: update_every must be an integer >= 1, not {update_every!r}")
        if buffers not in ("live", "average"):
            raise ValueError(f"FlatEMA: buffers must be 'live' or 'average', not {buffers!r}")
        self.decay, self.warmup, self.update_every, self.buffers = float(decay), warmup, update_every, buffers
        packed = self._init_segments(engine)
        engine._wait_buffer_sync()
        engine.wait_param_sync()
        f = engine.flat
        self.avg = torch.empty(packed, dtype=torch.float32, device=f.data.device)
        for seg in self.segments:
            self._packed(self.avg, seg).copy_(f.data[seg[0]:seg[1]])
        # the floating-point buffer block: full on every rank, arbitrary length (no alignment)
        self._n_buf = sum(b.numel() for b in engine.buffers.buffers)
        self.avg_buffers = (engine.buffers.data[:self._n_buf].clone()
                            if buffers == "average" and self._n_buf else None)
        state = [0.0] * EMA_STATE_LEN
        state[3] = self.decay
        self.state = torch.tensor(state, dtype=torch.float64, device=f.data.device)
        self._decay_uploaded = self.decay
        self._applied = False

    @staticmethod
    def _check_decay(decay):
        if not 0 <= decay < 1:
            raise ValueError(f"FlatEMA: decay must satisfy 0 <= decay < 1, not {decay!r}")

    # ------------------------------------------------------------------ device-resident scalars
    @property
    def num_updates(self) -> int:
        """updates taken so far (a host read of ``state[1]``: not for use inside a step)"""
        return int(self.state[1].item())

    @property
    def num_calls(self) -> int:
        """``update()`` calls so far (a host read of ``state[0]``: not for use inside a step)"""
        return int(self.state[0].item())

    def sync_hyper(self):
        """Upload ``self.decay`` to the device state block (one fill, no host sync).  Call it
        before replaying a captured step after changing ``decay``."""
        self._check_decay(self.decay)
        self.state[3:4].fill_(float(self.decay))
        self._decay_uploaded = float(self.decay)

    # --------------------------------------------------------------------------------- update
    def _live_buffers(self):
        return self.engine.buffers.data[:self._n_buf]

    def update(self):
        """One prep launch, then one update launch per segment, on the current stream.  In shard
        mode the optimizer's tail has already started the parameter all-gather: it reads this
        rank's own shards of ``flat.data`` and writes the others, and so does nothing to the
        ranges read here -- no wait."""
        from mi355x_dp.ops.functional import ema_prep_, ema_update_
        if self._applied:
            raise RuntimeError("FlatEMA.update() inside applied(): the flat buffer holds the averaged weights")
        e = self.engine
        capturing = self.state.is_cuda and torch.cuda.is_current_stream_capturing()
        if float(self.decay) != self._decay_uploaded and not capturing:
            self.sync_hyper()
        ema_prep_(self.state, self.warmup, self.update_every)
        for seg in self.segments:
            ema_update_(self._packed(self.avg, seg), e.flat.data[seg[0]:seg[1]], self.state)
        if self.avg_buffers is not None:
            # ranks other than 0 receive the running statistics by an asynchronous broadcast
            e._wait_buffer_sync()
            ema_update_(self.avg_buffers, self._live_buffers(), self.state)

    # ------------------------------------------------------------------------------ evaluation
    def _exchange(self):
        """average <-> master weights (and buffers), then publish to the compute copies"""
        from mi355x_dp.ops.functional import ema_swap_
        e = self.engine
        e._wait_buffer_sync()
        e.wait_param_sync()
        for seg in self.segments:
            ema_swap_(self._packed(self.avg, seg), e.flat.data[seg[0]:seg[1]])
        if self.avg_buffers is not None:
            ema_swap_(self.avg_buffers, self._live_buffers())
        if e.sharded:
            e.gather_params()
            e.wait_param_sync()  # refreshes the bf16 copy and the transposed operands
        else:
            e.flat.refresh_bf16()  # directly, so a foreign_optimizer engine's next forward is current too

    @contextlib.contextmanager
    def applied(self):
        """Evaluate with the averaged weights::

            with ema.applied():
                engine.eval(); evaluate(engine)

        Inside the block ``engine.module`` holds the averaged weights (with ``buffers="average"``
        also the averaged statistics) in every copy the native kernels read; leaving it, also by
        an exception, restores the training weights bit for bit.  Not capturable; in shard mode a
        collective: every rank must enter."""
        if self._applied:
            raise RuntimeError("FlatEMA.applied() is already active")
        self._exchange()
        self._applied = True
        try:
            yield self
        finally:
            self._exchange()
            self._applied = False

    def module_state_dict(self):
        """The averaged model in ``model.pth`` layout: cloned CPU tensors of
        ``engine.module.state_dict()`` taken inside ``applied()`` (in shard mode a collective).
        ``with ema.applied(): save_model(engine.module, dir)`` writes a servable averaged
        ``model.pth``."""
        with self.applied():
            return {k: v.detach().cpu().clone() for k, v in self.engine.module.state_dict().items()}

    # ----------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        """In shard mode ``avg`` is this rank's packed shards (a per-rank checkpoint, tagged with
        ``shard``)."""
        st = self.state.tolist()
        sd = {"avg": self.avg.detach().cpu(),
              "avg_buffers": self.avg_buffers.detach().cpu() if self.avg_buffers is not None else None,
              "calls": int(st[0]), "updates": int(st[1]), "decay": float(self.decay), "warmup": self.warmup,
              "update_every": self.update_every, "buffers": self.buffers}
        if self.engine.sharded:
            sd["shard"] = self._shard_meta()
        return sd

    def load_state_dict(self, sd):
        self._check_shard_meta(sd)
        if sd["buffers"] != self.buffers:
            raise ValueError(f"FlatEMA: checkpoint was written with buffers={sd['buffers']!r}, "
                             f"this one has buffers={self.buffers!r}")
        if sd["avg"].numel() != self.avg.numel():
            raise ValueError(f"FlatEMA: checkpoint holds {sd['avg'].numel()} averaged elements, "
                             f"this one {self.avg.numel()}")
        self.decay, self.warmup, self.update_every = float(sd["decay"]), sd["warmup"], int(sd["update_every"])
        self.avg.copy_(sd["avg"])
        if self.avg_buffers is not None:
            self.avg_buffers.copy_(sd["avg_buffers"])
        self.state[0:1].fill_(float(sd["calls"]))
        self.state[1:2].fill_(float(sd["updates"]))
        self.sync_hyper()
