"""Mixup / CutMix parameter source for ``ops.augment_mix``.

``BatchMixer.params(step, N, H, W)`` draws, on the host, the per-sample mixing parameters of one
step -- the partner image, the blend factor and the CutMix box -- and sends them with ONE
non-blocking copy from pinned memory into persistent device tensors.  The draw is a pure function of
``(seed, rank, step)``: it does not depend on what was drawn before, so resuming from a checkpoint
reproduces the stream, and different ranks mix differently.  No device RNG, no host synchronisation.

Default semantics are those of the common reference transforms: one draw per batch, the partner is
the batch rolled by one (``partner[i] = (i - 1) mod N``), Mixup or CutMix chosen per batch by
``switch_prob`` (an alpha of 0 disables that mode).  CutMix geometry: the centre is uniform over the
image, the half-extents are ``int(0.5 * sqrt(1 - lam) * W)`` and ``int(0.5 * sqrt(1 - lam) * H)``,
the box is clipped to the image and lam is recomputed from the clipped area.  ``per_sample=True``
draws everything per image, with a random permutation as partner.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch


class MixParams(NamedTuple):
    """``partner`` int32 [N] (outside [0, N): no mixing), ``lam`` fp32 [N], ``box`` int32 [N, 4] =
    (y0, y1, x0, x1) in output coordinates; an empty box means Mixup, a non-empty one CutMix."""
    partner: torch.Tensor
    lam: torch.Tensor
    box: torch.Tensor


def cutmix_box(lam, cy, cx, H, W):
    """The CutMix box (y0, y1, x0, x1) of blend factor ``lam`` centred at (cy, cx), clipped to the
    H x W image, and lam recomputed from the clipped area (fp32, as the kernel computes it)."""
    r = math.sqrt(max(0.0, 1.0 - float(lam)))
    hh, hw = int(0.5 * r * H), int(0.5 * r * W)
    y0, y1 = min(max(cy - hh, 0), H), min(max(cy + hh, 0), H)
    x0, x1 = min(max(cx - hw, 0), W), min(max(cx + hw, 0), W)
    area = (y1 - y0) * (x1 - x0)
    return (y0, y1, x0, x1), float(np.float32(1.0) - np.float32(area) / np.float32(H * W))


_RING = 4  # pinned staging buffers in flight before one is reused


class BatchMixer:
    def __init__(self, mixup_alpha=0.2, cutmix_alpha=1.0, prob=1.0, switch_prob=0.5, per_sample=False, seed=0,
                 rank=0, device=None):
        if mixup_alpha < 0 or cutmix_alpha < 0:
            raise ValueError("mixup_alpha / cutmix_alpha must be >= 0 (0 disables the mode)")
        if not (0.0 <= prob <= 1.0 and 0.0 <= switch_prob <= 1.0):
            raise ValueError("prob / switch_prob must be in [0, 1]")
        self.mixup_alpha, self.cutmix_alpha = float(mixup_alpha), float(cutmix_alpha)
        self.prob, self.switch_prob = float(prob), float(switch_prob)
        self.per_sample, self.seed, self.rank = bool(per_sample), int(seed), int(rank)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self._dev = {}     # N -> persistent int32 [6 * N] device buffer
        self._stage = {}   # N -> ring of (pinned int32 [6 * N], event of its last copy)
        self._turn = 0

    # ------------------------------------------------------------------ host draw
    def host_params(self, step, N, H, W):
        """(partner int32 [N], lam fp32 [N], box int32 [N, 4]) as numpy arrays: a pure function of
        (seed, rank, step).  Every variate is drawn on every call, in a fixed order, whatever the
        settings use of them."""
        rng = np.random.default_rng(np.random.SeedSequence([self.seed, self.rank, int(step)]))
        n = N if self.per_sample else 1
        u_mix, u_switch = rng.random(n), rng.random(n)
        # Beta(0, 0) is undefined; a disabled mode's draw is discarded below
        lam_m = rng.beta(self.mixup_alpha or 1.0, self.mixup_alpha or 1.0, n)
        lam_c = rng.beta(self.cutmix_alpha or 1.0, self.cutmix_alpha or 1.0, n)
        cy, cx = rng.integers(0, H, n), rng.integers(0, W, n)
        perm = rng.permutation(N)
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            use_cut = u_switch < self.switch_prob
        else:
            use_cut = np.full(n, self.cutmix_alpha > 0)
        active = (u_mix < self.prob) & (self.mixup_alpha > 0 or self.cutmix_alpha > 0)
        lam = np.ones(n, np.float32)
        box = np.zeros((n, 4), np.int32)
        for i in range(n):
            if not active[i]:
                continue
            if use_cut[i]:
                box[i], lam[i] = cutmix_box(lam_c[i], int(cy[i]), int(cx[i]), H, W)
                if lam[i] == 1.0:  # zero-area box: nothing is pasted
                    box[i] = 0
            else:
                lam[i] = lam_m[i]
        if self.per_sample:
            partner = perm.astype(np.int32)
        else:
            partner = ((np.arange(N) - 1) % N).astype(np.int32)
            lam, box = np.repeat(lam, N), np.repeat(box, N, axis=0)
        return partner, lam, box

    # ------------------------------------------------------------------ device side
    def upload(self, partner, lam, box):
        """Pack host parameters and send them with one non-blocking copy into the persistent device
        tensors of this batch size.  A partner outside [0, N) raises here: on the device it would
        silently mean "no mixing"."""
        partner = np.asarray(partner)
        N = partner.shape[0]
        lam = np.asarray(lam, np.float32)
        box = np.asarray(box, np.int32)
        if lam.shape != (N,) or box.shape != (N, 4):
            raise ValueError(f"expected partner [{N}], lam [{N}] and box [{N}, 4]")
        if N and (partner.min() < 0 or partner.max() >= N):
            raise ValueError(f"partner index out of range [0, {N})")
        if self.device.type != "cuda":
            buf = torch.empty(6 * N, dtype=torch.int32)
            self._pack(buf, partner, lam, box, N)
            return self._views(buf, N)
        if N not in self._dev:
            self._dev[N] = torch.empty(6 * N, dtype=torch.int32, device=self.device)
            self._stage[N] = [(torch.empty(6 * N, dtype=torch.int32).pin_memory(), torch.cuda.Event())
                              for _ in range(_RING)]
        self._turn = (self._turn + 1) % _RING
        host, ev = self._stage[N][self._turn]
        # the copy issued _RING uploads ago from this buffer has long completed, so nothing waits here;
        # the guard only keeps the buffer from being rewritten under a copy that is still in flight
        if not ev.query():
            ev.synchronize()
        self._pack(host, partner, lam, box, N)
        self._dev[N].copy_(host, non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))
        return self._views(self._dev[N], N)

    @staticmethod
    def _pack(buf, partner, lam, box, N):
        a = buf.numpy()
        a[:N] = partner
        a[N:2 * N] = lam.view(np.int32)
        a[2 * N:] = box.reshape(-1)

    @staticmethod
    def _views(buf, N):
        return MixParams(buf[:N], buf[N:2 * N].view(torch.float32), buf[2 * N:].view(N, 4))

    def params(self, step, N, H, W):
        """``MixParams`` of this step on the mixer's device (views of one persistent buffer per batch
        size: valid until the next call with the same N)."""
        return self.upload(*self.host_params(step, N, H, W))
