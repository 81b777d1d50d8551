"""RandomResizedCrop / RandomErasing / centre-crop parameter source for ``ops.augment_resized``.

``BatchCropper.params(step, N, Hs, Ws)`` draws, on the host, the per-image geometry of one step --
the crop box in the source, the flip and the erase box in the output -- and sends it with ONE
non-blocking copy from pinned memory into persistent device tensors, as ``data.mix.BatchMixer`` does
for the mixing parameters.  The draw is a pure function of ``(seed, rank, step)``: resuming from a
checkpoint reproduces the stream, different ranks crop differently, and a captured ``GraphedStep``
sees new values on every replay.  No device RNG, no host synchronisation.

The draws are those of the common reference transforms, vectorised over the batch.  Crop: ten tries
per image of ``area = Hs * Ws * U(scale)``, ``aspect = exp(U(log r0, log r1))``,
``w = round(sqrt(area * aspect))``, ``h = round(sqrt(area / aspect))``; the first try with
``0 < w <= Ws`` and ``0 < h <= Hs`` wins and is placed uniformly; otherwise the central crop with the
image's ratio clamped to ``ratio``.  Erase: with probability ``erase_prob``, ten tries in output
coordinates of ``h = round(sqrt(area * aspect))``, ``w = round(sqrt(area / aspect))``, accepted when
``h < Ho`` and ``w < Wo``; otherwise no box.  The erased value is 0 in normalized space.

Not done here (nor in the kernel): antialiased downscaling, bicubic resampling, sources of unequal
size within one batch, RandAugment / TrivialAugment.
"""
from __future__ import annotations

import math
from typing import NamedTuple

import numpy as np
import torch

TAG = 0x63726F70  # "crop": keeps this stream apart from BatchMixer's at the same (seed, rank, step)
_TRIES = 10
_RING = 4  # pinned staging buffers in flight before one is reused


class GeoParams(NamedTuple):
    """``crop`` int32 [N, 4] = (top, left, height, width) in source pixels, ``flip`` int32 [N],
    ``erase`` int32 [N, 4] = (y0, y1, x0, x1) in output pixels; an empty box erases nothing."""
    crop: torch.Tensor
    flip: torch.Tensor
    erase: torch.Tensor


def fallback_crop(Hs, Ws, ratio):
    """(top, left, height, width) of the central crop taken when no try fits: the whole image, with
    its aspect ratio clamped to ``ratio``."""
    in_ratio = Ws / Hs
    if in_ratio < min(ratio):
        w = Ws
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = Hs
        w = int(round(h * max(ratio)))
    else:
        w, h = Ws, Hs
    h, w = min(max(h, 1), Hs), min(max(w, 1), Ws)
    return (Hs - h) // 2, (Ws - w) // 2, h, w


def _first_true(ok):
    """Index of the first True per row and whether the row has one."""
    return ok.argmax(axis=1), ok.any(axis=1)


class BatchCropper:
    def __init__(self, size, scale=(0.08, 1.0), ratio=(3 / 4, 4 / 3), flip_prob=0.5, erase_prob=0.0,
                 erase_scale=(0.02, 0.33), erase_ratio=(0.3, 3.3), seed=0, rank=0, device=None):
        self.size = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
        if min(self.size) < 1:
            raise ValueError("size must be positive")
        for name, (lo, hi) in (("scale", scale), ("ratio", ratio), ("erase_scale", erase_scale),
                               ("erase_ratio", erase_ratio)):
            if not 0 < lo <= hi:
                raise ValueError(f"{name} must be (lo, hi) with 0 < lo <= hi")
        if not (0.0 <= flip_prob <= 1.0 and 0.0 <= erase_prob <= 1.0):
            raise ValueError("flip_prob / erase_prob must be in [0, 1]")
        self.scale, self.ratio = tuple(map(float, scale)), tuple(map(float, ratio))
        self.erase_scale, self.erase_ratio = tuple(map(float, erase_scale)), tuple(map(float, erase_ratio))
        self.flip_prob, self.erase_prob = float(flip_prob), float(erase_prob)
        self.seed, self.rank = int(seed), int(rank)
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else "cpu"
        self.device = torch.device(device)
        self._dev = {}     # N -> persistent int32 [9 * N] device buffer
        self._stage = {}   # N -> ring of (pinned int32 [9 * N], event of its last copy)
        self._turn = 0
        self._center = {}  # (N, Hs, Ws, crop_pct) -> GeoParams

    # ------------------------------------------------------------------ host draw
    def host_params(self, step, N, Hs, Ws):
        """(crop int32 [N, 4], flip int32 [N], erase int32 [N, 4]) as numpy arrays: a pure function
        of (seed, rank, step).  Every variate is drawn on every call, in a fixed order, whatever the
        settings use of them."""
        Ho, Wo = self.size
        rng = np.random.default_rng(np.random.SeedSequence([self.seed, self.rank, int(step), TAG]))
        u_area, u_logr = rng.random((N, _TRIES)), rng.random((N, _TRIES))
        u_top, u_left, u_flip = rng.random(N), rng.random(N), rng.random(N)
        u_erase, e_area, e_logr = rng.random(N), rng.random((N, _TRIES)), rng.random((N, _TRIES))
        e_top, e_left = rng.random(N), rng.random(N)

        def sides(u_a, u_r, area, scale, ratio):  # (sqrt(area * aspect), sqrt(area / aspect)), rounded
            a = area * (scale[0] + (scale[1] - scale[0]) * u_a)
            r = np.exp(math.log(ratio[0]) + (math.log(ratio[1]) - math.log(ratio[0])) * u_r)
            return np.rint(np.sqrt(a * r)).astype(np.int64), np.rint(np.sqrt(a / r)).astype(np.int64)

        rows = np.arange(N)
        w, h = sides(u_area, u_logr, Hs * Ws, self.scale, self.ratio)
        k, found = _first_true((w > 0) & (w <= Ws) & (h > 0) & (h <= Hs))
        h, w = h[rows, k], w[rows, k]
        top = np.minimum(np.floor(u_top * (Hs - h + 1)).astype(np.int64), Hs - h)
        left = np.minimum(np.floor(u_left * (Ws - w + 1)).astype(np.int64), Ws - w)
        crop = np.where(found[:, None], np.stack([top, left, h, w], 1), np.array(fallback_crop(Hs, Ws, self.ratio)))

        eh, ew = sides(e_area, e_logr, Ho * Wo, self.erase_scale, self.erase_ratio)
        k, found = _first_true((eh < Ho) & (ew < Wo))
        eh, ew = eh[rows, k], ew[rows, k]
        y0 = np.minimum(np.floor(e_top * (Ho - eh + 1)).astype(np.int64), Ho - eh)
        x0 = np.minimum(np.floor(e_left * (Wo - ew + 1)).astype(np.int64), Wo - ew)
        on = found & (u_erase < self.erase_prob)
        erase = np.where(on[:, None], np.stack([y0, y0 + eh, x0, x0 + ew], 1), 0)
        return crop.astype(np.int32), (u_flip < self.flip_prob).astype(np.int32), erase.astype(np.int32)

    # ------------------------------------------------------------------ device side
    def upload(self, crop, flip, erase, Hs, Ws):
        """Pack host parameters and send them with one non-blocking copy into the persistent device
        tensors of this batch size.  A crop box outside the ``Hs`` x ``Ws`` source or an erase box
        outside the output raises here: on the device it would silently be clipped."""
        crop, flip, erase = np.asarray(crop, np.int32), np.asarray(flip, np.int32), np.asarray(erase, np.int32)
        N = flip.shape[0]
        Ho, Wo = self.size
        if crop.shape != (N, 4) or flip.shape != (N,) or erase.shape != (N, 4):
            raise ValueError(f"expected crop [{N}, 4], flip [{N}] and erase [{N}, 4]")
        c = crop.astype(np.int64)
        if N and not ((c[:, 0] >= 0) & (c[:, 1] >= 0) & (c[:, 2] >= 1) & (c[:, 3] >= 1)
                      & (c[:, 0] + c[:, 2] <= Hs) & (c[:, 1] + c[:, 3] <= Ws)).all():
            raise ValueError(f"crop box outside the {Hs} x {Ws} source")
        if N and not ((erase[:, 0] >= 0) & (erase[:, 0] <= erase[:, 1]) & (erase[:, 1] <= Ho)
                      & (erase[:, 2] >= 0) & (erase[:, 2] <= erase[:, 3]) & (erase[:, 3] <= Wo)).all():
            raise ValueError(f"erase box outside the {Ho} x {Wo} output")
        if self.device.type != "cuda":
            buf = torch.empty(9 * N, dtype=torch.int32)
            self._pack(buf, crop, flip, erase, N)
            return self._views(buf, N)
        if N not in self._dev:
            self._dev[N] = torch.empty(9 * N, dtype=torch.int32, device=self.device)
            self._stage[N] = [(torch.empty(9 * N, dtype=torch.int32).pin_memory(), torch.cuda.Event())
                              for _ in range(_RING)]
        self._turn = (self._turn + 1) % _RING
        host, ev = self._stage[N][self._turn]
        # the copy issued _RING uploads ago from this buffer has long completed, so nothing waits here;
        # the guard only keeps the buffer from being rewritten under a copy that is still in flight
        if not ev.query():
            ev.synchronize()
        self._pack(host, crop, flip, erase, N)
        self._dev[N].copy_(host, non_blocking=True)
        ev.record(torch.cuda.current_stream(self.device))
        return self._views(self._dev[N], N)

    @staticmethod
    def _pack(buf, crop, flip, erase, N):
        a = buf.numpy()
        a[:4 * N] = crop.reshape(-1)
        a[4 * N:5 * N] = flip
        a[5 * N:] = erase.reshape(-1)

    @staticmethod
    def _views(buf, N):
        return GeoParams(buf[:4 * N].view(N, 4), buf[4 * N:5 * N], buf[5 * N:].view(N, 4))

    def params(self, step, N, Hs, Ws):
        """``GeoParams`` of this step on the cropper's device (views of one persistent buffer per
        batch size: valid until the next call with the same N)."""
        return self.upload(*self.host_params(step, N, Hs, Ws), Hs, Ws)

    # ------------------------------------------------------------------ evaluation
    def center_box(self, Hs, Ws, crop_pct=1.0):
        """(top, left, height, width) of the evaluation crop: the largest central box with the
        output's aspect ratio, scaled by ``crop_pct`` (for a square output, the central square of
        side ``max(1, round(crop_pct * min(Hs, Ws)))``)."""
        Ho, Wo = self.size
        if Ws * Ho >= Wo * Hs:  # the source is the wider one: full height
            bh, bw = float(Hs), Hs * Wo / Ho
        else:
            bh, bw = Ws * Ho / Wo, float(Ws)
        bh = min(max(1, int(round(crop_pct * bh))), Hs)
        bw = min(max(1, int(round(crop_pct * bw))), Ws)
        return (Hs - bh) // 2, (Ws - bw) // 2, bh, bw

    def center_params(self, N, Hs, Ws, crop_pct=1.0):
        """The evaluation transform: every image takes ``center_box``, no flip, no erase.  It is
        ``Resize(size / crop_pct)`` followed by ``CenterCrop(size)`` done in one resample: that pair
        scales the short side to ``size / crop_pct`` and keeps the central ``size``, the fraction
        ``crop_pct`` of the short side, which is this box in source pixels (rounded to whole source
        pixels here, to whole resized pixels there), sampled without antialiasing.  Cached per
        ``(N, Hs, Ws, crop_pct)``: separate device tensors, not the buffer ``params`` rewrites."""
        key = (int(N), int(Hs), int(Ws), float(crop_pct))
        if key not in self._center:
            if not 0 < crop_pct <= 1:
                raise ValueError("crop_pct must be in (0, 1]")
            buf = torch.zeros(9 * N, dtype=torch.int32)
            buf[:4 * N].view(N, 4)[:] = torch.tensor(self.center_box(Hs, Ws, crop_pct), dtype=torch.int32)
            self._center[key] = self._views(buf.to(self.device), N)
        return self._center[key]
