"""fp64 numpy reference of ``ops.augment_resized`` and the cases both test files run.

Written independently of the op's host path: the box is cut out by slicing, resampled one axis
after the other with weights (1 - lambda, lambda), flipped afterwards, normalized by dividing by
std, erased, then mixed with the fp32 value of lam.  Coordinates are the issue's integers:
    num = max((2 * o + 1) * len - n_out, 0); i0 = num // (2 * n_out);
    lambda = (num % (2 * n_out)) / (2 * n_out); i1 = min(i0 + 1, len - 1)

Accuracy rule of the GPU output: |out - ref| <= 2^-8 |ref| + 1e-5.  The first term is one correct
bf16 rounding (unit roundoff 2^-8); the second covers the fp32 blend and normalisation (about 2e-6
for std >= 0.05), including the case where that error moves a value across a rounding boundary.  The
fp32 host path has no bf16 term: |out - ref| <= 1e-5.
"""
import functools

import numpy as np

MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
BF16_U, ABS_TOL = 2.0 ** -8, 1e-5


def _axis(n_out, length):
    o = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * o + 1) * length - n_out, 0)
    i0 = num // (2 * n_out)
    return i0, np.minimum(i0 + 1, length - 1), (num % (2 * n_out)) / float(2 * n_out)


def resample(u8, size, cout, mean, std, crop, flip, erase):
    """fp64 [N, cout, Ho, Wo] of valid (unclipped) parameters."""
    N, _, _, C = u8.shape
    Ho, Wo = size
    mean, std = np.asarray(mean[:C], np.float64), np.asarray(std[:C], np.float64)
    out = np.zeros((N, cout, Ho, Wo), np.float64)
    for m in range(N):
        top, left, h, w = (int(v) for v in crop[m])
        box = u8[m, top:top + h, left:left + w].astype(np.float64)
        assert box.shape[:2] == (h, w) and h >= 1 and w >= 1
        y0, y1, ly = _axis(Ho, h)
        x0, x1, lx = _axis(Wo, w)
        rows = box[y0] * (1 - ly)[:, None, None] + box[y1] * ly[:, None, None]
        v = rows[:, x0] * (1 - lx)[None, :, None] + rows[:, x1] * lx[None, :, None]
        if flip[m]:
            v = v[:, ::-1]
        v = (v / 255.0 - mean) / std
        ey0, ey1, ex0, ex1 = (int(e) for e in erase[m])
        v[max(ey0, 0):max(min(ey1, Ho), 0), max(ex0, 0):max(min(ex1, Wo), 0)] = 0.0
        out[m, :C] = v.transpose(2, 0, 1)
    return out


def mix(x, labels, partner, lam, box):
    """Mixup / CutMix on resampled values: (x, y_a, y_b, lam_out fp32)."""
    N, _, H, W = x.shape
    out, ya, yb = x.copy(), np.asarray(labels).copy(), np.asarray(labels).copy()
    lam_out = np.ones(N, np.float32)
    for n in range(N):
        p = int(partner[n])
        if not 0 <= p < N:
            continue
        yb[n] = labels[p]
        y0, y1 = max(int(box[n][0]), 0), min(int(box[n][1]), H)
        x0, x1 = max(int(box[n][2]), 0), min(int(box[n][3]), W)
        if y1 > y0 and x1 > x0:
            out[n, :, y0:y1, x0:x1] = x[p, :, y0:y1, x0:x1]
            lam_out[n] = np.float32(1.0) - np.float32((y1 - y0) * (x1 - x0)) / np.float32(H * W)
        else:
            la = float(np.float32(lam[n]))
            out[n] = la * x[n] + (1.0 - la) * x[p]
            lam_out[n] = np.float32(lam[n])
    return out, ya, yb, lam_out


def excess(out, ref, rel=BF16_U):
    """max of |out - ref| - (rel |ref| + 1e-5): the rule holds when this is <= 0."""
    out, ref = np.asarray(out, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(out - ref) - (rel * np.abs(ref) + ABS_TOL)).max())


# ------------------------------------------------------------------------------------- cases
SHAPES = [((9, 7), (5, 11)),       # down one axis, up the other; fewer than 256 output pixels
          ((32, 32), (40, 24)),    # more than one block plus a tail
          ((37, 53), (16, 24)),
          ((32, 32), (224, 224))]  # the workload's own ratio
CHANNELS = [(3, 8), (3, 3), (1, 1)]
CASE_IDS = [(s, c, f) for s in range(len(SHAPES)) for c in range(len(CHANNELS)) for f in (0, 1)]
N = 5


@functools.lru_cache(maxsize=None)
def case(s, c, f):
    """(u8, size, C, Cout, crop, flip, erase, ref): five images -- the full image, a 1 x 1 box, a
    box touching the bottom-right corner (the i1 clamp), two random interior boxes -- with flips
    0 1 0 1 1 (f = 0) or the opposite (f = 1).  Computed once per process; do not modify."""
    (Hs, Ws), size = SHAPES[s]
    C, cout = CHANNELS[c]
    rng = np.random.default_rng(1000 * s + 10 * c + f)
    u8 = rng.integers(0, 256, (N, Hs, Ws, C), dtype=np.uint8)
    crop = np.zeros((N, 4), np.int32)
    crop[0] = (0, 0, Hs, Ws)
    crop[1] = (rng.integers(0, Hs), rng.integers(0, Ws), 1, 1)
    h, w = int(rng.integers(2, Hs)), int(rng.integers(2, Ws))
    crop[2] = (Hs - h, Ws - w, h, w)
    for m in (3, 4):
        h, w = int(rng.integers(2, Hs - 1)), int(rng.integers(2, Ws - 1))
        crop[m] = (rng.integers(1, Hs - h), rng.integers(1, Ws - w), h, w)
    flip = np.array([0, 1, 0, 1, 1], np.int32) ^ f
    erase = np.zeros((N, 4), np.int32)
    ref = resample(u8, size, cout, MEAN, STD, crop, flip, erase)
    for a in (u8, crop, flip, erase, ref):
        a.setflags(write=False)
    return u8, size, C, cout, crop, flip, erase, ref
