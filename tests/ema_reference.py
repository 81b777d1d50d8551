"""The reference and the accuracy rule of the FlatEMA tests (test_ema_cpu.py, test_ema_gpu.py).

Reference: a per-tensor fp64 recursion with the formulas of csrc/kernels/ema.hip,

    c += 1
    if c % every != 0:   skip
    else:  d_t = decay                                    without warm-up
               = min(decay, (1 + n) / (warmup + n))       with warm-up
           w = 1 - d_t ;  n += 1 ;  ema += w * (p - ema)

fed with fp64 copies of the engine's OWN master weights after each step, so the check is
independent of the training numerics.

Accuracy rule: after ``k`` updates

    |ema_fp32 - ema_fp64| <= 8 * k * 2^-24 * M

with ``M`` the largest magnitude any ``p`` or ``ema`` element of that tensor took.  Derivation:
one update commits at most three roundings of values no larger than ``2 M`` (the difference ``p - ema``, the
product ``w * (p - ema)`` on the host path -- the device's fused multiply-add does not round it --
and the sum), each at most ``2^-24 * 2 M``; rounding ``w`` to fp32 moves the product by at most
one more term of that size; ``w <= 1`` and the recursion is a convex combination, so an earlier
error is never amplified.  One update therefore adds at most about ``7 * 2^-24 * M`` and the
rule leaves a little slack.  Measured on the host: the unfused fp32 path over 40 updates of
200,003 normal values (``decay=0.999, warmup=10``) stays below ``2.1 * k * 2^-24 * M``, the worst
at the first update, where ``w = 0.9``; the device's fused path stays below ``1.7 * k * 2^-24 *
M`` over all of test_ema_gpu.py.  A correct implementation passes with a margin, while a wrong weight, a
wrong counter or a missed element misses the rule by orders of magnitude.

The prep scalars are checked on their own: ``state[2]`` (w) and ``state[4]`` (d_t) within 2 fp64
ulps of ``host_scalars``, the counters ``state[0]`` and ``state[1]`` exactly.
"""
import math

import torch


def host_scalars(c, n, decay, warmup, every):
    """one call of the prep formula in host fp64: (c, n, w, d_t or None when the call skips)"""
    c += 1
    if c % every != 0:
        return c, n, 0.0, None
    d = float(decay)
    if warmup is not None and warmup > 0:
        d = min(d, (1.0 + n) / (float(warmup) + n))
    return c, n + 1, 1.0 - d, d


class RefEMA:
    """fp64 recursion over a list of tensors (one flat buffer counts as one tensor)"""

    def __init__(self, tensors, decay, warmup=None, every=1):
        self.ema = [t.detach().double().cpu().clone() for t in tensors]
        self.decay, self.warmup, self.every = decay, warmup, every
        self.c = self.n = 0
        self.w = 0.0
        self.d = None  # d_t of the last call that updated
        self.M = [float(e.abs().max()) if e.numel() else 0.0 for e in self.ema]  # per tensor

    def update(self, tensors):
        self.c, self.n, self.w, d = host_scalars(self.c, self.n, self.decay, self.warmup, self.every)
        ps = [t.detach().double().cpu() for t in tensors]
        self.M = [max(m, float(p.abs().max())) if p.numel() else m for m, p in zip(self.M, ps)]
        if d is None:
            return
        self.d = d
        for e, p in zip(self.ema, ps):
            e.add_(self.w * (p - e))

    def bound(self, index=0):
        return 8.0 * self.n * 2.0 ** -24 * self.M[index]


def check_rule(got, ref: RefEMA, what, index=0):
    """``got`` (fp32) against ``ref.ema[index]`` under the rule; returns the largest error"""
    g = got.detach().double().cpu().reshape(-1)
    want = ref.ema[index].reshape(-1)
    assert g.shape == want.shape, (what, g.shape, want.shape)
    err = float((g - want).abs().max()) if g.numel() else 0.0
    bound, M = ref.bound(index), ref.M[index]
    print(f"{what}: max |fp32 - fp64| {err:.3e}, bound {bound:.3e} (k = {ref.n}, M = {M:.3e})")
    assert err <= bound, f"{what}: error {err:.3e} exceeds 8 k 2^-24 M = {bound:.3e} (k = {ref.n}, M = {M:.3e})"
    return err


def ulp64(x):
    return math.ulp(abs(float(x)))


def check_scalars(state, ref: RefEMA, what):
    """the device state block against the host formula: counters exact, w and d_t within 2 ulps"""
    st = state.detach().cpu().tolist()
    assert st[0] == ref.c and st[1] == ref.n, f"{what}: counters {st[0]}, {st[1]} != {ref.c}, {ref.n}"
    assert abs(st[2] - ref.w) <= 2 * ulp64(ref.w), f"{what}: w {st[2]!r} != {ref.w!r}"
    if ref.d is not None:
        assert abs(st[4] - ref.d) <= 2 * ulp64(ref.d), f"{what}: d_t {st[4]!r} != {ref.d!r}"
    assert st[3] == float(ref.decay), f"{what}: decay {st[3]!r} != {ref.decay!r}"
