"""Shared by test_layerwise_cpu.py and test_layerwise_gpu.py: per-tensor LARS and LAMB written
straight from the formulas in mi355x_dp/parallel/optim.py's docstring (torch ships neither), run
on the host in a chosen dtype and fed the flat gradient the native optimizer saw.

The accuracy rule is adamw_reference.check_accuracy: the native error against the fp64 run of
this reference must be at most 2 x the error of its fp32 run + one fp32 ulp of the largest
parameter.  The fp32 run does everything in fp32, norms included (``torch.linalg.vector_norm`` of
the fp32 tensor), like a per-tensor implementation on stock ops would."""
import torch

from adamw_reference import check_accuracy, ulp32  # noqa: F401  (re-exported for the tests)

LARS = dict(lr=0.5, momentum=0.9, weight_decay=1e-4, trust_coefficient=1e-3, eps=1e-8)
LAMB = dict(lr=2e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01)


class _Ref:
    """``layout``: (lo, hi, excluded) of every parameter in the flat vector; elements outside every
    parameter (alignment padding) are never touched"""

    def __init__(self, p0, layout, dtype):
        self.dtype = dtype
        self.layout = [(int(lo), int(hi), bool(ex)) for lo, hi, ex in layout]
        self.p = p0.detach().cpu().reshape(-1).to(dtype).clone()
        self.q = [1.0] * len(self.layout)

    def set_lr(self, lr):
        self.lr = lr

    def flat(self):
        return self.p.clone()

    def _norm(self, t):
        return torch.linalg.vector_norm(t)


class RefLARS(_Ref):
    def __init__(self, p0, layout, dtype, lr, momentum=0.9, weight_decay=0.0, trust_coefficient=1e-3, eps=1e-8):
        super().__init__(p0, layout, dtype)
        self.lr, self.momentum, self.wd, self.tc, self.eps = lr, momentum, weight_decay, trust_coefficient, eps
        self.buf = torch.zeros_like(self.p)

    def step(self, grad, grad_scale=1.0):
        g_all = grad.detach().cpu().reshape(-1).to(self.dtype) * grad_scale
        for i, (lo, hi, ex) in enumerate(self.layout):
            w, g = self.p[lo:hi], g_all[lo:hi]
            if ex:
                d, self.q[i] = g, 1.0
            else:
                wn, gn = self._norm(w), self._norm(g)
                q = torch.ones((), dtype=self.dtype)
                if wn > 0 and gn > 0:
                    q = self.tc * wn / (gn + self.wd * wn + self.eps)
                d, self.q[i] = q * (g + self.wd * w), float(q)
            self.buf[lo:hi] = self.momentum * self.buf[lo:hi] + d
            self.p[lo:hi] = w - self.lr * self.buf[lo:hi]


class RefLAMB(_Ref):
    def __init__(self, p0, layout, dtype, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, max_norm=None):
        super().__init__(p0, layout, dtype)
        self.lr, self.betas, self.eps, self.wd, self.max_norm = lr, betas, eps, weight_decay, max_norm
        self.m, self.v, self.t = torch.zeros_like(self.p), torch.zeros_like(self.p), 0

    def step(self, grad, grad_scale=1.0):
        """returns the pre-clip global gradient norm (None without ``max_norm``)"""
        g_all = grad.detach().cpu().reshape(-1).to(self.dtype) * grad_scale
        total = None
        if self.max_norm is not None:
            total = self._norm(torch.cat([g_all[lo:hi] for lo, hi, _ in self.layout]))
            g_all = g_all * torch.clamp(self.max_norm / (total + 1e-6), max=1.0)
        self.t += 1
        b1, b2 = self.betas
        bc1, bc2 = 1.0 - b1 ** self.t, 1.0 - b2 ** self.t
        for i, (lo, hi, ex) in enumerate(self.layout):
            w, g = self.p[lo:hi], g_all[lo:hi]
            m = self.m[lo:hi] = b1 * self.m[lo:hi] + (1.0 - b1) * g
            v = self.v[lo:hi] = b2 * self.v[lo:hi] + (1.0 - b2) * g * g
            r = (m / bc1) / ((v / bc2).sqrt() + self.eps)
            if ex:
                u, q = r, torch.ones((), dtype=self.dtype)
            else:
                u = r + self.wd * w
                wn, un = self._norm(w), self._norm(u)
                q = wn / un if (wn > 0 and un > 0) else torch.ones((), dtype=self.dtype)
            self.q[i] = float(q)
            self.p[lo:hi] = w - self.lr * q * u
        return total


def ref_pair(kind, p0, layout, **kw):
    """(fp64 reference, fp32 yardstick) from the same start; ``kind``: "lars" or "lamb" """
    cls = RefLARS if kind == "lars" else RefLAMB
    return cls(p0, layout, torch.float64, **kw), cls(p0, layout, torch.float32, **kw)


def layout_of(opt):
    """(lo, hi, excluded) of every parameter of a FlatLARS / FlatLAMB's flat buffer"""
    f = opt.engine.flat
    ex = opt.excluded.cpu().tolist()
    return [(o, o + p.numel(), bool(e)) for p, o, e in zip(f.params, f.offsets, ex)]
