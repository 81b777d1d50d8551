"""Shared by test_adamw_cpu.py and test_adamw_gpu.py: the fp64 AdamW reference, the stock fp32
yardstick and the accuracy rule.

Accuracy rule: the reference is ``torch.optim.AdamW`` on double copies (two param groups: decay /
no decay; ``clip_grad_norm_`` before the step).  The yardstick is stock fp32 ``torch.optim.AdamW``'s
own max error against that fp64 run on the same inputs.  The native result must be within
2 x the yardstick + one fp32 ulp of the largest parameter magnitude (the margin covers FMA
contraction and division ordering)."""
import math

import torch


def ulp32(x: float) -> float:
    """spacing of fp32 numbers at magnitude ``x``"""
    x = abs(float(x))
    if x == 0.0 or not math.isfinite(x):
        return 2.0 ** -149
    return 2.0 ** (max(math.floor(math.log2(x)), -126) - 23)


class RefAdamW:
    """torch.optim.AdamW over a flat vector split into a decay and a no-decay parameter, in
    ``dtype`` on the host; gradients are handed in per step."""

    def __init__(self, p0, decay_mask, dtype, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None):
        p0 = p0.detach().cpu().reshape(-1)
        self.mask = (torch.ones(p0.numel(), dtype=torch.bool) if decay_mask is None
                     else decay_mask.detach().cpu().reshape(-1).bool())
        self.dtype, self.max_norm = dtype, max_norm
        self.pd = p0[self.mask].to(dtype).clone().requires_grad_()
        self.pn = p0[~self.mask].to(dtype).clone().requires_grad_()
        groups = [dict(params=[self.pd], weight_decay=weight_decay), dict(params=[self.pn], weight_decay=0.0)]
        self.opt = torch.optim.AdamW([g for g in groups if g["params"][0].numel()], lr=lr, betas=betas, eps=eps)
        self.params = [g["params"][0] for g in self.opt.param_groups]

    def set_lr(self, lr):
        for g in self.opt.param_groups:
            g["lr"] = lr

    def step(self, grad, grad_scale=1.0):
        """``grad``: the flat fp32 gradient the native optimizer saw; returns the pre-clip norm"""
        g = grad.detach().cpu().reshape(-1).to(self.dtype) * grad_scale
        self.pd.grad, self.pn.grad = g[self.mask], g[~self.mask]
        norm = None
        if self.max_norm is not None:
            norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm)
        self.opt.step()
        return norm

    def flat(self):
        out = torch.empty(self.mask.numel(), dtype=self.dtype)
        out[self.mask] = self.pd.detach()
        out[~self.mask] = self.pn.detach()
        return out


def ref_pair(p0, decay_mask, **kw):
    """(fp64 reference, stock fp32 yardstick) from the same start"""
    return RefAdamW(p0, decay_mask, torch.float64, **kw), RefAdamW(p0, decay_mask, torch.float32, **kw)


def check_accuracy(native, stock, ref64, what=""):
    """the accuracy rule; all three are tensors of one shape"""
    ref64 = ref64.detach().cpu().double().reshape(-1)
    e_native = float((native.detach().cpu().double().reshape(-1) - ref64).abs().max())
    e_stock = float((stock.detach().cpu().double().reshape(-1) - ref64).abs().max())
    bound = 2.0 * e_stock + ulp32(float(ref64.abs().max()))
    print(f"{what}: native err {e_native:.3e}, stock fp32 err {e_stock:.3e}, bound {bound:.3e}")
    assert e_native <= bound, (f"{what}: native max error vs fp64 {e_native:.3e} > bound {bound:.3e} "
                               f"(stock fp32 max error {e_stock:.3e})")
    return e_native, e_stock


def decay_mask_of(opt):
    """per-element decay mask of a FlatAdamW's whole flat buffer"""
    return opt.decay_map.cpu().bool().repeat_interleave(64)
