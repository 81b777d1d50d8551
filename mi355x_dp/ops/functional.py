"""Autograd functions over the native gfx950 kernels.

Device contract (GPU path): activations are bf16 tensors in ``channels_last``
memory format (NHWC storage), conv weights are read as bf16 ``[K][R][S][C]``
(= channels_last storage of a ``[K, C, R, S]`` tensor), accumulation is fp32.
Host tensors take the fp32 PyTorch reference path (used by the CPU tests and
the gloo CPU configuration) -- the two paths are selected by device, never by
availability: a CUDA tensor without the native library is an error.

Gradient sinks: a parameter registered with a flat-buffer engine
(``mi355x_dp.parallel.flat``) carries ``_mi_flat = True``; its ``.grad`` is a
view into the engine's fp32 gradient buffer and our backward kernels
accumulate straight into it (split-K atomics / ``+=``), then signal the engine
via ``_mi_on_grad_ready`` so the bucket all-reduce can start while backward
continues.  Any other parameter gets a freshly allocated gradient returned
through autograd as usual (works with stock ``torch.nn.parallel.DDP``).
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import NamedTuple

import torch
import torch.nn.functional as F

from . import _lib
from . import kernels as _k  # noqa: F401  (registers signatures)
from ._lib import ptr, stream_of

CL = torch.channels_last
BF16 = torch.bfloat16


# --------------------------------------------------------------------- helpers
def _nhwc(x: torch.Tensor) -> torch.Tensor:
    if x.dtype != BF16:
        x = x.to(BF16)
    if x.dim() == 4 and not x.is_contiguous(memory_format=CL):
        x = x.contiguous(memory_format=CL)
    return x


def weight_bf16(w: torch.Tensor) -> torch.Tensor:
    """bf16 compute copy of a parameter in kernel layout (flat-engine shadow if present)."""
    w16 = getattr(w, "_mi_bf16", None)
    if w16 is not None:
        return w16
    with torch.no_grad():
        if w.dim() == 4:
            return w.detach().to(BF16).contiguous(memory_format=CL)
        return w.detach().to(BF16).contiguous()


def weight_bf16_t(w: torch.Tensor) -> torch.Tensor:
    """Conv-dgrad operand [C][R][S][K] (bf16) of a [K, C, R, S] conv weight: the flat engine's
    transposed copy (refreshed once per optimizer step for every conv) or a fresh transpose."""
    wt = getattr(w, "_mi_bf16_t", None)
    if wt is not None:
        return wt
    K, C, R, S = w.shape
    w16 = weight_bf16(w)
    wt = torch.empty((C, R, S, K), dtype=BF16, device=w.device)
    _lib.call("mi_conv_wtrans", ptr(w16), ptr(wt), K, R * S, C, stream_of(w16))
    return wt


def linear_weight_t(w: torch.Tensor) -> torch.Tensor:
    """Linear data-gradient operand W^T [in][out] (bf16): the flat engine's cached transpose
    (refreshed once per optimizer step) or a fresh one."""
    wt = getattr(w, "_mi_bf16_t", None)
    if wt is not None and wt.dim() == 2:
        return wt
    return weight_bf16(w).t().contiguous()


def _flat(p) -> bool:
    return p is not None and getattr(p, "_mi_flat", False) and p.grad is not None


def _grad_buffer(p: torch.Tensor) -> torch.Tensor:
    """fp32 gradient target in kernel layout: the engine's view, or a fresh zero tensor."""
    if _flat(p):
        return p.grad
    if p.dim() == 4:
        return torch.zeros_like(p, dtype=torch.float32, memory_format=CL)
    return torch.zeros_like(p, dtype=torch.float32)


class WgradStream:
    """Weight gradients on a side HIP stream (owned by the flat-buffer engine, one per device).

    A conv's weight gradient is needed by nothing but the optimizer, while its data gradient is
    the critical path of backward; on one stream every kernel's tail (its last, partly filled
    wave of workgroups) and every small split-K reduce / BN finalize idles most of the 256 CUs.
    With the weight gradients on their own stream the two chains overlap and fill each other's
    tails.  Ordering rules (no host synchronisation anywhere):

    * ``run``: the side stream waits for the compute stream (the kernel's operands were produced
      there), the weight-gradient kernels run on it, their operands are ``record_stream``-ed so
      the caching allocator does not recycle them early, and the parameter is marked ready ON
      the side stream -- so a bucket's collective (which waits on the current stream) waits for
      the side stream, which itself has waited for everything the compute stream did before;
    * marks of gradients produced on the compute stream (BN affine) while side work is pending
      are deferred and issued on the side stream at its next ``run`` (or ``join``), for the same
      reason: a bucket may mix both kinds;
    * ``join`` (engine: before the optimizer / reducer finish, at forward, at zero_grad) makes
      the compute stream wait for the side stream.
    Disabled inside HIP graph capture (the captured step stays single-stream)."""

    _streams = {}  # device index -> the side stream (shared by every engine on that device)

    def __init__(self, device):
        self.device = torch.device(device)
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        if idx not in WgradStream._streams:
            # MI355X_DP_WGRAD_PRIORITY=-1: the side stream's workgroups are dispatched ahead of the
            # compute stream's (default 0: equal priority; profiles/rn50_bs256_wgrad_stream.md)
            with torch.cuda.device(idx):
                cus = int(os.environ.get("MI355X_DP_WGRAD_CUS", "0"))
                if cus > 0:
                    # A/B knob: the side stream confined to `cus` CUs (spread over the CU ids; the
                    # compute stream keeps every CU), MI355X_DP_WGRAD_CU_BLOCK=1: the first `cus` ids
                    h = ctypes.c_void_p()
                    _lib.call("mi_create_cu_masked_stream", cus, int(os.environ.get("MI355X_DP_WGRAD_CU_BLOCK", "0")
                                                                      != "1"), ctypes.addressof(h))
                    st = torch.cuda.ExternalStream(h.value, device=self.device)
                else:
                    st = torch.cuda.Stream(device=self.device,
                                           priority=int(os.environ.get("MI355X_DP_WGRAD_PRIORITY", "0")))
                # its own split-K slab workspace (gemm_conv.hip)
                _lib.call("mi_register_wgrad_stream", ctypes.c_void_p(st.cuda_stream))
            WgradStream._streams[idx] = st
        self.stream = WgradStream._streams[idx]
        self.dirty = False
        self.deferred = []
        self.runs = 0

    # > 0 while a GraphedStep warms up / captures: the captured step is single-stream, and its
    # warm-up must run the same kernels on the same stream so the native library's lazily sized
    # workspaces exist before capture (no allocation may happen inside it)
    suspended = 0

    def active(self) -> bool:
        return WgradStream.suspended == 0 and not torch.cuda.is_current_stream_capturing()

    def run(self, fn, tensors=(), cb=None):
        main = torch.cuda.current_stream(self.device)
        self.stream.wait_stream(main)
        with torch.cuda.stream(self.stream):
            out = fn()
            for t in tensors:
                if t is not None:
                    t.record_stream(self.stream)
            self.dirty = True
            self.runs += 1
            self._flush_locked()
            if cb is not None:
                cb()
        return out

    def _flush_locked(self):
        pending, self.deferred = self.deferred, []
        for d in pending:
            d()

    def mark(self, cb):
        if self.dirty:
            self.deferred.append(cb)
        else:
            cb()

    def join(self):
        if self.deferred:
            self.stream.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(self.stream):
                self._flush_locked()
        if self.dirty:
            torch.cuda.current_stream(self.device).wait_stream(self.stream)
            self.dirty = False


def _side(p):
    """the engine's weight-gradient stream for parameter p, if it should be used now"""
    s = getattr(p, "_mi_side", None)
    if s is None or not _flat(p) or not s.active():
        return None
    return s


def _finish_grad(p: torch.Tensor, g: torch.Tensor):
    """Return value for autograd: None if accumulated in place (flat engine)."""
    if _flat(p):
        cb = getattr(p, "_mi_on_grad_ready", None)
        if cb is not None:
            s = getattr(p, "_mi_side", None)
            if s is not None:
                s.mark(cb)
            else:
                cb()
        return None
    return g.to(p.dtype) if g.dtype != p.dtype else g


def run_wgrad(p: torch.Tensor, fn, tensors=()):
    """Run ``fn`` (which writes p's fp32 gradient into the flat buffer) on the engine's weight-
    gradient stream when there is one, else inline; then signal the engine (see WgradStream)."""
    s = _side(p)
    if s is None:
        fn()
        return
    s.run(fn, tensors, getattr(p, "_mi_on_grad_ready", None))


def _conv_out(h, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1


# ======================================================================= conv
def pad_channels8(x: torch.Tensor) -> torch.Tensor:
    """[N, C<=8, H, W] -> bf16 channels_last [N, 8, H, W] (zero channels appended): one 16-byte
    chunk per pixel, the layout the small-channel (stem) conv mode of the MFMA kernel gathers."""
    N, C, H, W = x.shape
    out = torch.empty((N, 8, H, W), dtype=BF16, device=x.device, memory_format=CL)
    out[:, C:].zero_()
    out[:, :C].copy_(x)
    return out


class _Conv2d(torch.autograd.Function):
    """Implicit-GEMM convolution.  Paths (chosen by channel count, all MFMA):
      direct : C % 64 == 0                      (every ResNet conv but the stem)
      c8     : C <= 8, input padded to 8 channels (the 7x7 stem: one 16-B chunk = one tap)
      col    : other C (explicit im2col + GEMM)"""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, stats):
        N, C, H, W = x.shape
        K, Cw, R, S = weight.shape
        P, Q = _conv_out(H, R, stride, padding), _conv_out(W, S, stride, padding)
        w16 = weight_bf16(weight)
        if C <= 8 and C % 64 != 0:
            if C != 8:
                x = pad_channels8(x)
                C = 8
            mode = "c8"
        elif C % 64 == 0:
            mode = "direct"
        else:
            mode = "col"
        x = _nhwc(x)
        st = stream_of(x)
        y = torch.empty((N, K, P, Q), dtype=BF16, device=x.device, memory_format=CL)
        saved = x
        if mode == "direct":
            _lib.call("mi_conv2d_fwd", ptr(x), ptr(w16), ptr(y), ptr(None), ptr(stats), N, H, W, C, K, R, S,
                      stride, padding, P, Q, 0, st)
        elif mode == "c8":
            wp = torch.zeros((K, R, S, 8), dtype=BF16, device=x.device)
            wp[..., :Cw].copy_(w16.permute(0, 2, 3, 1))
            _lib.call("mi_conv2d_fwd", ptr(x), ptr(wp), ptr(y), ptr(None), ptr(stats), N, H, W, 8, K, R, S,
                      stride, padding, P, Q, 0, st)
        else:
            # explicit im2col (k = (r*S+s)*C + c) + MFMA GEMM
            Kr = R * S * C
            Kp = (Kr + 7) // 8 * 8
            col = torch.empty((N * P * Q, Kp), dtype=BF16, device=x.device)
            _lib.call("mi_im2col", ptr(x), ptr(col), N, H, W, C, R, S, stride, padding, P, Q, Kp, st)
            wp = torch.zeros((K, Kp), dtype=BF16, device=x.device)
            wp[:, :Kr].copy_(w16.permute(0, 2, 3, 1).reshape(K, Kr))
            _lib.call("mi_gemm_nt", ptr(col), ptr(wp), ptr(y), ptr(None), ptr(stats), N * P * Q, K, Kp, Kp, Kp, K,
                      0, 0, st)
            saved = col
        if bias is not None:
            y = y + bias.to(BF16).view(1, K, 1, 1)
        ctx.geom = (N, C, H, W, K, Cw, R, S, stride, padding, P, Q)
        ctx.has_bias = bias is not None
        ctx.bias_param = bias
        ctx.mode = mode
        ctx.save_for_backward(saved, weight, w16)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W, K, Cw, R, S, stride, padding, P, Q = ctx.geom
        xs, weight, w16 = ctx.saved_tensors
        dy = _nhwc(dy)
        st = stream_of(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            if ctx.mode != "direct":
                raise NotImplementedError("input gradient of a small-channel (stem) convolution")
            wt = weight_bf16_t(weight)
            dx = torch.empty((N, C, H, W), dtype=BF16, device=dy.device, memory_format=CL)
            _lib.call("mi_conv2d_dgrad", ptr(dy), ptr(wt), ptr(dx), N, H, W, C, K, R, S, stride, padding, P, Q, st)
        if ctx.needs_input_grad[1]:
            g = _grad_buffer(weight)
            on_side = ctx.mode == "direct" and _side(weight) is not None
            if on_side:
                # flat engine with a weight-gradient stream: kernels + ready signal on the side stream
                run_wgrad(weight, lambda: _lib.call("mi_conv2d_wgrad", ptr(xs), ptr(dy), ptr(g), N, H, W, C, K, R,
                                                    S, stride, padding, P, Q, stream_of(dy)), (xs, dy))
            elif ctx.mode == "direct":
                _lib.call("mi_conv2d_wgrad", ptr(xs), ptr(dy), ptr(g), N, H, W, C, K, R, S, stride, padding, P, Q, st)
            elif ctx.mode == "c8":
                gp = torch.zeros((K, R, S, 8), dtype=torch.float32, device=dy.device)
                _lib.call("mi_conv2d_wgrad", ptr(xs), ptr(dy), ptr(gp), N, H, W, 8, K, R, S, stride, padding, P, Q,
                          st)
                g.add_(gp[..., :Cw].permute(0, 3, 1, 2))
            else:
                Kr = R * S * C
                Kp = xs.shape[1]
                gp = torch.zeros((K, Kp), dtype=torch.float32, device=dy.device)
                _lib.call("mi_gemm_tn", ptr(dy), ptr(xs), ptr(gp), K, Kp, N * P * Q, K, Kp, Kp, st)
                g.add_(gp[:, :Kr].reshape(K, R, S, C).permute(0, 3, 1, 2))
            if not on_side:
                dw = _finish_grad(weight, g)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            bias = ctx.bias_param
            gb = _grad_buffer(bias)
            if K % 8 == 0:  # dy is NHWC storage: a [N*P*Q][K] row-major matrix
                _lib.call("mi_colsum_bf16", ptr(dy), ptr(gb), N * P * Q, K, K, st)
            else:
                gb.add_(dy.float().sum(dim=(0, 2, 3)))
            db = _finish_grad(bias, gb)
        return dx, dw, db, None, None, None


def conv2d(x, weight, bias=None, stride=1, padding=0):
    if not x.is_cuda:
        return F.conv2d(x, weight, bias, stride, padding)
    return _Conv2d.apply(x, weight, bias, stride, padding, None)


def conv2d_with_stats(x, weight, stride=1, padding=0):
    """Conv (no bias) whose epilogue also writes per-channel (sum, sumsq) partials of its bf16
    output -> (y, (slab, rows)); feeds ``batch_norm_act(..., stats=...)`` so BN skips its own
    statistics pass over y (one full read of the activation saved per BN layer)."""
    N, C, H, W = x.shape
    K, _, R, S = weight.shape
    P, Q = _conv_out(H, R, stride, padding), _conv_out(W, S, stride, padding)
    lib = _lib.load()
    rows = lib.mi_conv_stat_rows_g(N, H, W, C if C % 64 == 0 else 8, K, R, S, stride, padding, P, Q)
    slab = torch.empty((rows + lib.mi_bn_slab_extra_rows(), 2, K), dtype=torch.float32, device=x.device)
    y = _Conv2d.apply(x, weight, None, stride, padding, slab)
    return y, (slab, rows)


# ================================================================ batch norm
class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, residual, running_mean, running_var, nbt, training, momentum, eps, relu,
                stats):
        N, C, H, W = x.shape
        M = N * H * W
        x = _nhwc(x)
        res = _nhwc(residual) if residual is not None else None
        st = stream_of(x)
        dev = x.device
        y = torch.empty_like(x, memory_format=CL)
        f32 = dict(dtype=torch.float32, device=dev)
        scale = torch.empty(C, **f32)
        shift = torch.empty(C, **f32)
        if training:
            if stats is not None:
                part, pre_rows = stats
            else:
                lib = _lib.load()
                part = torch.empty((lib.mi_bn_partial_rows(M, C) + lib.mi_bn_slab_extra_rows(), 2, C), **f32)
                pre_rows = 0
            mean = torch.empty(C, **f32)
            invstd = torch.empty(C, **f32)
            _lib.call("mi_bn_fwd_train", ptr(x), ptr(res), ptr(y), M, C, float(eps), float(momentum),
                      ptr(weight), ptr(bias), ptr(running_mean), ptr(running_var), ptr(nbt), ptr(mean),
                      ptr(invstd), ptr(scale), ptr(shift), ptr(part), int(pre_rows), int(relu), st)
        else:
            mean = invstd = None
            _lib.call("mi_bn_fwd_eval", ptr(x), ptr(res), ptr(y), M, C, float(eps), ptr(weight), ptr(bias),
                      ptr(running_mean), ptr(running_var), ptr(scale), ptr(shift), int(relu), st)
        ctx.training = training
        ctx.relu = relu
        ctx.has_res = residual is not None
        ctx.save_for_backward(x, y, weight, bias, mean, invstd, scale)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, weight, bias, mean, invstd, scale = ctx.saved_tensors
        dy = _nhwc(dy)
        N, C, H, W = x.shape
        M = N * H * W
        st = stream_of(dy)
        dev = dy.device
        dx = torch.empty_like(x, memory_format=CL)
        dres = torch.empty_like(x, memory_format=CL) if (ctx.has_res and ctx.needs_input_grad[3]) else None
        dw = db = None
        if ctx.training:
            gw = _grad_buffer(weight) if (weight is not None and ctx.needs_input_grad[1]) else None
            gb = _grad_buffer(bias) if (bias is not None and ctx.needs_input_grad[2]) else None
            lib = _lib.load()
            nblk = lib.mi_bn_partial_rows(M, C) + lib.mi_bn_slab_extra_rows()
            part = torch.empty((nblk, 2, C), dtype=torch.float32, device=dev)
            coef = torch.empty((3, C), dtype=torch.float32, device=dev)
            _lib.call("mi_bn_bwd_train", ptr(dy), ptr(y), ptr(x), ptr(dx), ptr(dres), M, C, ptr(weight), ptr(mean),
                      ptr(invstd), ptr(gw), ptr(gb), ptr(coef), ptr(part), int(ctx.relu), st)
            if gw is not None:
                dw = _finish_grad(weight, gw)
            if gb is not None:
                db = _finish_grad(bias, gb)
        else:
            _lib.call("mi_bn_bwd_eval", ptr(dy), ptr(y), ptr(scale), ptr(dx), ptr(dres), M, C, int(ctx.relu), st)
        return dx, dw, db, dres, None, None, None, None, None, None, None, None


def batch_norm_act(x, weight, bias, running_mean, running_var, num_batches_tracked, training, momentum, eps,
                   relu=False, residual=None, stats=None):
    """y = act(BN(x) + residual).  ``momentum=None`` (cumulative average) is resolved by the caller."""
    if not x.is_cuda:
        y = F.batch_norm(x, running_mean, running_var, weight, bias, training, momentum, eps)
        if training and num_batches_tracked is not None:
            num_batches_tracked.add_(1)
        if residual is not None:
            y = y + residual
        return F.relu(y) if relu else y
    if not training and running_mean is None:
        raise ValueError("eval-mode batch_norm without running statistics")
    return _BatchNormAct.apply(x, weight, bias, residual, running_mean, running_var,
                               num_batches_tracked if training else None, bool(training), float(momentum),
                               float(eps), bool(relu), stats if training else None)


# ==================================================================== pooling
class _MaxPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k, s, pad):
        N, C, H, W = x.shape
        P, Q = _conv_out(H, k, s, pad), _conv_out(W, k, s, pad)
        x = _nhwc(x)
        y = torch.empty((N, C, P, Q), dtype=BF16, device=x.device, memory_format=CL)
        idx = torch.empty((N, P, Q, C), dtype=torch.uint8, device=x.device)
        _lib.call("mi_maxpool_fwd", ptr(x), ptr(y), ptr(idx), N, H, W, C, P, Q, k, s, pad, stream_of(x))
        ctx.save_for_backward(idx)
        ctx.geom = (N, C, H, W, P, Q, k, s, pad)
        return y

    @staticmethod
    def backward(ctx, dy):
        (idx,) = ctx.saved_tensors
        N, C, H, W, P, Q, k, s, pad = ctx.geom
        dy = _nhwc(dy)
        dx = torch.empty((N, C, H, W), dtype=BF16, device=dy.device, memory_format=CL)
        _lib.call("mi_maxpool_bwd", ptr(dy), ptr(idx), ptr(dx), N, H, W, C, P, Q, k, s, pad, stream_of(dy))
        return dx, None, None, None


def max_pool2d(x, kernel_size=3, stride=2, padding=1):
    if not x.is_cuda:
        return F.max_pool2d(x, kernel_size, stride, padding)
    return _MaxPool.apply(x, int(kernel_size), int(stride), int(padding))


class _GlobalAvgPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        N, C, H, W = x.shape
        x = _nhwc(x)
        y = torch.empty((N, C), dtype=BF16, device=x.device)
        _lib.call("mi_gap_fwd", ptr(x), ptr(y), N, H * W, C, stream_of(x))
        ctx.geom = (N, C, H, W)
        return y

    @staticmethod
    def backward(ctx, dy):
        N, C, H, W = ctx.geom
        dy = dy.to(BF16).contiguous()
        dx = torch.empty((N, C, H, W), dtype=BF16, device=dy.device, memory_format=CL)
        _lib.call("mi_gap_bwd", ptr(dy), ptr(dx), N, H * W, C, stream_of(dy))
        return dx


def global_avg_pool(x):
    """[N,C,H,W] -> [N,C]  (AdaptiveAvgPool2d(1) + flatten)."""
    if not x.is_cuda:
        return torch.flatten(F.adaptive_avg_pool2d(x, 1), 1)
    return _GlobalAvgPool.apply(x)


# ===================================================================== linear
class _Linear(torch.autograd.Function):
    """y = x W^T + b on MFMA GEMMs; output fp32.  Feature dims that are not a multiple
    of 8 (e.g. a 10-class head) are zero-padded to the 16-byte vector granule."""

    @staticmethod
    def forward(ctx, x, weight, bias, out_bf16=False):
        x2 = x.reshape(-1, x.shape[-1])
        if x2.dtype != BF16:
            x2 = x2.to(BF16)
        x2 = x2.contiguous()
        M, Kd = x2.shape
        N = weight.shape[0]
        if Kd % 8:
            raise NotImplementedError("native linear needs in_features % 8 == 0")
        Np = (N + 7) // 8 * 8
        w16 = weight_bf16(weight)
        bp = bias
        if Np != N:
            wp = torch.zeros((Np, Kd), dtype=BF16, device=x.device)
            wp[:N].copy_(w16)
            w16 = wp
            if bias is not None:
                bp = torch.zeros(Np, dtype=torch.float32, device=x.device)
                bp[:N].copy_(bias)
        y = torch.empty((M, Np), dtype=BF16 if out_bf16 else torch.float32, device=x.device)
        _lib.call("mi_gemm_nt", ptr(x2), ptr(w16), ptr(y), ptr(bp), ptr(None), M, Np, Kd, Kd, Kd, Np,
                  0 if out_bf16 else 1, 0, stream_of(x))
        if Np != N:
            y = y[:, :N].contiguous()
        ctx.save_for_backward(x2, weight, w16)
        ctx.bias_param = bias
        ctx.has_bias = bias is not None
        ctx.in_shape = x.shape
        ctx.in_dtype = x.dtype
        return y.reshape(*x.shape[:-1], N)

    @staticmethod
    def backward(ctx, dy):
        x2, weight, w16 = ctx.saved_tensors  # w16 is [Np][Kd] (padded if needed)
        M, Kd = x2.shape
        N = weight.shape[0]
        Np = w16.shape[0]
        dy2 = dy.reshape(M, N)
        gb32 = None
        if Np != N:
            dyp = torch.zeros((M, Np), dtype=BF16, device=dy.device)
            dyp[:, :N].copy_(dy2)
            dy2 = dyp
        elif dy2.dtype == torch.float32 and dy2.is_contiguous() and N % 8 == 0:
            # fp32 logits gradient: one native pass casts it to the bf16 GEMM operand and sums the
            # bias gradient from the fp32 values
            d16 = torch.empty((M, N), dtype=BF16, device=dy.device)
            if ctx.has_bias and ctx.needs_input_grad[2]:
                gb32 = _grad_buffer(ctx.bias_param)
            _lib.call("mi_cast_colsum_f32", ptr(dy2), ptr(d16), ptr(gb32), M, N, stream_of(dy))
            dy2 = d16
        else:
            dy2 = dy2.to(BF16).contiguous()
        st = stream_of(dy)
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            # dX[M][Kd] = dY[M][Np] * W[Np][Kd]  ->  NT with B = W^T [Kd][Np]
            wt = linear_weight_t(weight) if Np == N else w16.t().contiguous()
            dxf = torch.empty((M, Kd), dtype=BF16, device=dy.device)
            _lib.call("mi_gemm_nt", ptr(dy2), ptr(wt), ptr(dxf), ptr(None), ptr(None), M, Kd, Np, Np, Np, Kd, 0, 0, st)
            dx = dxf.reshape(ctx.in_shape).to(ctx.in_dtype)
        if ctx.needs_input_grad[1]:
            g = _grad_buffer(weight)
            if Np == N:
                _lib.call("mi_gemm_tn", ptr(dy2), ptr(x2), ptr(g), N, Kd, M, N, Kd, Kd, st)
            else:
                gp = torch.zeros((Np, Kd), dtype=torch.float32, device=dy.device)
                _lib.call("mi_gemm_tn", ptr(dy2), ptr(x2), ptr(gp), Np, Kd, M, Np, Kd, Kd, st)
                g.add_(gp[:N])
            dw = _finish_grad(weight, g)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            bias = ctx.bias_param
            gb = gb32 if gb32 is not None else _grad_buffer(bias)  # gb32: summed by the cast pass
            if gb32 is None and dy2.dtype == BF16 and Np == N and dy.dtype == BF16:
                _lib.call("mi_colsum_bf16", ptr(dy2), ptr(gb), M, N, N, st)
            elif gb32 is None:
                gb.add_(dy.reshape(M, N).float().sum(0))
            db = _finish_grad(bias, gb)
        return dx, dw, db, None


def linear(x, weight, bias=None, out_bf16=False):
    """MFMA GEMM linear layer; ``out_bf16`` keeps activations bf16 (transformer internals),
    otherwise fp32 output (classifier heads / logits)."""
    if not x.is_cuda:
        return F.linear(x, weight, bias)
    return _Linear.apply(x, weight, bias, bool(out_bf16))


# ============================================================= cross entropy
class _CrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target):
        lg = logits.float().contiguous()
        N, ncls = lg.shape
        tgt = target.to(torch.int64).contiguous()
        lse = torch.empty(2 * N, dtype=torch.float32, device=lg.device)  # [lse rows | per-row losses]
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        _lib.call("mi_ce_fwd", ptr(lg), ptr(tgt), ptr(lse), ptr(loss), N, ncls, ncls, stream_of(lg))
        ctx.save_for_backward(lg, tgt, lse)
        ctx.in_dtype = logits.dtype
        return loss

    @staticmethod
    def backward(ctx, gout):
        lg, tgt, lse = ctx.saved_tensors
        N, ncls = lg.shape
        g = gout.float().contiguous().reshape(1)
        f32 = ctx.in_dtype == torch.float32  # the gradient in the logits' dtype: no autograd cast launch
        dl = torch.empty((N, ncls), dtype=torch.float32 if f32 else BF16, device=lg.device)
        _lib.call("mi_ce_bwd", ptr(lg), ptr(tgt), ptr(lse), ptr(g), ptr(dl), N, ncls, ncls, ncls, int(f32),
                  stream_of(lg))
        return dl.to(ctx.in_dtype), None


class MixedTarget(NamedTuple):
    """Mixup / CutMix target: row n is ``lam[n]`` of class ``y_a[n]`` and ``1 - lam[n]`` of class
    ``y_b[n]``.  ``y_a`` / ``y_b`` int64 [N], ``lam`` fp32 [N] on the logits' device (a device tensor,
    so a loss captured in a HIP graph sees the new values on every replay)."""
    y_a: torch.Tensor
    y_b: torch.Tensor
    lam: torch.Tensor

    def dense(self, num_classes, dtype=torch.float32):
        """The equivalent [N, C] probability target (reference / CPU path; the kernels never build it)."""
        lam = self.lam.to(dtype).unsqueeze(1)
        return lam * F.one_hot(self.y_a, num_classes).to(dtype) + (1 - lam) * F.one_hot(self.y_b, num_classes).to(dtype)


class _CrossEntropyPair(torch.autograd.Function):
    """Pair target (y_a, y_b, lam) with label smoothing; ``lam is None``: hard labels (y_a is y_b)."""

    @staticmethod
    def forward(ctx, logits, y_a, y_b, lam, eps):
        lg = logits.float().contiguous()
        N, ncls = lg.shape
        ws = torch.empty(2 * N, dtype=torch.float32, device=lg.device)  # [lse rows | per-row losses]
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        _lib.call("mi_ce_pair_fwd", ptr(lg), ptr(y_a), ptr(y_b), ptr(lam), ptr(ws),
                  ptr(loss), N, ncls, ncls, eps, stream_of(lg))
        ctx.save_for_backward(lg, y_a, y_b, ws, *(() if lam is None else (lam,)))
        ctx.in_dtype, ctx.eps = logits.dtype, eps
        return loss

    @staticmethod
    def backward(ctx, gout):
        lg, y_a, y_b, ws, *rest = ctx.saved_tensors
        lam = rest[0] if rest else None
        N, ncls = lg.shape
        g = gout.float().contiguous().reshape(1)
        f32 = ctx.in_dtype == torch.float32  # the gradient in the logits' dtype: no autograd cast launch
        dl = torch.empty((N, ncls), dtype=torch.float32 if f32 else BF16, device=lg.device)
        _lib.call("mi_ce_pair_bwd", ptr(lg), ptr(y_a), ptr(y_b), ptr(lam), ptr(ws),
                  ptr(g), ptr(dl), N, ncls, ncls, ncls, ctx.eps, int(f32), stream_of(lg))
        return dl.to(ctx.in_dtype), None, None, None, None


class _CrossEntropyDense(torch.autograd.Function):
    """Dense [N, C] probability targets (fp32 or bf16; rows need not sum to one) with label smoothing."""

    @staticmethod
    def forward(ctx, logits, target, eps):
        lg = logits.float().contiguous()
        N, ncls = lg.shape
        tgt = target.contiguous()
        ws = torch.empty(3 * N, dtype=torch.float32, device=lg.device)  # [lse rows | per-row losses | sum q]
        loss = torch.empty((), dtype=torch.float32, device=lg.device)
        _lib.call("mi_ce_dense_fwd", ptr(lg), ptr(tgt), int(tgt.dtype == BF16), ptr(ws), ptr(loss), N, ncls, ncls,
                  ncls, eps, stream_of(lg))
        ctx.save_for_backward(lg, tgt, ws)
        ctx.in_dtype, ctx.eps = logits.dtype, eps
        return loss

    @staticmethod
    def backward(ctx, gout):
        lg, tgt, ws = ctx.saved_tensors
        N, ncls = lg.shape
        g = gout.float().contiguous().reshape(1)
        f32 = ctx.in_dtype == torch.float32
        dl = torch.empty((N, ncls), dtype=torch.float32 if f32 else BF16, device=lg.device)
        _lib.call("mi_ce_dense_bwd", ptr(lg), ptr(tgt), int(tgt.dtype == BF16), ptr(ws), ptr(g), ptr(dl), N, ncls,
                  ncls, ncls, ncls, ctx.eps, int(f32), stream_of(lg))
        return dl.to(ctx.in_dtype), None, None


def _index_target(t, N, dev, what):
    if t.dtype != torch.int64 or t.shape != (N,) or t.device != dev:
        raise ValueError(f"cross_entropy: {what} must be an int64 [{N}] tensor on {dev}")
    return t.contiguous()


def cross_entropy(logits, target, label_smoothing=0.0):
    """Mean-reduced cross entropy (log-softmax + NLL) fused fwd/bwd, ``F.cross_entropy`` semantics.

    ``target``: int64 [N] class indices, a ``MixedTarget(y_a, y_b, lam)`` (Mixup / CutMix; [N, C] is
    never materialised) or a floating-point [N, C] probability tensor (fp32 or bf16).  Smoothing acts
    on probability targets as ``q = (1 - eps) * t + eps / C``."""
    eps = float(label_smoothing)
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"label_smoothing must be in [0, 1], got {label_smoothing}")
    if logits.dim() != 2:
        raise ValueError("cross_entropy expects [N, C] logits")
    N, ncls = logits.shape
    mixed = isinstance(target, MixedTarget)
    dense = not mixed and target.is_floating_point()
    if not logits.is_cuda:
        if not mixed and not dense and eps == 0.0:
            return F.cross_entropy(logits.float(), target)
        if mixed:
            t = target.dense(ncls)
        elif dense:
            t = target.float()
        else:
            t = F.one_hot(target, ncls).float()
        return F.cross_entropy(logits.float(), t, label_smoothing=eps)
    dev = logits.device
    if mixed:
        y_a = _index_target(target.y_a, N, dev, "MixedTarget.y_a")
        y_b = _index_target(target.y_b, N, dev, "MixedTarget.y_b")
        lam = target.lam
        if lam.dtype != torch.float32 or lam.shape != (N,) or lam.device != dev:
            raise ValueError(f"cross_entropy: MixedTarget.lam must be an fp32 [{N}] tensor on {dev}")
        return _CrossEntropyPair.apply(logits, y_a, y_b, lam.contiguous(), eps)
    if dense:
        if target.shape != (N, ncls) or target.device != dev:
            raise ValueError(f"cross_entropy: dense targets must be [{N}, {ncls}] on {dev}")
        if target.dtype not in (torch.float32, BF16):
            target = target.float()
        return _CrossEntropyDense.apply(logits, target, eps)
    if eps == 0.0:
        return _CrossEntropy.apply(logits, target)  # today's hard-label kernels, unchanged
    y = _index_target(target.to(torch.int64), N, dev, "target")
    return _CrossEntropyPair.apply(logits, y, y, None, eps)


# ================================================================= optimizer
def _f32(x) -> float:
    """host fallbacks: ``x`` rounded to fp32, the way the launchers round the constants they pass"""
    return float(torch.tensor(x, dtype=torch.float32))


def _check_f32(n, *tensors):
    for t in tensors:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n


def _clip_coef_host(state, sumsq, max_norm, grad_scale) -> float:
    """host fallback of the prep kernels' clip coefficient (``clip_grad_norm_``): 1 without
    ``max_norm``, else ``state[2]`` = the total norm and min(1, max_norm / (total + 1e-6))"""
    if max_norm is None:
        return 1.0
    total = grad_scale * math.sqrt(float(sumsq.reshape(-1)[0]))
    state[2] = total
    c = float(max_norm) / (total + 1e-6)
    return 1.0 if c > 1.0 else c  # NaN stays NaN, like torch's clamp(max=1)


def sgd_flat_(params, grads, momentum_buf, params_bf16, lr, momentum=0.0, dampening=0.0, weight_decay=0.0,
              nesterov=False, first_step=False, grad_scale=1.0):
    """One fused SGD update over flat fp32 buffers (+ bf16 compute-copy refresh)."""
    if not params.is_cuda:
        with torch.no_grad():
            d = grads * grad_scale
            if weight_decay:
                d = d + weight_decay * params
            if momentum:
                if first_step:
                    momentum_buf.copy_(d)
                else:
                    momentum_buf.mul_(momentum).add_(d, alpha=1 - dampening)
                d = d + momentum * momentum_buf if nesterov else momentum_buf
            params.add_(d, alpha=-lr)
            if params_bf16 is not None:
                params_bf16.copy_(params)
        return
    _lib.call("mi_sgd_flat", ptr(params), ptr(grads), ptr(momentum_buf), ptr(params_bf16), params.numel(),
              float(lr), float(momentum), float(dampening), float(weight_decay), int(nesterov), int(first_step),
              float(grad_scale), stream_of(params))


# flat AdamW (csrc/kernels/optim.hip).  Device state block, float64:
#   [0] step t  [1] lr  [2] total_norm  [3] clip coefficient
#   [4] lr / bc1  [5] 1 / sqrt(bc2)  [6] grad_scale * coef  [7] lr * wd
ADAMW_STATE_LEN = 8


def grad_sqnorm_slots(numels) -> int:
    """fp64 partial slots ``grad_sqnorm_`` needs for segments of these sizes (0 on the host)."""
    lib = _lib.load(required=False)
    if lib is None:
        return 0
    return sum(lib.mi_grad_sqnorm_blocks(int(n)) for n in numels)


def grad_sqnorm_(segments, out, partials=None):
    """``out[0]`` (float64, one element) = sum of squares over all fp32 ``segments``, accumulated in
    fp64 and deterministic: block partials in fixed slots of ``partials`` (``grad_sqnorm_slots``
    doubles), summed in a fixed order by one block.  The result stays on the device."""
    segments = list(segments)
    if not out.is_cuda:
        with torch.no_grad():
            s = torch.zeros((), dtype=torch.float64)
            for x in segments:
                xd = x.double().reshape(-1)
                s = s + (xd * xd).sum()
            out.reshape(-1)[0] = s
        return out
    lib = _lib.load(True)
    blocks = [lib.mi_grad_sqnorm_blocks(x.numel()) for x in segments]
    if partials is None:
        partials = torch.empty(sum(blocks), dtype=torch.float64, device=out.device)
    assert partials.dtype == torch.float64 and partials.numel() >= sum(blocks) and out.dtype == torch.float64
    st, slot = stream_of(out), 0
    for x, nb in zip(segments, blocks):
        _check_f32(x.numel(), x)
        _lib.call("mi_grad_sqnorm_partial", ptr(x), x.numel(), ctypes.c_void_p(partials.data_ptr() + 8 * slot), st)
        slot += nb
    _lib.call("mi_grad_sqnorm_final", ptr(partials), slot, ptr(out), st)
    return out


def adamw_prep_(state, sumsq, beta1, beta2, weight_decay, max_norm=None, grad_scale=1.0):
    """Advance the device step counter and derive this step's scalars in ``state`` (layout above)
    from ``state[1]`` (lr) and, when ``max_norm`` is given, the squared gradient norm ``sumsq``:
    ``total_norm = grad_scale * sqrt(sumsq)``, ``coef = min(1, max_norm / (total_norm + 1e-6))``
    (``torch.nn.utils.clip_grad_norm_``).  No host read."""
    clip = max_norm is not None
    if not state.is_cuda:
        with torch.no_grad():
            t = float(state[0]) + 1.0
            lr = float(state[1])
            bc1, bc2 = 1.0 - beta1 ** t, 1.0 - beta2 ** t
            coef = _clip_coef_host(state, sumsq, max_norm, grad_scale)
            state[0] = t
            state[3] = coef
            state[4] = lr / bc1
            state[5] = 1.0 / math.sqrt(bc2)
            state[6] = grad_scale * coef
            state[7] = lr * weight_decay
        return
    assert state.dtype == torch.float64 and state.numel() >= ADAMW_STATE_LEN
    _lib.call("mi_adamw_prep", ptr(state), ptr(sumsq) if clip else ptr(None), float(beta1), float(beta2),
              float(weight_decay), float(max_norm) if clip else 0.0, float(grad_scale), int(clip), stream_of(state))


def adamw_flat_(params, grads, exp_avg, exp_avg_sq, params_bf16, state, beta1, beta2, eps, decay_map=None,
                unit_base=0):
    """One fused AdamW update over flat fp32 buffers (+ bf16 compute-copy refresh) with the
    per-step scalars of ``adamw_prep_``.  ``decay_map``: uint8, one byte per 64-element unit of the
    whole flat buffer (nonzero: the unit decays), ``unit_base`` the unit index of ``params[0]``;
    None decays everything."""
    n = params.numel()
    if decay_map is not None:
        assert decay_map.dtype == torch.uint8 and decay_map.numel() >= unit_base + (n + 63) // 64
    if not params.is_cuda:
        with torch.no_grad():
            s = state.tolist()
            g = grads * _f32(s[6])
            decayed = params * _f32(1.0 - s[7])
            if decay_map is None:
                params.copy_(decayed)
            else:
                units = decay_map[unit_base:unit_base + (n + 63) // 64] != 0
                params.copy_(torch.where(units.repeat_interleave(64)[:n], decayed, params))
            exp_avg.mul_(beta1).add_(g, alpha=1 - beta1)
            exp_avg_sq.mul_(beta2).addcmul_(g, g, value=1 - beta2)
            denom = exp_avg_sq.sqrt().mul_(_f32(s[5])).add_(eps)
            params.addcdiv_(exp_avg, denom, value=-_f32(s[4]))
            if params_bf16 is not None:
                params_bf16.copy_(params)
        return
    _check_f32(n, params, grads, exp_avg, exp_avg_sq)
    _lib.call("mi_adamw_flat", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), ptr(params_bf16), n,
              ptr(state), ptr(decay_map), int(unit_base), float(beta1), float(beta2), float(eps), stream_of(params))


# layer-wise optimizers (second half of csrc/kernels/optim.hip).  Every range is whole 64-element
# units; a unit belongs to one parameter or to none (``pidx < 0``).  Device state blocks, float64:
#   LARS  [0] step t  [1] lr
#   LAMB  [0] step t  [1] lr  [2] total_norm  [3] clip coefficient  [4] bc1  [5] bc2
#         [6] grad_scale * coef  [7] unused
LARS_STATE_LEN = 2
LAMB_STATE_LEN = 8
SEG_UNIT = 64


def _unit_lookup(pidx, excl, q, unit_base, n):
    """host: per-element (excluded, q) of ``n`` elements starting at unit ``unit_base``"""
    idx = pidx[unit_base:unit_base + n // SEG_UNIT].long()
    safe = idx.clamp(min=0)
    ex = (idx < 0) | (excl[safe] != 0)
    qu = None if q is None else torch.where(ex, torch.ones((), dtype=torch.float32), q[safe])
    rep = lambda t: None if t is None else t.repeat_interleave(SEG_UNIT)  # noqa: E731
    return rep(ex), rep(qu)


def _unit_sq_host(t):
    """host: fp64 sum of squares of every 64-element unit of ``t``"""
    return t.double().reshape(-1, SEG_UNIT).pow(2).sum(1)


def seg_sqnorm_units_(x, part, y=None, part_y=None):
    """Pass 1 of the segmented norms: ``part[u]`` (float64) = sum of squares of the fp32 elements
    ``x[64 u : 64 u + 64]``; with ``y`` also ``part_y[u]`` from ``y`` in the same launch.  The bits of
    a unit's partial depend on its 64 values alone."""
    n = x.numel()
    assert n % SEG_UNIT == 0 and part.dtype == torch.float64 and part.numel() >= n // SEG_UNIT
    if y is not None:
        assert y.numel() == n and part_y.dtype == torch.float64 and part_y.numel() >= n // SEG_UNIT
    if not x.is_cuda:
        with torch.no_grad():
            for src, dst in ((x, part), (y, part_y)):
                if src is not None:
                    dst[:n // SEG_UNIT] = _unit_sq_host(src)
        return
    _check_f32(n, *(t for t in (x, y) if t is not None))
    assert part.is_contiguous() and (part_y is None or part_y.is_contiguous())
    _lib.call("mi_seg_sqnorm_units", ptr(x), ptr(y), n, ptr(part), ptr(part_y), stream_of(x))


def seg_sqnorm_reduce_(parts, table, out):
    """Pass 2: ``out[s * P + p]`` = sum of ``parts[s, table[p, 0]:table[p, 1]]`` in a fixed order
    that depends on the range alone.  ``parts``: float64 ``[nsets, U]`` (or ``[U]``) unit partials,
    ``table``: int64 ``[P, 2]`` unit ranges (may be empty), ``out``: float64, ``nsets * P``."""
    parts2 = parts.reshape(1, -1) if parts.dim() == 1 else parts
    nsets, stride = parts2.shape
    P = table.shape[0]
    assert table.dtype == torch.int64 and table.shape == (P, 2) and table.is_contiguous()
    assert out.dtype == torch.float64 and out.numel() >= nsets * P and parts2.dtype == torch.float64
    if not out.is_cuda:
        with torch.no_grad():
            flat = out.reshape(-1)
            for s in range(nsets):
                for p, (lo, hi) in enumerate(table.tolist()):
                    flat[s * P + p] = parts2[s, lo:hi].sum()
        return out
    assert parts2.is_contiguous() and out.is_contiguous()
    _lib.call("mi_seg_sqnorm_reduce", ptr(parts2), int(stride), int(nsets), ptr(table), int(P), ptr(out),
              stream_of(out))
    return out


def lars_trust_(sums, excl, q, state, trust_coefficient, weight_decay, eps, grad_scale=1.0):
    """``q[p]`` (float32) from ``sums`` = [sum w^2 per parameter | sum g^2 per parameter] (float64,
    g unscaled): ``tc * |w| / (grad_scale * |g| + wd * |w| + eps)`` where both norms are > 0 and
    the parameter is not excluded, else 1.  Advances ``state[0]`` (the step counter)."""
    P = excl.numel()
    assert sums.numel() >= 2 * P and q.numel() >= P
    if not sums.is_cuda:
        with torch.no_grad():
            wn = sums[:P].sqrt()
            gn = grad_scale * sums[P:2 * P].sqrt()
            r = trust_coefficient * wn / (gn + weight_decay * wn + eps)
            ok = (excl == 0) & (wn > 0) & (gn > 0)
            q[:P] = torch.where(ok, r, torch.ones_like(r)).float()
            state[0] += 1.0
        return
    assert sums.dtype == torch.float64 and excl.dtype == torch.uint8 and q.dtype == torch.float32
    assert state.dtype == torch.float64 and state.numel() >= LARS_STATE_LEN
    _lib.call("mi_lars_trust", ptr(sums), ptr(excl), ptr(q), ptr(state), int(P), float(trust_coefficient),
              float(weight_decay), float(eps), float(grad_scale), stream_of(sums))


def lamb_trust_(sums, excl, q):
    """``q[p]`` = ``|w| / |u|`` from ``sums`` = [sum w^2 | sum u^2] where both are > 0 and the
    parameter is not excluded, else 1."""
    P = excl.numel()
    assert sums.numel() >= 2 * P and q.numel() >= P
    if not sums.is_cuda:
        with torch.no_grad():
            wn, un = sums[:P].sqrt(), sums[P:2 * P].sqrt()
            ok = (excl == 0) & (wn > 0) & (un > 0)
            q[:P] = torch.where(ok, wn / un, torch.ones_like(wn)).float()
        return
    assert sums.dtype == torch.float64 and excl.dtype == torch.uint8 and q.dtype == torch.float32
    _lib.call("mi_lamb_trust", ptr(sums), ptr(excl), ptr(q), int(P), stream_of(sums))


def _check_units(n, pidx, unit_base, *tensors):
    assert n % SEG_UNIT == 0, "layer-wise kernels take whole 64-element units"
    assert pidx.dtype == torch.int32 and pidx.numel() >= unit_base + n // SEG_UNIT and unit_base >= 0
    _check_f32(n, *tensors)


def lars_flat_(params, grads, momentum_buf, params_bf16, state, pidx, excl, q, unit_base, momentum, weight_decay,
               grad_scale=1.0):
    """One fused LARS update over whole units of the flat buffers (+ bf16 compute-copy refresh):
    ``g' = grad_scale * g``; ``d = q * (g' + wd * w)``, for excluded units ``d = g'``;
    ``buf = momentum * buf + d``; ``w -= lr * buf`` with ``lr = state[1]``.  ``pidx``: int32 parameter
    index per unit of the whole flat buffer (< 0: no parameter), ``excl`` / ``q`` per parameter."""
    n = params.numel()
    _check_units(n, pidx, unit_base, params, grads, momentum_buf)
    if not params.is_cuda:
        with torch.no_grad():
            ex, qe = _unit_lookup(pidx, excl, q, unit_base, n)
            g = grads * _f32(grad_scale)
            d = torch.where(ex, g, qe * (g + _f32(weight_decay) * params))
            momentum_buf.mul_(_f32(momentum)).add_(d)
            params.sub_(_f32(float(state[1])) * momentum_buf)
            if params_bf16 is not None:
                params_bf16.copy_(params)
        return
    _lib.call("mi_lars_flat", ptr(params), ptr(grads), ptr(momentum_buf), ptr(params_bf16), n, ptr(state),
              ptr(pidx), ptr(excl), ptr(q), int(unit_base), float(momentum), float(weight_decay), float(grad_scale),
              stream_of(params))


def lamb_prep_(state, sumsq, beta1, beta2, max_norm=None, grad_scale=1.0):
    """Advance the LAMB step counter and derive the bias corrections and, when ``max_norm`` is
    given, the clip coefficient from the squared gradient norm ``sumsq`` (as ``adamw_prep_``)."""
    clip = max_norm is not None
    if not state.is_cuda:
        with torch.no_grad():
            t = float(state[0]) + 1.0
            coef = _clip_coef_host(state, sumsq, max_norm, grad_scale)
            state[0] = t
            state[3] = coef
            state[4] = 1.0 - beta1 ** t
            state[5] = 1.0 - beta2 ** t
            state[6] = grad_scale * coef
        return
    assert state.dtype == torch.float64 and state.numel() >= LAMB_STATE_LEN
    _lib.call("mi_lamb_prep", ptr(state), ptr(sumsq) if clip else ptr(None), float(beta1), float(beta2),
              float(max_norm) if clip else 0.0, float(grad_scale), int(clip), stream_of(state))


def _lamb_u_host(params, exp_avg, exp_avg_sq, ex, state, eps, weight_decay):
    r = (exp_avg / _f32(float(state[4]))) / ((exp_avg_sq / _f32(float(state[5]))).sqrt() + _f32(eps))
    return torch.where(ex, r, r + _f32(weight_decay) * params)


def lamb_moments_(params, grads, exp_avg, exp_avg_sq, state, pidx, excl, unit_base, part_w, part_u, beta1, beta2,
                  eps, weight_decay):
    """LAMB, first launch of a segment: ``m``, ``v`` updated from ``g' = state[6] * g``;
    ``u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * w`` (excluded units: no ``wd * w``) is formed in
    registers and its per-unit sums of squares go to ``part_u``, those of ``w`` to ``part_w`` (float64,
    one per unit of this range, the scheme of ``seg_sqnorm_units_``).  ``params`` is not written."""
    n = params.numel()
    _check_units(n, pidx, unit_base, params, grads, exp_avg, exp_avg_sq)
    for t in (part_w, part_u):
        assert t.dtype == torch.float64 and t.numel() >= n // SEG_UNIT and t.is_contiguous()
    if not params.is_cuda:
        with torch.no_grad():
            ex, _ = _unit_lookup(pidx, excl, None, unit_base, n)
            g = grads * _f32(float(state[6]))
            exp_avg.mul_(_f32(beta1)).add_(g, alpha=_f32(1.0 - beta1))
            exp_avg_sq.mul_(_f32(beta2)).add_(g * g, alpha=_f32(1.0 - beta2))
            u = _lamb_u_host(params, exp_avg, exp_avg_sq, ex, state, eps, weight_decay)
            part_w[:n // SEG_UNIT] = _unit_sq_host(params)
            part_u[:n // SEG_UNIT] = _unit_sq_host(u)
        return
    _lib.call("mi_lamb_moments", ptr(params), ptr(grads), ptr(exp_avg), ptr(exp_avg_sq), n, ptr(state), ptr(pidx),
              ptr(excl), int(unit_base), ptr(part_w), ptr(part_u), float(beta1), float(beta2), float(eps),
              float(weight_decay), stream_of(params))


def lamb_apply_(params, exp_avg, exp_avg_sq, params_bf16, state, pidx, excl, q, unit_base, beta1, beta2, eps,
                weight_decay):
    """LAMB, second launch of a segment: ``w -= lr * q * u`` with ``u`` recomputed from the stored
    moments and the still unchanged ``w`` (+ bf16 compute-copy refresh)."""
    n = params.numel()
    _check_units(n, pidx, unit_base, params, exp_avg, exp_avg_sq)
    if not params.is_cuda:
        with torch.no_grad():
            ex, qe = _unit_lookup(pidx, excl, q, unit_base, n)
            u = _lamb_u_host(params, exp_avg, exp_avg_sq, ex, state, eps, weight_decay)
            params.sub_((_f32(float(state[1])) * qe) * u)
            if params_bf16 is not None:
                params_bf16.copy_(params)
        return
    _lib.call("mi_lamb_apply", ptr(params), ptr(exp_avg), ptr(exp_avg_sq), ptr(params_bf16), n, ptr(state), ptr(pidx),
              ptr(excl), ptr(q), int(unit_base), float(beta1), float(beta2), float(eps), float(weight_decay),
              stream_of(params))


# weight averaging on the flat buffer (csrc/kernels/ema.hip, parallel/ema.py).  Device state
# block, float64:
#   [0] calls c  [1] updates n  [2] w of this call (0 = this call skips)  [3] decay
#   [4] d_t of the last call that updated
EMA_STATE_LEN = 5


def ema_prep_(state, warmup, every):
    """Advance the call counter and derive this call's weight in ``state`` (layout above), all in
    fp64::

        c += 1
        if c % every != 0:   w = 0                                       (n, d_t unchanged)
        else:  d_t = decay if warmup is None or warmup <= 0 else min(decay, (1 + n) / (warmup + n))
               w = 1 - d_t ;  n += 1

    ``decay`` is read from ``state[3]``.  No host read."""
    warmup = 0.0 if warmup is None else float(warmup)
    every = int(every)
    assert every >= 1 and state.dtype == torch.float64 and state.numel() >= EMA_STATE_LEN
    if not state.is_cuda:
        with torch.no_grad():
            c = float(state[0]) + 1.0
            state[0] = c
            if int(c) % every != 0:
                state[2] = 0.0
                return
            n, d = float(state[1]), float(state[3])
            if warmup > 0.0:
                d = min(d, (1.0 + n) / (warmup + n))
            state[1] = n + 1.0
            state[2] = 1.0 - d
            state[4] = d
        return
    _lib.call("mi_ema_prep", ptr(state), warmup, every, stream_of(state))


def ema_update_(ema, p, state):
    """``ema += w * (p - ema)`` over two fp32 buffers of any length and 4-byte alignment, with
    ``w = state[2]`` of ``ema_prep_`` rounded to fp32 (device: one fused multiply-add per element;
    host: product and sum rounded separately).  ``w == 0`` leaves ``ema`` untouched."""
    n = ema.numel()
    _check_f32(n, ema, p)
    if not ema.is_cuda:
        with torch.no_grad():
            w = float(state[2])
            if w != 0.0:
                ema.add_(torch.tensor(w, dtype=torch.float32) * (p - ema))
        return
    assert state.dtype == torch.float64 and state.numel() >= EMA_STATE_LEN
    _lib.call("mi_ema_update", ptr(ema), ptr(p), n, ptr(state), stream_of(ema))


def ema_swap_(a, b):
    """Exchange two fp32 buffers of equal length in place as 32-bit patterns (NaN payloads, signed
    zeros and denormals pass through): the exchange is its own inverse bit for bit."""
    n = a.numel()
    _check_f32(n, a, b)
    if not a.is_cuda:
        with torch.no_grad():
            ai, bi = a.view(torch.int32), b.view(torch.int32)
            t = ai.clone()
            ai.copy_(bi)
            bi.copy_(t)
        return
    _lib.call("mi_ema_swap", ptr(a), ptr(b), n, stream_of(a))


def cast_bf16_(src, dst):
    if not src.is_cuda:
        dst.copy_(src)
        return
    _lib.call("mi_cast_bf16", ptr(src), ptr(dst), src.numel(), stream_of(src))


def checksum(x: torch.Tensor) -> float:
    """Position-weighted fp64 checksum of an fp32 buffer (replica-divergence detector)."""
    if not x.is_cuda:
        idx = (torch.arange(x.numel(), dtype=torch.float64) % 7) + 1
        return float((x.double().reshape(-1) * idx).sum())
    out = torch.empty(1 + 1024, dtype=torch.float64, device=x.device)  # [0] result, [1:] block partials
    _lib.call("mi_checksum", ptr(x), x.numel(), ptr(out), stream_of(x))
    return out[:1]


# ============================================================ input pipeline
_AUG_CONST = {}


def _aug_const(dev, C, out_channels, mean, std):
    """(mean, 1 / std) as fp32 [max(Cout, C)] tensors on ``dev``: device constants built once and
    shared by the input-pipeline ops (no per-step host->device copies)."""
    key = (str(dev), max(out_channels, C), C, tuple(mean), tuple(std))
    if key not in _AUG_CONST:
        mean_t = torch.zeros(max(out_channels, C), dtype=torch.float32, device=dev)
        stdinv_t = torch.ones(max(out_channels, C), dtype=torch.float32, device=dev)
        mean_t[:C] = torch.tensor(mean, dtype=torch.float32)
        stdinv_t[:C] = 1.0 / torch.tensor(std, dtype=torch.float32)
        _AUG_CONST[key] = (mean_t, stdinv_t)
    return _AUG_CONST[key]


def augment(images_u8, out_channels, mean, std, pad=4, flip=True, seed=0, out=None):
    """uint8 NHWC [N,H,W,C] -> bf16 channels_last [N,Cout,H,W]: random crop (zero padding
    ``pad``) + horizontal flip + normalize, all on the GPU (replaces the reference's per-sample
    PIL transforms, cifar10-distributed-smddp-gpu.py:55-62).  ``out``: write into a static
    buffer (the input of a captured HIP-graph step).

    Per image n, one hash of ``(seed mod 2^32, n)`` gives offsets dy, dx in [-pad, pad] and the flip
    bit; output pixel (h, w) is source pixel (h + dy, (W - 1 - w if flipped else w) + dx), i.e. pad,
    crop at (pad + dy, pad + dx), then flip.  The border the padding adds is 0 in the output
    (filled after normalising, not (0 - mean) / std), as are channels C..Cout-1.

    Host tensors: only the normalisation, as fp32 [N,C,H,W] -- no crop, no flip, no channel fill,
    whatever ``pad``, ``flip``, ``seed`` and ``out_channels`` say."""
    N, H, W, C = images_u8.shape
    dev = images_u8.device
    mean_t, stdinv_t = _aug_const(dev, C, out_channels, mean, std)
    if not images_u8.is_cuda:
        x = images_u8.float().div(255.0).permute(0, 3, 1, 2)
        x = (x - mean_t[:C].view(1, C, 1, 1)) * stdinv_t[:C].view(1, C, 1, 1)
        return x
    if out is None:
        out = torch.empty((N, out_channels, H, W), dtype=BF16, device=dev, memory_format=CL)
    elif not (out.shape == (N, out_channels, H, W) and out.dtype == BF16 and out.is_contiguous(memory_format=CL)):
        raise ValueError("augment(out=...) needs a bf16 channels_last [N, Cout, H, W] tensor")
    _lib.call("mi_augment", ptr(images_u8.contiguous()), ptr(out), N, H, W, C, out_channels, int(pad), int(flip),
              seed & 0xFFFFFFFF, ptr(mean_t), ptr(stdinv_t), stream_of(images_u8))
    return out


def _mix_cpu(x, labels, params):
    """Host reference of the Mixup / CutMix rule on already augmented values ``x`` [N, C, H, W]."""
    N, _, H, W = x.shape
    partner, lam = params.partner.long(), params.lam.float().clone()
    ok = (partner >= 0) & (partner < N)
    partner = torch.where(ok, partner, torch.arange(N))
    lam[~ok] = 1.0
    box = params.box.long()
    y0, y1 = box[:, 0].clamp(0, H), box[:, 1].clamp(0, H)
    x0, x1 = box[:, 2].clamp(0, W), box[:, 3].clamp(0, W)
    cut = ok & (y1 > y0) & (x1 > x0)
    hh, ww = torch.arange(H).view(1, H, 1), torch.arange(W).view(1, 1, W)
    inbox = (cut.view(N, 1, 1) & (hh >= y0.view(N, 1, 1)) & (hh < y1.view(N, 1, 1))
             & (ww >= x0.view(N, 1, 1)) & (ww < x1.view(N, 1, 1))).unsqueeze(1)
    lam_px = torch.where(cut, torch.ones_like(lam), lam).view(N, 1, 1, 1)
    xb = x[partner]
    x = torch.where(inbox, xb, lam_px * x + (1 - lam_px) * xb)
    lam = torch.where(cut, 1.0 - ((y1 - y0) * (x1 - x0)).float() / float(H * W), lam)
    return x, MixedTarget(labels.long(), labels.long()[partner], lam)


def augment_mix(images_u8, labels, out_channels, mean, std, params, pad=4, flip=True, seed=0, out=None, target=None):
    """``augment`` with Mixup / CutMix folded into the same uint8 -> bf16 pass; returns
    ``(x, MixedTarget)``.

    ``params`` carries the per-sample, device-resident mixing parameters (``data.mix.BatchMixer``):
    ``partner`` int32 [N], ``lam`` fp32 [N], ``box`` int32 [N, 4] = (y0, y1, x0, x1) in output
    coordinates.  An empty box blends ``lam * a + (1 - lam) * b`` in fp32 (Mixup); a non-empty box
    takes the partner inside it and the image outside (CutMix).  Image and partner each keep the
    crop / flip that ``augment`` gives them for this ``seed``.  The kernel also writes the target:
    ``y_a = labels``, ``y_b = labels[partner]`` and the label-side lam (CutMix: 1 - clipped box
    area / (H * W)).  ``out`` / ``target``: static buffers to write into (the inputs of a captured
    HIP-graph step)."""
    N, H, W, C = images_u8.shape
    dev = images_u8.device
    if not images_u8.is_cuda:
        x = augment(images_u8, out_channels, mean, std, pad=pad, flip=flip, seed=seed)
        return _mix_cpu(x, labels, params)
    if labels.dtype != torch.int64 or labels.shape != (N,) or labels.device != dev:
        raise ValueError(f"augment_mix: labels must be an int64 [{N}] tensor on {dev}")
    partner, lam, box = params.partner, params.lam, params.box
    if not (partner.dtype == torch.int32 and partner.shape == (N,) and partner.device == dev
            and partner.is_contiguous()):
        raise ValueError(f"augment_mix: params.partner must be a contiguous int32 [{N}] tensor on {dev}")
    if not (lam.dtype == torch.float32 and lam.shape == (N,) and lam.device == dev and lam.is_contiguous()):
        raise ValueError(f"augment_mix: params.lam must be a contiguous fp32 [{N}] tensor on {dev}")
    if not (box.dtype == torch.int32 and box.shape == (N, 4) and box.device == dev and box.is_contiguous()):
        raise ValueError(f"augment_mix: params.box must be a contiguous int32 [{N}, 4] tensor on {dev}")
    mean_t, stdinv_t = _aug_const(dev, C, out_channels, mean, std)
    if out is None:
        out = torch.empty((N, out_channels, H, W), dtype=BF16, device=dev, memory_format=CL)
    elif not (out.shape == (N, out_channels, H, W) and out.dtype == BF16 and out.is_contiguous(memory_format=CL)):
        raise ValueError("augment_mix(out=...) needs a bf16 channels_last [N, Cout, H, W] tensor")
    if target is None:
        target = MixedTarget(torch.empty_like(labels), torch.empty_like(labels),
                             torch.empty(N, dtype=torch.float32, device=dev))
    else:
        for t, dt in ((target.y_a, torch.int64), (target.y_b, torch.int64), (target.lam, torch.float32)):
            if not (t.dtype == dt and t.shape == (N,) and t.device == dev and t.is_contiguous()):
                raise ValueError(f"augment_mix(target=...) needs contiguous int64 / int64 / fp32 [{N}] tensors on {dev}")
    _lib.call("mi_augment_mix", ptr(images_u8.contiguous()), ptr(out), ptr(labels.contiguous()), ptr(partner),
              ptr(lam), ptr(box), ptr(target.y_a), ptr(target.y_b), ptr(target.lam), N, H, W, C, out_channels,
              int(pad), int(flip), seed & 0xFFFFFFFF, ptr(mean_t), ptr(stdinv_t), stream_of(images_u8))
    return out, target


def _resized_cpu(images_u8, Ho, Wo, out_channels, geo, mean_t, stdinv_t):
    """Host reference of the resample of ``augment_resized``: fp32 [N, Cout, Ho, Wo]."""
    N, Hs, Ws, C = images_u8.shape
    crop, flip, erase = geo.crop.long(), geo.flip.long(), geo.erase.long()
    top, left = crop[:, 0].clamp(0, Hs - 1), crop[:, 1].clamp(0, Ws - 1)
    ch = torch.minimum(crop[:, 2].clamp(min=1), Hs - top)
    cw = torch.minimum(crop[:, 3].clamp(min=1), Ws - left)

    def axis(o, length, n_out):  # o [N, n_out], length [N] -> first tap, second tap, weight of the second
        num = ((2 * o + 1) * length[:, None] - n_out).clamp(min=0)
        i0 = num // (2 * n_out)
        return i0, torch.minimum(i0 + 1, length[:, None] - 1), (num % (2 * n_out)).float() / float(2 * n_out)

    oh = torch.arange(Ho).expand(N, Ho)
    ow = torch.arange(Wo).expand(N, Wo)
    y0, y1, ly = axis(oh, ch, Ho)
    x0, x1, lx = axis(torch.where(flip[:, None] != 0, Wo - 1 - ow, ow), cw, Wo)
    img, n = images_u8.float(), torch.arange(N).view(N, 1, 1)
    ys, xs = [(top[:, None] + y)[:, :, None] for y in (y0, y1)], [(left[:, None] + x)[:, None, :] for x in (x0, x1)]
    a, b, d, e = img[n, ys[0], xs[0]], img[n, ys[0], xs[1]], img[n, ys[1], xs[0]], img[n, ys[1], xs[1]]
    lx, ly = lx.view(N, 1, Wo, 1), ly.view(N, Ho, 1, 1)
    up, dn = a + lx * (b - a), d + lx * (e - d)
    v = (up + ly * (dn - up)).div(255.0)  # [N, Ho, Wo, C]
    v = (v - mean_t[:C]) * stdinv_t[:C]
    ey0, ey1 = erase[:, 0].clamp(0, Ho).view(N, 1, 1), erase[:, 1].clamp(0, Ho).view(N, 1, 1)
    ex0, ex1 = erase[:, 2].clamp(0, Wo).view(N, 1, 1), erase[:, 3].clamp(0, Wo).view(N, 1, 1)
    erased = (oh.view(N, Ho, 1) >= ey0) & (oh.view(N, Ho, 1) < ey1) & (ow.view(N, 1, Wo) >= ex0) & (ow.view(N, 1, Wo) < ex1)
    v = torch.where(erased.unsqueeze(-1), torch.zeros((), dtype=v.dtype), v)
    x = torch.zeros((N, max(out_channels, C), Ho, Wo), dtype=torch.float32)
    x[:, :C] = v.permute(0, 3, 1, 2)
    return x


def augment_resized(images_u8, size, out_channels, mean, std, geo, mix=None, labels=None, out=None, target=None):
    """uint8 NHWC [N,Hs,Ws,C] -> bf16 channels_last [N,Cout,Ho,Wo] through a per-image crop box and a
    bilinear resample: RandomResizedCrop, resize + centre crop and RandomErasing in ``augment``'s one
    pass (``csrc/kernels/resample.hip``).  Returns ``x``, or ``(x, MixedTarget)`` when ``mix`` is given.

    ``size`` is ``Ho`` or ``(Ho, Wo)``.  ``geo`` carries the per-image, device-resident geometry
    (``data.crops.BatchCropper``): ``crop`` int32 [N, 4] = (top, left, height, width) in source
    pixels, ``flip`` int32 [N], ``erase`` int32 [N, 4] = (y0, y1, x0, x1) in output pixels (empty: no
    erasing).  The value of an output pixel is "crop, then ``F.interpolate(mode="bilinear",
    align_corners=False, antialias=False)``", with source coordinates in exact integer arithmetic
    (a box of the output's size returns the source pixels), then the flip, ``augment``'s
    normalisation, and 0 inside the image's erase box.  Every box is clipped to its domain by the
    kernel.  ``mix`` (``data.mix.MixParams``, with ``labels`` int64 [N]) applies ``augment_mix``'s
    Mixup / CutMix rule to those values; image and partner each use their own crop, flip and erase
    box.  ``out`` / ``target``: static buffers to write into (the inputs of a captured HIP-graph step).

    Not done here: antialiased downscaling (torchvision's tensor default is ``antialias=True``; it
    matters only when the box is much larger than the output), bicubic resampling, sources of
    unequal size within one batch, RandAugment / TrivialAugment.

    Host tensors take a torch implementation of the same semantics (fp32 output)."""
    N, Hs, Ws, C = images_u8.shape
    Ho, Wo = (int(size), int(size)) if isinstance(size, int) else (int(size[0]), int(size[1]))
    dev = images_u8.device
    if (mix is None) != (labels is None):
        raise ValueError("augment_resized: mix and labels go together")
    mean_t, stdinv_t = _aug_const(dev, C, out_channels, mean, std)
    if not images_u8.is_cuda:
        x = _resized_cpu(images_u8, Ho, Wo, out_channels, geo, mean_t, stdinv_t)
        return x if mix is None else _mix_cpu(x, labels, mix)
    crop, flip, erase = geo.crop, geo.flip, geo.erase
    for name, t, shape in (("crop", crop, (N, 4)), ("flip", flip, (N,)), ("erase", erase, (N, 4))):
        if not (t.dtype == torch.int32 and t.shape == shape and t.device == dev and t.is_contiguous()):
            raise ValueError(f"augment_resized: geo.{name} must be a contiguous int32 {list(shape)} tensor on {dev}")
    if out is None:
        out = torch.empty((N, out_channels, Ho, Wo), dtype=BF16, device=dev, memory_format=CL)
    elif not (out.shape == (N, out_channels, Ho, Wo) and out.dtype == BF16 and out.is_contiguous(memory_format=CL)):
        raise ValueError("augment_resized(out=...) needs a bf16 channels_last [N, Cout, Ho, Wo] tensor")
    if mix is None:
        if target is not None:
            raise ValueError("augment_resized(target=...) needs mix")
        mix_args = (ptr(None),) * 7
    else:
        if labels.dtype != torch.int64 or labels.shape != (N,) or labels.device != dev:
            raise ValueError(f"augment_resized: labels must be an int64 [{N}] tensor on {dev}")
        partner, lam, box = mix.partner, mix.lam, mix.box
        if not (partner.dtype == torch.int32 and partner.shape == (N,) and partner.device == dev
                and partner.is_contiguous()):
            raise ValueError(f"augment_resized: mix.partner must be a contiguous int32 [{N}] tensor on {dev}")
        if not (lam.dtype == torch.float32 and lam.shape == (N,) and lam.device == dev and lam.is_contiguous()):
            raise ValueError(f"augment_resized: mix.lam must be a contiguous fp32 [{N}] tensor on {dev}")
        if not (box.dtype == torch.int32 and box.shape == (N, 4) and box.device == dev and box.is_contiguous()):
            raise ValueError(f"augment_resized: mix.box must be a contiguous int32 [{N}, 4] tensor on {dev}")
        if target is None:
            target = MixedTarget(torch.empty_like(labels), torch.empty_like(labels),
                                 torch.empty(N, dtype=torch.float32, device=dev))
        else:
            for t, dt in ((target.y_a, torch.int64), (target.y_b, torch.int64), (target.lam, torch.float32)):
                if not (t.dtype == dt and t.shape == (N,) and t.device == dev and t.is_contiguous()):
                    raise ValueError(
                        f"augment_resized(target=...) needs contiguous int64 / int64 / fp32 [{N}] tensors on {dev}")
        mix_args = (ptr(labels.contiguous()), ptr(partner), ptr(lam), ptr(box), ptr(target.y_a), ptr(target.y_b),
                    ptr(target.lam))
    _lib.call("mi_augment_resized", ptr(images_u8.contiguous()), ptr(out), ptr(crop), ptr(flip), ptr(erase), *mix_args,
              N, Hs, Ws, Ho, Wo, C, out_channels, ptr(mean_t), ptr(stdinv_t), stream_of(images_u8))
    return out if mix is None else (out, target)
