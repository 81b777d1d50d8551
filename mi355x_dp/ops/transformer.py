"""Transformer (ViT-B/16) ops on the native gfx950 kernels.

``encoder_layer`` runs one pre-LN encoder block (torchvision ``EncoderBlock`` semantics:
``y = x + proj(attn(ln_1(x)))``, ``z = y + fc2(gelu(fc1(ln_2(y))))``) as ONE autograd node
with an explicit backward, so every elementwise op rides on a kernel that runs anyway:

  forward                                   backward
  ln_1            mi_layernorm_fwd          dz -> fc2: TN(dW2 + db2), NT+gelu' epilogue -> du
  qkv = h1 Wqkvᵀ  NT (+bias)                du -> fc1: TN(dW1 + db1), NT -> dh2
  attention       attention kernel          dy = dz + ln_2ᵀ(dh2)       (LN bwd, residual add fused)
  y = x + o Woᵀ   NT, residual epilogue     dy -> proj: TN(+bias), NT -> do -> attention bwd -> dqkv
  ln_2            mi_layernorm_fwd          dqkv -> TN(+bias), NT -> dh1
  g = gelu(h2W1ᵀ) NT, GELU epilogue         dx = dy + ln_1ᵀ(dh1)       (LN bwd, residual add fused)
                  (+ gelu' kept for the backward's epilogue, which only multiplies by it)
  z = y + g W2ᵀ   NT, residual epilogue

No torch elementwise kernels, no autograd-inserted residual-gradient adds, and the bias
gradients are column sums of the bf16 gradient computed by the weight-gradient GEMM itself (an
extra MFMA against a ones operand on fragments it already holds -- no second pass over dY).
The data-gradient GEMMs read the flat engine's cached transposed weights.  Weight gradients go
straight into the flat fp32 gradient buffer of the DP engine (``functional._grad_buffer``).

Regularisation inside the layer (``encoder_layer(..., drop=LayerDrop(...))``): hidden dropout and
stochastic depth (drop-path, row mode) are modes of the same epilogues -- ``y = x + m * (o Woᵀ + b)``
with ``m`` = element mask x per-sample mask, ``g = m * gelu(.)`` with ``gelu'`` stored already masked --
drawn by a counter-based generator (Philox4x32-10, ``csrc/kernels/philox.h``) from
(seed, rank, step, site, position), so the backward recomputes them (``mi_drop_bwd``) and no mask is
saved.  ``DropState`` owns seed and step on the device.

Reference: the ViT-B/16 config is a BASELINE.json target (config 5), not part of the
reference repo; semantics follow torchvision ``vision_transformer.EncoderBlock``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from . import kernels as _k  # noqa: F401
from ._lib import ptr, stream_of
from .functional import BF16, _finish_grad, _grad_buffer, _side, linear_weight_t, weight_bf16

F32 = torch.float32
EPI_NONE, EPI_GELU, EPI_GELU_BWD, EPI_RESIDUAL = 0, 1, 2, 3


# ------------------------------------------------------------------ primitives
def _ln_fwd(x2, w, b, eps):
    M, D = x2.shape
    y = torch.empty_like(x2)
    mean = torch.empty(M, dtype=F32, device=x2.device)
    rstd = torch.empty(M, dtype=F32, device=x2.device)
    _lib.call("mi_layernorm_fwd", ptr(x2), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), M, D, float(eps),
              stream_of(x2))
    return y, mean, rstd


def _ln_bwd(dy2, x2, w, b, mean, rstd, dres=None):
    """dx (+dres), and dW / dB accumulated into the parameters' gradient sinks."""
    M, D = x2.shape
    dx = torch.empty_like(x2)
    gw, gb = _grad_buffer(w), _grad_buffer(b)
    _lib.call("mi_layernorm_bwd", ptr(dy2), ptr(x2), ptr(w), ptr(mean), ptr(rstd), ptr(dres), ptr(dx), ptr(gw),
              ptr(gb), M, D, stream_of(x2))
    return dx, _finish_grad(w, gw), _finish_grad(b, gb)


def _gemm(a2, w16, bias=None, epi=EPI_NONE, aux=None):
    """bf16 out[M][N] = a2[M][K] · w16[N][K]ᵀ (+bias) with the fused epilogue ``epi``."""
    M, K = a2.shape
    N = w16.shape[0]
    out = torch.empty((M, N), dtype=BF16, device=a2.device)
    if epi == EPI_GELU:
        aux = torch.empty((M, N), dtype=BF16, device=a2.device)
    _lib.call("mi_gemm_nt_epi", ptr(a2), ptr(w16), ptr(out), ptr(bias), ptr(aux), epi, M, N, K, K, K, N,
              stream_of(a2))
    return (out, aux) if epi == EPI_GELU else out


def _wbgrad(weight, bias, dy2, x2):
    """weight AND bias gradient from one TN GEMM (the bias column sums ride on its A fragments) --
    on the engine's weight-gradient stream when it has one (functional.WgradStream), overlapping
    the layer's data-gradient chain."""
    g, gb = _grad_buffer(weight), _grad_buffer(bias)
    M, N = dy2.shape
    K = x2.shape[1]

    def launch():
        _lib.call("mi_gemm_tn_bias", ptr(dy2), ptr(x2), ptr(g), ptr(gb), N, K, M, N, K, K, stream_of(dy2))
    side = _side(weight)
    if side is not None and _side(bias) is not None:
        cw, cb = getattr(weight, "_mi_on_grad_ready", None), getattr(bias, "_mi_on_grad_ready", None)

        def ready():
            for c in (cw, cb):
                if c is not None:
                    c()
        side.run(launch, (dy2, x2), ready)
        return None, None
    launch()
    return _finish_grad(weight, g), _finish_grad(bias, gb)


# Plain data-gradient GEMMs (no fused epilogue: the qkv / proj / fc1 input gradients) run on the
# native 256x256 kernel like every other GEMM of the step.  MI355X_DP_BLAS_DGRAD=1 routes them to
# the library GEMM (hipBLASLt) instead: 1.1-1.4x faster on these N = 768 shapes in isolation
# (profiles/vit_r3_gemm_attention.md) but only +1.8 % on the whole ViT-B/16 step
# (profiles/raw/r4_vit_{lib,native}.log: 6,307 vs 6,196 img/s), so the all-native step is the default.
import os as _os
BLAS_DGRAD = _os.environ.get("MI355X_DP_BLAS_DGRAD", "0") == "1"


def _dgrad(dy2, weight, epi=EPI_NONE, aux=None):
    """dX[M][K] = dY[M][N] · W[N][K] (NT against the transposed bf16 weight, cached by the flat
    engine once per optimizer step)."""
    if epi == EPI_NONE and BLAS_DGRAD:
        return torch.matmul(dy2, weight_bf16(weight))
    return _gemm(dy2, linear_weight_t(weight), None, epi, aux)


# ------------------------------------------------------------------ dropout / stochastic depth
# mask sites of layer l: 8 l + kind (the embedding dropout: layer = num_layers, kind 0)
SITE_ATTN_DROP, SITE_GELU_DROP, SITE_MLP_DROP, SITE_ATTN_PATH, SITE_MLP_PATH = range(5)
DROP_RESIDUAL, DROP_GELU = 1, 2  # kinds of the dropped GEMM epilogues


def drop_threshold(p) -> int:
    """``thr = round(p * 65536)`` of the keep rule ``r >= thr`` on 16-bit draws; 0: the site is
    inactive.  ``ValueError`` outside ``0 <= p < 1``."""
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"drop probability must be in [0, 1), got {p}")
    return min(int(p * 65536.0 + 0.5), 65535)


def _default_rank() -> int:
    import torch.distributed as dist
    return dist.get_rank() if dist.is_available() and dist.is_initialized() else 0


class DropState:
    """Seed and step of the dropout / stochastic-depth masks.  On the GPU they live in a device
    block of two 64-bit words that the kernels read through a pointer and a one-thread native kernel
    advances, so a captured graph draws new masks on every replay.  ``rank`` (default: the process
    group's, resolved at first use; 0 without one) goes into the counter, so ranks draw different
    masks from one seed.  Not a module: it never appears in a model's ``state_dict()``;
    ``utils.checkpoint`` stores ``state_dict()`` beside it."""

    def __init__(self, seed=0, rank=None):
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        self._rank = None if rank is None else self._check_rank(rank)
        self._step = 0
        self._block = None

    @staticmethod
    def _check_rank(rank):
        rank = int(rank)
        if not 0 <= rank < 65536:
            raise ValueError(f"rank must be in [0, 65536), got {rank}")
        return rank

    @property
    def seed(self) -> int:
        return self._seed

    @property
    def rank(self) -> int:
        if self._rank is None:
            self._rank = self._check_rank(_default_rank())
        return self._rank

    @property
    def step(self) -> int:
        if self._block is not None:
            self._step = int(self._block[1].item())
        return self._step

    @step.setter
    def step(self, value):
        self._step = int(value)
        if self._block is not None:
            self._block[1] = self._step

    def reseed(self, seed, rank=None):
        """New seed (and rank); the step restarts at 0."""
        self._seed = int(seed) & 0xFFFFFFFFFFFFFFFF
        if rank is not None:
            self._rank = self._check_rank(rank)
        self._step = 0
        self._block = None

    def block(self, device):
        """The live device block ``[seed, step]`` (int64) on ``device``."""
        device = torch.device(device)
        if self._block is None or self._block.device != device:
            step = self.step
            s = self._seed - (1 << 64) if self._seed >= (1 << 63) else self._seed
            self._block = torch.tensor([s, step], dtype=torch.int64, device=device)
        return self._block

    def _advance(self, device, inc, snapshot):
        blk = self.block(device)
        snap = torch.empty(2, dtype=torch.int64, device=blk.device) if snapshot else None
        _lib.call("mi_drop_state_advance", ptr(blk), ptr(snap), inc, stream_of(blk))
        return snap

    def advance(self, device=None, snapshot=False):
        """step += 1 (on the device when the block lives there).  ``snapshot=True`` returns a copy of
        the advanced block: what the kernels of one forward / backward pair read, whatever advances
        later."""
        if device is None and self._block is not None:
            device = self._block.device
        if device is None or torch.device(device).type != "cuda":  # host only: nothing on a device reads it
            self._step = self.step + 1
            return None
        return self._advance(device, 1, snapshot)

    def snapshot(self, device):
        """A copy of the current block, without advancing."""
        return self._advance(device, 0, True)

    def state_dict(self):
        return {"seed": self._seed, "rank": self.rank, "step": self.step}

    def load_state_dict(self, sd):
        """Restores seed and step.  The rank stays this process's own (a checkpoint is written by
        rank 0 and read by every rank)."""
        self._seed = int(sd["seed"]) & 0xFFFFFFFFFFFFFFFF
        self._step = int(sd["step"])
        self._block = None


class LayerDrop:
    """Regularisation of one fused encoder layer: ``dropout`` (hidden dropout after out_proj, GELU
    and fc2) and ``stochastic_depth`` (row mode, both residual branches) of layer ``layer``, masks
    drawn from ``state`` (a ``DropState``).  ``snap``: the block copy of this forward
    (``DropState.advance(snapshot=True)``), shared by the layers of one model forward; without it
    the layer takes its own copy of the current block."""
    __slots__ = ("state", "layer", "dropout", "stochastic_depth", "snap")

    def __init__(self, state, layer, dropout=0.0, stochastic_depth=0.0, snap=None):
        self.state, self.layer, self.snap = state, int(layer), snap
        self.dropout, self.stochastic_depth = float(dropout), float(stochastic_depth)


class _Drop:
    """A LayerDrop resolved for one call: thresholds, site base, rank and the block copy."""
    __slots__ = ("snap", "rank", "base", "thr_e", "thr_r")

    def site(self, kind):
        return self.base + kind


def _resolve_drop(drop, device):
    if drop is None:
        return None
    thr_e, thr_r = drop_threshold(drop.dropout), drop_threshold(drop.stochastic_depth)
    if thr_e == 0 and thr_r == 0:
        return None
    if not 0 <= 8 * drop.layer + 7 < 65536:
        raise ValueError(f"layer index {drop.layer} is outside the mask site range")
    d = _Drop()
    d.snap = drop.snap if drop.snap is not None else drop.state.snapshot(device)
    d.rank, d.base, d.thr_e, d.thr_r = drop.state.rank, 8 * drop.layer, thr_e, thr_r
    return d


def _gemm_drop(a2, w16, bias, kind, aux, d, site_e, thr_e, site_r=0, thr_r=0, rows_per_sample=1):
    """``_gemm`` with a dropped epilogue: DROP_RESIDUAL out = (a2 w16ᵀ + bias) * m + aux, DROP_GELU
    out = gelu(.) * m and gelu'(.) * m; m = element mask (thr_e, site_e) x per-sample mask (thr_r, site_r)."""
    M, K = a2.shape
    N = w16.shape[0]
    out = torch.empty((M, N), dtype=BF16, device=a2.device)
    if kind == DROP_GELU:
        aux = torch.empty((M, N), dtype=BF16, device=a2.device)
    _lib.call("mi_gemm_nt_epi_drop", ptr(a2), ptr(w16), ptr(out), ptr(bias), ptr(aux), kind, M, N, K, K, K, N,
              ptr(d.snap), thr_e, site_e, thr_r, site_r, d.rank, rows_per_sample, stream_of(a2))
    return (out, aux) if kind == DROP_GELU else out


def _drop_bwd(dz2, d, site_e, thr_e, site_r, thr_r, rows_per_sample):
    """bf16(dz * m): the gradient a dropped residual branch hands to its GEMMs (the masks recomputed)."""
    M, N = dz2.shape
    out = torch.empty_like(dz2)
    _lib.call("mi_drop_bwd", ptr(dz2), ptr(out), M, N, ptr(d.snap), thr_e, site_e, thr_r, site_r, d.rank,
              rows_per_sample, stream_of(dz2))
    return out


def drop_mask(M, N, state_block, rank, site_e=0, thr_e=0, site_r=0, thr_r=0, rows_per_sample=1):
    """fp32 [M][N] multiplier matrix of a site, from the kernels' own device function (tests, debugging)."""
    out = torch.empty((M, N), dtype=F32, device=state_block.device)
    _lib.call("mi_drop_mask", ptr(out), M, N, ptr(state_block), thr_e, site_e, thr_r, site_r, rank, rows_per_sample,
              stream_of(out))
    return out


# ------------------------------------------------------------------ attention
ATT_RESIDENT_MAX = 256  # mi_attn_fwd / mi_attn_bwd: the head's whole K, V (Q, dO) in LDS
_ATT_LONG_MAX = []


def _att_long_max():
    """Longest sequence of the slab-streaming kernels (mi_attn_fwd_long / mi_attn_bwd_long).
    MI355X_DP_ATT_LONG=0 (read at call time, for A/B runs) switches them off: T > 256 then takes the
    SDPA fallback as it did before they existed."""
    if _os.environ.get("MI355X_DP_ATT_LONG", "1") == "0":
        return ATT_RESIDENT_MAX
    if not _ATT_LONG_MAX:
        _ATT_LONG_MAX.append(int(_lib.load().mi_attn_long_max_seq()))
    return _ATT_LONG_MAX[0]


def native_attention_ok(T, head_dim):
    if head_dim != 64 or T <= 0:
        return False
    return T <= ATT_RESIDENT_MAX or T <= _att_long_max()


_SDPA_WARNED = set()


def _warn_sdpa(T, Dh):
    """The native kernels cover head dim 64 at any sequence length the long kernels take (T <= 256:
    operands resident in LDS, ViT-B/16 at 224²; above: streamed in slabs, e.g. 577 tokens at 384²);
    anything else runs torch's scaled_dot_product_attention -- said once per shape, so a non-native
    path is never silent.  MI355X_DP_STRICT_NATIVE=1 makes it an error instead."""
    if _os.environ.get("MI355X_DP_STRICT_NATIVE", "0") == "1":
        raise RuntimeError(f"attention: no native kernel for T={T}, head_dim={Dh} (MI355X_DP_STRICT_NATIVE=1)")
    if (T, Dh) not in _SDPA_WARNED:
        _SDPA_WARNED.add((T, Dh))
        import warnings
        warnings.warn(f"mi355x_dp attention: T={T}, head_dim={Dh} is outside the native kernels "
                      f"(head_dim 64, T <= {_att_long_max()}; MI355X_DP_ATT_LONG=0 keeps T <= 256); using torch "
                      f"scaled_dot_product_attention", stacklevel=3)


def _attn_fwd(qkv2, B, T, H, need_grad):
    """softmax(q kᵀ/√d) v over the packed [B·T][3·H·Dh] projection; returns o [B·T][H·Dh].
    Native kernels (csrc/kernels/attention.hip) for Dh = 64: T <= 256 on the resident-operand
    kernels (ViT-B/16 at 224²: T = 197), longer sequences on the slab-streaming pair."""
    D3 = qkv2.shape[1]
    Dh = D3 // (3 * H)
    scale = 1.0 / (Dh ** 0.5)
    if native_attention_ok(T, Dh):
        o = torch.empty((B * T, H * Dh), dtype=BF16, device=qkv2.device)
        lse = torch.empty((B * H * T,), dtype=F32, device=qkv2.device)
        fn = "mi_attn_fwd" if T <= ATT_RESIDENT_MAX else "mi_attn_fwd_long"
        _lib.call(fn, ptr(qkv2), ptr(o), ptr(lse), B, T, H, float(scale), stream_of(qkv2))
        return o, (("native", lse, o) if need_grad else None)
    _warn_sdpa(T, Dh)
    if not need_grad:
        q, k, v = qkv2.view(B, T, 3, H, Dh).permute(2, 0, 3, 1, 4).unbind(0)
        o4 = F.scaled_dot_product_attention(q, k, v)
        return o4.transpose(1, 2).reshape(B * T, H * Dh), None
    with torch.enable_grad():
        leaf = qkv2.detach().requires_grad_()
        q, k, v = leaf.view(B, T, 3, H, Dh).permute(2, 0, 3, 1, 4).unbind(0)
        o4 = F.scaled_dot_product_attention(q, k, v)
    return o4.detach().transpose(1, 2).reshape(B * T, H * Dh), ("sdpa", leaf, o4)


def _attn_bwd(state, qkv2, do2, B, T, H):
    Dh = do2.shape[1] // H
    if state[0] == "native":
        _, lse, o = state
        dqkv = torch.empty_like(qkv2)
        dvec = torch.empty((B * H * T,), dtype=F32, device=qkv2.device)
        fn = "mi_attn_bwd" if T <= ATT_RESIDENT_MAX else "mi_attn_bwd_long"
        _lib.call(fn, ptr(qkv2), ptr(o), ptr(do2), ptr(lse), ptr(dvec), ptr(dqkv), B, T, H,
                  float(1.0 / (Dh ** 0.5)), stream_of(qkv2))
        return dqkv
    _, leaf, o4 = state
    (dqkv,) = torch.autograd.grad(o4, leaf, do2.view(B, T, H, Dh).transpose(1, 2))
    return dqkv.contiguous()


def attention(qkv2, B, T, H):
    """Differentiable packed-QKV attention (standalone use / tests)."""
    return _Attention.apply(qkv2, B, T, H)


class _Attention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv2, B, T, H):
        qkv2 = qkv2.to(BF16).contiguous()
        o, state = _attn_fwd(qkv2, B, T, H, True)
        ctx.state = state
        ctx.dims = (B, T, H)
        ctx.save_for_backward(qkv2)
        return o

    @staticmethod
    def backward(ctx, do):
        (qkv2,) = ctx.saved_tensors
        B, T, H = ctx.dims
        dqkv = _attn_bwd(ctx.state, qkv2, do.to(BF16).contiguous(), B, T, H)
        ctx.state = None
        return dqkv, None, None, None


# ------------------------------------------------------------------ encoder layer
PARAM_ORDER = ("ln_1.weight", "ln_1.bias", "self_attention.in_proj_weight", "self_attention.in_proj_bias",
               "self_attention.out_proj.weight", "self_attention.out_proj.bias", "ln_2.weight", "ln_2.bias",
               "mlp.0.weight", "mlp.0.bias", "mlp.3.weight", "mlp.3.bias")


def _layer_forward(x2, B, T, heads, eps, params, need_grad, d=None):
    ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2 = params
    h1, m1, r1 = _ln_fwd(x2, ln1w, ln1b, eps)
    qkv = _gemm(h1, weight_bf16(wqkv), bqkv)
    o, attn = _attn_fwd(qkv, B, T, heads, need_grad)
    if d is None:
        y = _gemm(o, weight_bf16(wo), bo, EPI_RESIDUAL, x2)
    else:
        y = _gemm_drop(o, weight_bf16(wo), bo, DROP_RESIDUAL, x2, d, d.site(SITE_ATTN_DROP), d.thr_e,
                       d.site(SITE_ATTN_PATH), d.thr_r, T)
    h2, m2, r2 = _ln_fwd(y, ln2w, ln2b, eps)
    # u = gelu'(pre-activation) (x the dropout mask): all the backward needs
    if d is None or d.thr_e == 0:
        g, u = _gemm(h2, weight_bf16(w1), b1, EPI_GELU)
    else:
        g, u = _gemm_drop(h2, weight_bf16(w1), b1, DROP_GELU, None, d, d.site(SITE_GELU_DROP), d.thr_e)
    if d is None:
        z = _gemm(g, weight_bf16(w2), b2, EPI_RESIDUAL, y)
    else:
        z = _gemm_drop(g, weight_bf16(w2), b2, DROP_RESIDUAL, y, d, d.site(SITE_MLP_DROP), d.thr_e,
                       d.site(SITE_MLP_PATH), d.thr_r, T)
    saved = (x2, h1, m1, r1, qkv, o, y, h2, m2, r2, u, g) if need_grad else None
    return z, saved, attn


class _EncoderLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, heads, eps, d, *params):
        B, T, D = x.shape
        x2 = x.reshape(B * T, D)
        if x2.dtype != BF16:
            x2 = x2.to(BF16)
        x2 = x2.contiguous()
        z, saved, attn = _layer_forward(x2, B, T, heads, eps, params, True, d)
        ctx.save_for_backward(*saved, *params)
        ctx.attn = attn
        ctx.drop = d  # thresholds, sites and this forward's block copy: the backward redraws the masks
        ctx.dims = (B, T, D, heads)
        ctx.in_dtype = x.dtype
        return z.view(B, T, D)

    @staticmethod
    def backward(ctx, dz):
        B, T, D, heads = ctx.dims
        (x2, h1, m1, r1, qkv, o, y, h2, m2, r2, u, g, ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2,
         b2) = ctx.saved_tensors
        dz2 = dz.reshape(B * T, D)
        if dz2.dtype != BF16:
            dz2 = dz2.to(BF16)
        dz2 = dz2.contiguous()
        d = ctx.drop
        ctx.drop = None
        # MLP (a dropped branch's GEMMs see the masked gradient; the residual path keeps dz)
        dzm = dz2 if d is None else _drop_bwd(dz2, d, d.site(SITE_MLP_DROP), d.thr_e, d.site(SITE_MLP_PATH),
                                              d.thr_r, T)
        d_w2, d_b2 = _wbgrad(w2, b2, dzm, g)
        du = _dgrad(dzm, w2, EPI_GELU_BWD, u)
        d_w1, d_b1 = _wbgrad(w1, b1, du, h2)
        dh2 = _dgrad(du, w1)
        dy, d_ln2w, d_ln2b = _ln_bwd(dh2, y, ln2w, ln2b, m2, r2, dres=dz2)
        # attention
        dym = dy if d is None else _drop_bwd(dy, d, d.site(SITE_ATTN_DROP), d.thr_e, d.site(SITE_ATTN_PATH),
                                             d.thr_r, T)
        d_wo, d_bo = _wbgrad(wo, bo, dym, o)
        do = _dgrad(dym, wo)
        dqkv = _attn_bwd(ctx.attn, qkv, do, B, T, heads)
        ctx.attn = None
        d_wqkv, d_bqkv = _wbgrad(wqkv, bqkv, dqkv, h1)
        dh1 = _dgrad(dqkv, wqkv)
        dx, d_ln1w, d_ln1b = _ln_bwd(dh1, x2, ln1w, ln1b, m1, r1, dres=dy)
        dx = dx.view(B, T, D)
        if ctx.in_dtype != BF16:
            dx = dx.to(ctx.in_dtype)
        return (dx, None, None, None, d_ln1w, d_ln1b, d_wqkv, d_bqkv, d_wo, d_bo, d_ln2w, d_ln2b, d_w1, d_b1, d_w2,
                d_b2)


def encoder_layer(x, heads, eps, params, drop=None):
    """x [B, T, D] (cuda) -> [B, T, D] bf16.  ``params`` in ``PARAM_ORDER``.  ``drop``: a ``LayerDrop``
    (hidden dropout / stochastic depth of a training forward); ``None`` or all probabilities 0: the
    launches are those of the plain layer."""
    d = _resolve_drop(drop, x.device)
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
        return _EncoderLayer.apply(x, heads, eps, d, *params)
    B, T, D = x.shape
    x2 = x.reshape(B * T, D).to(BF16).contiguous()
    z, _, _ = _layer_forward(x2, B, T, heads, eps, params, False, d)
    return z.view(B, T, D)


# ------------------------------------------------------------------ standalone LayerNorm
class _LayerNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if x2.dtype != BF16:
            x2 = x2.to(BF16)
        x2 = x2.contiguous()
        y, mean, rstd = _ln_fwd(x2, w, b, eps)
        ctx.save_for_backward(x2, w, b, mean, rstd)
        ctx.shape = shape
        ctx.in_dtype = x.dtype
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, b, mean, rstd = ctx.saved_tensors
        dy2 = dy.reshape(x2.shape)
        if dy2.dtype != BF16:
            dy2 = dy2.to(BF16)
        dx, dw, db = _ln_bwd(dy2.contiguous(), x2, w, b, mean, rstd)
        dx = dx.view(ctx.shape)
        if ctx.in_dtype != BF16:
            dx = dx.to(ctx.in_dtype)
        return dx, dw, db, None


class _PatchEmbed(torch.autograd.Function):
    """Stride = kernel = p patch embedding as patchify + one plain GEMM: the NHWC input's real
    channels C are gathered into [patches][p * p * C] rows in (r, s, c) order -- the flat engine's
    [K][R][S][C] conv weight layout, so the weight and its gradient are used as [K][p * p * C]
    matrices in place -- instead of the 8-channel-padded implicit-GEMM conv (K = 768 instead of 2048
    for ViT-B/16).  Returns [N][patches][K] bf16; no input gradient (images)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        N, Cs, H, W = x.shape
        K, C, R, S = weight.shape
        Kd = R * S * C
        rows = N * (H // R) * (W // S)
        st = stream_of(x)
        xp = torch.empty((rows, Kd), dtype=BF16, device=x.device)
        _lib.call("mi_vit_patchify", ptr(x), ptr(xp), N, H, W, Cs, C, R, st)
        w2 = weight_bf16(weight).permute(0, 2, 3, 1)
        w2 = w2.reshape(K, Kd) if w2.is_contiguous() else w2.contiguous().reshape(K, Kd)
        y = torch.empty((rows, K), dtype=BF16, device=x.device)
        _lib.call("mi_gemm_nt", ptr(xp), ptr(w2), ptr(y), ptr(bias), ptr(None), rows, K, Kd, Kd, Kd, K, 0, 0, st)
        ctx.save_for_backward(xp)
        ctx.params = (weight, bias)
        return y.view(N, rows // N, K)

    @staticmethod
    def backward(ctx, dy):
        (xp,) = ctx.saved_tensors
        weight, bias = ctx.params
        rows, Kd = xp.shape
        K = weight.shape[0]
        dy2 = dy.reshape(rows, K).to(BF16).contiguous()
        st = stream_of(dy2)
        dw = db = None
        if ctx.needs_input_grad[1]:
            g = _grad_buffer(weight)
            g2 = g.permute(0, 2, 3, 1)  # [K][R][S][C]: contiguous in the kernel layout
            tmp = None if g2.is_contiguous() else torch.zeros(g2.shape, dtype=F32, device=g.device)
            _lib.call("mi_gemm_tn", ptr(dy2), ptr(xp), ptr(g2 if tmp is None else tmp), K, Kd, rows, K, Kd, Kd, st)
            if tmp is not None:
                g2.add_(tmp)
            dw = _finish_grad(weight, g)
        if bias is not None and ctx.needs_input_grad[2]:
            gb = _grad_buffer(bias)
            _lib.call("mi_colsum_bf16", ptr(dy2), ptr(gb), rows, K, K, st)
            db = _finish_grad(bias, gb)
        return None, dw, db


def patch_embed_ok(x, conv) -> bool:
    K, C, R, S = conv.weight.shape
    return (x.is_cuda and x.dtype == BF16 and x.is_contiguous(memory_format=torch.channels_last)
            and tuple(conv.stride) == (R, S) and R == S and tuple(conv.padding) == (0, 0) and conv.groups == 1
            and C <= x.shape[1] and (R * S * C) % 8 == 0 and K % 8 == 0 and x.shape[2] % R == 0
            and x.shape[3] % S == 0 and conv.weight.dtype == torch.float32)


def patch_embed(x, conv):
    """[N][patches][K] bf16 embedding of the NHWC bf16 image batch ``x`` by the stride-p conv ``conv``."""
    return _PatchEmbed.apply(x, conv.weight, conv.bias)


class _VitEmbed(torch.autograd.Function):
    """[class token ; patch embeddings] + position embedding as one native pass
    (``mi_vit_embed_fwd``); backward: the patches' dense gradient plus the fixed-order batch sums
    for the position embedding and the class token (``mi_vit_embed_bwd``) -- no concatenation,
    broadcast-add, cast or reduction launches.  ``drop`` = (block copy, rank, site, threshold): the
    embedding dropout folded into both passes (the backward redraws the mask)."""

    @staticmethod
    def forward(ctx, patches, cls, pos, drop=None):
        N, P, D = patches.shape
        T = P + 1
        p = patches.contiguous()
        out = torch.empty((N, T, D), dtype=BF16, device=p.device)
        if drop is None:
            _lib.call("mi_vit_embed_fwd", ptr(p), ptr(cls), ptr(pos), ptr(out), N, T, D, stream_of(p))
        else:
            snap, rank, site, thr = drop
            _lib.call("mi_vit_embed_fwd_drop", ptr(p), ptr(cls), ptr(pos), ptr(out), N, T, D, ptr(snap), thr, site,
                      rank, stream_of(p))
        ctx.drop = drop
        ctx.params = (cls, pos)
        ctx.shape = (N, T, D)
        return out

    @staticmethod
    def backward(ctx, dout):
        cls, pos = ctx.params
        N, T, D = ctx.shape
        d = dout.to(BF16).contiguous()
        dp = torch.empty((N, T - 1, D), dtype=BF16, device=d.device)
        gpos = _grad_buffer(pos) if ctx.needs_input_grad[2] else None
        gcls = _grad_buffer(cls) if ctx.needs_input_grad[1] else None
        part = torch.empty(int(_lib.load().mi_vit_embed_bwd_part_floats(N, T, D)), dtype=F32, device=d.device)
        if ctx.drop is None:
            _lib.call("mi_vit_embed_bwd", ptr(d), ptr(dp), ptr(gpos), ptr(gcls), ptr(part), N, T, D, stream_of(d))
        else:
            snap, rank, site, thr = ctx.drop
            _lib.call("mi_vit_embed_bwd_drop", ptr(d), ptr(dp), ptr(gpos), ptr(gcls), ptr(part), N, T, D, ptr(snap),
                      thr, site, rank, stream_of(d))
        dcls = _finish_grad(cls, gcls) if gcls is not None else None
        dpos = _finish_grad(pos, gpos) if gpos is not None else None
        return dp, dcls, dpos, None


def vit_embed(patches, cls, pos, drop=None):
    """bf16 [N][T][D] tokens = cat(cls, patches) + pos for fp32 ``cls`` [1,1,D] / ``pos`` [1,T,D].
    ``drop`` = (state, snap, layer, p): the embedding dropout (site 8 * layer, element mask) of a
    training forward, folded into the pass."""
    if drop is not None:
        state, snap, layer, p = drop
        thr = drop_threshold(p)
        drop = None if thr == 0 else (snap if snap is not None else state.snapshot(patches.device), state.rank,
                                      8 * layer + SITE_ATTN_DROP, thr)
    return _VitEmbed.apply(patches, cls, pos, drop)


def layer_norm(x, weight, bias, eps):
    """Native LayerNorm over the last dim (bf16 out, fp32 affine parameters)."""
    return _LayerNorm.apply(x, weight, bias, eps)
