"""Shared by test_misc_reference_cpu.py and test_misc_kernels_gpu.py: host references, in fp64, of
the operations in csrc/kernels/misc.hip (and the fp32-mode pooling kernels of fp32.hip) -- the input
pipeline's crop / flip / normalize, max pool, global average pool, hard-label cross entropy, the flat
SGD update and the stem's im2col -- with the accuracy rules the GPU tests apply.

Nothing here follows the kernels' index arithmetic: images are built from ``F.pad``, slicing and
``flip``; pooling comes from ``F.max_pool2d`` and a scatter; im2col from ``F.unfold``.  The one
thing copied from a kernel is the per-image random draw (``draw``), because the kernel's stream of
random numbers is part of its contract (reproducible from ``(seed, image index)``, no state)."""
import torch
import torch.nn.functional as F

BF = torch.bfloat16
F64 = torch.float64
SWEEP = 8192 * 256  # work items one pass of the capped element-wise grids covers (ew_grid)


# ------------------------------------------------------------------------------- bf16 helpers
def bf16_ulp_diff(a, b):
    """distance between two bf16 tensors in units of the last place (0 and -0 coincide)"""
    def key(t):
        bits = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(bits < 0, -(bits & 0x7FFF), bits)
    assert a.dtype == BF and b.dtype == BF and a.shape == b.shape
    return (key(a) - key(b)).abs()


# ------------------------------------------------------------------------- augment: the draw
def hash32(x: int) -> int:
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    x ^= x >> 16
    return x


def draw(seed: int, n: int, pad: int, flip: bool):
    """(dy, dx, flip) of image ``n``: offsets in [-pad, pad], all from one hash of (seed, n) in
    uint32 arithmetic.  Only the low 32 bits of ``seed`` count."""
    hv = hash32(((seed & 0xFFFFFFFF) * 0x9E3779B9 + n) & 0xFFFFFFFF)
    dy = dx = 0
    if pad > 0:
        dy = hv % (2 * pad + 1) - pad
        dx = (hv >> 8) % (2 * pad + 1) - pad
    return dy, dx, bool((hv >> 20) & 1) if flip else False


# ------------------------------------------------------------------ augment: the composition
def compose(img_u8, dy, dx, fl, pad, out_channels, mean, std):
    """One image, uint8 [H, W, C] -> bf16 [Cout, H, W], in the transform order of
    RandomCrop(padding) -> RandomHorizontalFlip -> ToTensor -> Normalize:
      1. ``F.pad`` by ``pad`` with zeros   2. crop H x W at (pad + dy, pad + dx)   3. ``flip(-1)``
      4. (u8 / 255 - mean) / std in fp64, rounded to bf16   5. zero channels up to ``Cout``.
    The border the padding adds is zero in the *output*: ``augment`` fills with 0 after normalising,
    where torchvision's pipeline would give (0 - mean) / std.  The validity mask that travels with
    the image through steps 1-3 expresses that."""
    H, W, C = img_u8.shape
    x = img_u8.permute(2, 0, 1).to(F64)
    valid = torch.ones(1, H, W, dtype=F64)
    x, valid = (F.pad(t, (pad, pad, pad, pad)) for t in (x, valid))
    top, left = pad + dy, pad + dx
    x, valid = (t[:, top:top + H, left:left + W] for t in (x, valid))
    if fl:
        x, valid = x.flip(-1), valid.flip(-1)
    m = torch.tensor(mean, dtype=F64).view(C, 1, 1)
    s = torch.tensor(std, dtype=F64).view(C, 1, 1)
    x = (x / 255.0 - m) / s * valid
    out = torch.zeros(out_channels, H, W, dtype=F64)
    out[:C] = x
    return out.to(BF)


def augment_reference(images_u8, out_channels, mean, std, pad, flip, seed, first=0):
    """uint8 [N, H, W, C] (host) -> bf16 [N, Cout, H, W]; ``first``: index of images_u8[0] in the
    batch the kernel saw (to check a slice of a large batch)"""
    imgs = images_u8.cpu()
    return torch.stack([compose(imgs[i], *draw(seed, first + i, pad, flip), pad, out_channels, mean, std)
                        for i in range(imgs.shape[0])])


def check_augment(out, ref, what=""):
    """zeros of the reference (border, channel fill) exactly zero, everything else within 1 bf16 ulp
    (the kernel multiplies by fp32 1/255 and 1/std where the reference divides in fp64); returns
    (largest ulp distance, number of elements that differ)"""
    out = out.detach().cpu().contiguous()
    assert out.dtype == BF and out.shape == ref.shape, (out.dtype, out.shape, ref.shape)
    zero = ref == 0
    assert bool((out[zero] == 0).all()), f"{what}: nonzero where the reference is zero"
    assert bool((out[~zero] != 0).all()), f"{what}: zero where the reference is not"
    d = bf16_ulp_diff(out, ref)
    worst, count = int(d.max()) if d.numel() else 0, int((d > 0).sum())
    print(f"{what}: max ulp distance {worst}, {count} of {d.numel()} elements differ")
    assert worst <= 1, f"{what}: {worst} bf16 ulps from the reference"
    return worst, count


def position_coded(N, size=8):
    """uint8 [N, size, size, 1] with pixel value 16 * row + col: an output pixel names its source"""
    r = torch.arange(size).view(size, 1)
    c = torch.arange(size).view(1, size)
    return (16 * r + c).to(torch.uint8).view(1, size, size, 1).repeat(N, 1, 1, 1)


POS_MEAN, POS_STD = (0.0,), (1.0 / 255.0,)  # (v / 255 - 0) * 255: the output is the pixel value itself


def decode_positions(out, pad):
    """``augment`` outputs [N, 1, S, S] of position_coded images -> the (dy, dx, flip) each image
    shows, found by matching it against all (2 pad + 1)^2 * 2 compositions; every image must
    match exactly one"""
    out = out.detach().cpu().float().reshape(out.shape[0], -1)
    size = int(round(out.shape[1] ** 0.5))
    img = position_coded(1, size)[0]
    combos = [(dy, dx, fl) for dy in range(-pad, pad + 1) for dx in range(-pad, pad + 1) for fl in (False, True)]
    cand = torch.stack([compose(img, dy, dx, fl, pad, 1, POS_MEAN, POS_STD).float().reshape(-1)
                        for dy, dx, fl in combos])
    match = (out[:, None, :] == cand[None, :, :]).all(-1)  # [N, combos]
    assert bool((match.sum(1) == 1).all()), "an output image is not exactly one crop/flip of its source"
    return [combos[i] for i in match.int().argmax(1).tolist()]


# ---------------------------------------------------------------------------------- max pool
# (H, W, k, stride, pad): overlapping 3/2/1 on odd and even sizes, stride 1, non-overlapping 2/2/0,
# no padding, k > 2 s, a 5 x 5 image, H != W, and 8 x 8 with 3/2/0, whose last row and column no
# window covers
POOL_GEOMS = [(9, 9, 3, 2, 1), (7, 7, 3, 1, 1), (8, 8, 2, 2, 0), (9, 9, 3, 2, 0), (11, 11, 5, 3, 2), (5, 5, 3, 2, 1),
              (9, 12, 3, 2, 1), (8, 8, 3, 2, 0)]
POOL_N, POOL_CHANNELS = 2, (8, 24)


def pool_out(h, k, s, pad):
    return (h + 2 * pad - k) // s + 1


def pool_inputs(geom, C, integer, seed=0, N=POOL_N):
    """(x, dy) in fp64, NCHW, exactly representable in bf16.  ``integer``: x in [-3, 3], dy in
    [-8, 8] -- plenty of ties for the maximum, and every gradient sum stays below 256 in
    magnitude (at most k * k <= 25 windows x 8 = 200), so a correct kernel is bit-exact."""
    H, W, k, s, pad = geom
    g = torch.Generator().manual_seed(1000 * seed + 10 * H + W + k + C)
    P, Q = pool_out(H, k, s, pad), pool_out(W, k, s, pad)
    if integer:
        x = torch.randint(-3, 4, (N, C, H, W), generator=g).to(F64)
        dy = torch.randint(-8, 9, (N, C, P, Q), generator=g).to(F64)
    else:
        x = torch.randn(N, C, H, W, generator=g).to(BF).to(F64)
        dy = torch.randn(N, C, P, Q, generator=g).to(BF).to(F64)
    return x, dy


def maxpool_reference(x, dy, k, s, pad):
    """(y, dx) of ``F.max_pool2d`` in fp64: dx scatters dy to the indices torch returns"""
    y, idx = F.max_pool2d(x, k, s, pad, return_indices=True)
    N, C, H, W = x.shape
    dx = torch.zeros(N, C, H * W, dtype=F64)
    dx.scatter_add_(2, idx.reshape(N, C, -1), dy.reshape(N, C, -1))
    return y, dx.view(N, C, H, W), idx


def _windows(x, k, s, pad):
    """[N, C, P, Q, k * k] windows in scan order (row by row), -inf outside the image"""
    xp = F.pad(x, (pad, pad, pad, pad), value=float("-inf"))
    win = xp.unfold(2, k, s).unfold(3, k, s)
    return win.reshape(*win.shape[:4], k * k)


def first_max_indices(x, k, s, pad):
    """flat input index (h * W + w) of the FIRST maximum of every window in scan order"""
    N, C, H, W = x.shape
    win = _windows(x, k, s, pad)
    is_max = win == win.max(-1, keepdim=True).values
    first = is_max & (is_max.cumsum(-1) == 1)
    tap = (first * torch.arange(k * k)).sum(-1)
    P, Q = win.shape[2], win.shape[3]
    h = torch.arange(P).view(1, 1, P, 1) * s - pad + tap // k
    w = torch.arange(Q).view(1, 1, 1, Q) * s - pad + tap % k
    return h * W + w


def tie_share(x, k, s, pad):
    """share of windows whose maximum occurs more than once"""
    win = _windows(x, k, s, pad)
    return float(((win == win.max(-1, keepdim=True).values).sum(-1) > 1).double().mean())


# ----------------------------------------------------------------------- global average pool
# (HW, C, N): N * C / 8 is no multiple of the 256-thread block except at C = 2048, where C / 8 = 256
# makes every N one
GAP_CASES = [(1, 8, 3), (49, 2048, 2), (3136, 64, 5), (9, 24, 7)]
GAP_BWD_SWEEP_CASE = (3136, 64, 85)  # 85 * 3136 * 8 = 2,132,480 octets > SWEEP


def gap_inputs(HW, C, N, dtype=BF):
    g = torch.Generator().manual_seed(HW + C + N)
    x = torch.randn(N, C, HW, 1, generator=g).to(dtype).to(F64)
    dy = torch.randn(N, C, generator=g).to(dtype).to(F64)
    return x, dy


def gap_forward_bound(x):
    """per-element bound of the bf16 kernel's forward: half a bf16 ulp of the result (2^-8 |ref|) plus
    the bound of a sequential fp32 sum of HW terms, HW * 2^-24 * mean|x|.  Returns (ref, bound)."""
    HW = x.shape[2] * x.shape[3]
    ref = x.mean((2, 3))
    return ref, 2.0 ** -8 * ref.abs() + HW * 2.0 ** -24 * x.abs().mean((2, 3))


# ------------------------------------------------------------------- hard-label cross entropy
CE_SHAPES = [(3, 10), (1, 1), (2, 257), (300, 1000), (5, 64)]
F32_TINY = float(torch.finfo(torch.float32).tiny)  # smallest normal fp32 (and bf16) magnitude


def ce_inputs(N, C, dtype):
    """logits already rounded to ``dtype`` and labels that include class 0 and class C - 1"""
    g = torch.Generator().manual_seed(N * 1009 + C)
    lg = (torch.randn(N, C, generator=g) * 3).to(dtype)
    y = torch.randint(0, C, (N,), generator=g)
    y[0], y[-1] = 0, C - 1
    return lg, y


def ce_reference(lg, y, gout=1.0):
    """``F.cross_entropy`` in fp64 on the given (already rounded) logits: (loss, gout * dloss/dlogits)"""
    r = lg.detach().cpu().to(F64).requires_grad_()
    loss = F.cross_entropy(r, y.cpu())
    (loss * gout).backward()
    return float(loss.detach()), r.grad


def row_rel_err(got, ref):
    """worst row of max|got - ref| / max|ref| per ROW: a small-magnitude row that is entirely wrong
    shows, where a batch-wide maximum would hide it.  A row whose exact gradient lies below the
    smallest normal fp32 number cannot be represented in either gradient dtype and is measured
    against that floor."""
    got, ref = got.detach().cpu().to(F64), ref.detach().cpu().to(F64)
    err = (got - ref).abs().max(1).values / ref.abs().max(1).values.clamp_min(F32_TINY)
    return float(err.max())


# ------------------------------------------------------------------------------------ flat SGD
# (momentum, dampening, weight_decay, nesterov, first_step)
SGD_CONFIGS = [(0.0, 0.0, 0.0, False, False), (0.9, 0.0, 0.0, False, True), (0.9, 0.1, 5e-4, False, True),
               (0.9, 0.1, 5e-4, False, False), (0.9, 0.0, 1e-4, True, False)]
SGD_SIZES = [1, 255, 257, 2 ** 21 + 2 ** 20 + 3]
# Learning rate of the one-step test.  The bound below is stated for p; applied to buf it has to
# cover the buffer's own roundings, which at an element with p ~ 0 are those of
# b = mu * buf + (1 - dampening) * d: half an ulp each of d, of 1 - dampening, of the product and of
# b, at most 2^-24 * 3.4 * M with M = |g scale| + wd |p| + mu |buf|.  S >= lr (1 + mu) M, so
# 2^-21 S covers that for every correct fp32 evaluation once 8 * lr * 1.9 >= 3.4, i.e. lr >= 0.23.
SGD_LR = 0.4


def f32(v) -> float:
    """a Python scalar rounded to fp32, as the launcher hands it to the kernel"""
    return float(torch.tensor(v, dtype=torch.float32))


def sgd_reference(p, g, buf, lr, momentum, dampening, wd, nesterov, first, grad_scale):
    """fp64 evaluation of one ``sgd_flat_`` step (the formula of its host branch) from fp32 state,
    with the scalars rounded to fp32 first because that is what the kernel is given.  Returns
    (p_new, buf_new, bound): per element |result - ref| <= 2^-21 * S,
    S = |p| + lr (1 + mu) (|g scale| + wd |p| + mu |buf|) -- fewer than eight fp32 roundings, eight
    half-ulps of the magnitudes involved; the same bound for p and buf."""
    lr, momentum, dampening, wd, grad_scale = (f32(v) for v in (lr, momentum, dampening, wd, grad_scale))
    p, g, buf = (t.detach().cpu().to(F64) for t in (p, g, buf))
    S = p.abs() + lr * (1 + momentum) * ((g * grad_scale).abs() + wd * p.abs() + momentum * buf.abs())
    d = g * grad_scale
    if wd:
        d = d + wd * p
    if momentum:
        buf = d.clone() if first else momentum * buf + (1 - dampening) * d
        d = d + momentum * buf if nesterov else buf
    return p - lr * d, buf, 2.0 ** -21 * S


# ------------------------------------------------------------------------------------- im2col
IM2COL_GEOMS = [(3, 7, 2, 3, 30), (3, 3, 1, 1, 9), (5, 2, 2, 0, 8)]  # (C, R, stride, pad, H)


def im2col_reference(x, R, S, stride, pad, Kp):
    """[N, C, H, W] -> [N * P * Q, Kp] with k = (r * S + s) * C + c, zero for k >= R * S * C and in
    the padding: ``F.unfold`` (k = (c * R + r) * S + s) permuted"""
    N, C, H, W = x.shape
    P, Q = pool_out(H, R, stride, pad), pool_out(W, S, stride, pad)
    u = F.unfold(x.to(F64), (R, S), padding=pad, stride=stride)  # [N, C * R * S, P * Q]
    u = u.view(N, C, R, S, P * Q).permute(0, 4, 2, 3, 1).reshape(N * P * Q, R * S * C)
    col = torch.zeros(N * P * Q, Kp, dtype=F64)
    col[:, :R * S * C] = u
    return col
