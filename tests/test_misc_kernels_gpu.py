"""The kernels of csrc/kernels/misc.hip -- the input pipeline's crop / flip / normalize, max pool,
global average pool, hard-label cross entropy, the flat SGD update, the bf16 cast and add, the stem's
im2col -- and the fp32-mode pooling kernels of fp32.hip, each against the fp64 host reference of
misc_reference.py: at the geometries, channel counts, seeds and scalar settings where such kernels
go wrong, and past one pass of the capped element-wise grid (8192 blocks x 256 threads), where the
grid-stride loops take their second trip.  Measured worst cases: profiles/misc_kernel_tests.md."""
import pytest
import torch

import misc_reference as mr
from misc_reference import BF, F64, SWEEP

pytestmark = pytest.mark.gpu
CL = torch.channels_last
DEV = "cuda"


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mi355x_dp.ops import _lib
    _lib.load(True)  # fail loudly if the extension is missing


@pytest.fixture
def fp32_mode(monkeypatch):
    from mi355x_dp.ops import fp32
    monkeypatch.setattr(fp32, "COMPUTE_FP32", True)
    return fp32


# ================================================================================== 1. augment
MEAN, STD = (0.4914, 0.4822, 0.4465, 0.5), (0.2023, 0.1994, 0.2010, 0.25)
AUG_SEEDS = [0, 3, 2 ** 31, 2 ** 32 - 1]
# Cout == 8 takes the one-store-per-pixel path, everything else the per-channel path
AUG_CHANNELS = [(3, 3), (3, 8), (3, 4), (1, 1), (1, 8), (4, 8)]


def _images(N, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (N, H, W, C), dtype=torch.uint8, generator=g)


@pytest.mark.parametrize("flip", [False, True], ids=["noflip", "flip"])
@pytest.mark.parametrize("pad", [0, 1, 4])
@pytest.mark.parametrize("C,Cout", AUG_CHANNELS)
def test_augment_matches_composition(C, Cout, pad, flip):
    """a non-square 9 x 11 batch against pad -> crop -> flip -> normalize -> channel fill"""
    from mi355x_dp.ops import augment
    u8 = _images(6, 9, 11, C, seed=C + Cout)
    dev = u8.to(DEV)
    for seed in AUG_SEEDS:
        out = augment(dev, Cout, MEAN[:C], STD[:C], pad=pad, flip=flip, seed=seed)
        assert out.shape == (6, Cout, 9, 11) and out.is_contiguous(memory_format=CL)
        ref = mr.augment_reference(u8, Cout, MEAN[:C], STD[:C], pad, flip, seed)
        mr.check_augment(out, ref, f"C={C} Cout={Cout} pad={pad} flip={flip} seed={seed}")
    # the out= form: same bits, written in place (sentinel-filled first)
    static = torch.full((6, Cout, 9, 11), 7.0, dtype=BF, device=DEV).contiguous(memory_format=CL)
    back = augment(dev, Cout, MEAN[:C], STD[:C], pad=pad, flip=flip, seed=AUG_SEEDS[-1], out=static)
    assert back is static and torch.equal(static, out)


def test_augment_seed_is_taken_mod_2_32():
    from mi355x_dp.ops import augment
    dev = _images(16, 9, 11, 3).to(DEV)
    a = augment(dev, 8, MEAN[:3], STD[:3], pad=4, flip=True, seed=5)
    b = augment(dev, 8, MEAN[:3], STD[:3], pad=4, flip=True, seed=2 ** 32 + 5)
    c = augment(dev, 8, MEAN[:3], STD[:3], pad=4, flip=True, seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)


@pytest.mark.parametrize("seed,Cout", [(0, 1), (3, 1), (17, 1), (2 ** 31, 1), (2 ** 32 - 1, 1), (17, 8)])
def test_augment_position_coded_coverage(seed, Cout):
    """pixel value = 16 row + col on 8 x 8: the output itself says which crop and flip produced it.
    Every image is exactly one of the 162 compositions, the one the draw names, and at N = 2048 all
    162 occur (so every offset from -pad to +pad and both flip states are reached)."""
    from mi355x_dp.ops import augment
    N, pad = 2048, 4
    out = augment(mr.position_coded(N).to(DEV), Cout, mr.POS_MEAN, mr.POS_STD, pad=pad, flip=True, seed=seed)
    assert not out[:, 1:].any()
    got = mr.decode_positions(out[:, :1], pad)
    assert got == [mr.draw(seed, n, pad, True) for n in range(N)]
    assert len(set(got)) == 162


def test_augment_second_grid_stride_trip():
    """2048 images of 32 x 33: 2,162,688 pixels, more than one pass of the capped grid; the pixels of
    the second trip are in the last 62 images"""
    from mi355x_dp.ops import augment
    N, H, W = 2048, 32, 33
    assert N * H * W > SWEEP
    u8 = _images(N, H, W, 3, seed=9)
    out = augment(u8.to(DEV), 8, MEAN[:3], STD[:3], pad=4, flip=True, seed=3)
    mr.check_augment(out[-64:], mr.augment_reference(u8[-64:], 8, MEAN[:3], STD[:3], 4, True, 3, first=N - 64),
                     "last 64 images")
    mr.check_augment(out[:8], mr.augment_reference(u8[:8], 8, MEAN[:3], STD[:3], 4, True, 3), "first 8 images")


# ================================================================================== 2. pooling
def _pool_on_gpu(op, x, dy, k, s, pad, dtype):
    xc = x.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    y = op(xc, k, s, pad)
    assert y.dtype == dtype and y.is_contiguous(memory_format=CL)
    y.backward(dy.to(dtype).to(DEV).contiguous(memory_format=CL))
    assert xc.grad.dtype == dtype
    return y.detach().cpu(), xc.grad.cpu()


def _pool_op(dtype, fp32_mode):
    if dtype == torch.float32:
        return fp32_mode.max_pool2d
    from mi355x_dp.ops import max_pool2d
    return max_pool2d


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32mode"])
@pytest.mark.parametrize("C", mr.POOL_CHANNELS)
@pytest.mark.parametrize("geom", mr.POOL_GEOMS)
def test_maxpool_exact_on_integer_data(fp32_mode, geom, C, dtype):
    """integers in [-3, 3] (gradients in [-8, 8]): every value and every sum is exact in bf16, so y
    and dx must equal ``F.max_pool2d``'s bit for bit -- including which of several equal maxima
    (the first in scan order) receives the gradient"""
    H, W, k, s, pad = geom
    x, dy = mr.pool_inputs(geom, C, integer=True)
    assert mr.tie_share(x, k, s, pad) >= 0.15  # a condition on the inputs, not on the kernel
    y_ref, dx_ref, _ = mr.maxpool_reference(x, dy, k, s, pad)
    y, dx = _pool_on_gpu(_pool_op(dtype, fp32_mode), x, dy, k, s, pad, dtype)
    assert torch.equal(y.to(F64), y_ref), "y"
    assert torch.equal(dx.to(F64), dx_ref), "dx"


@pytest.mark.parametrize("dtype", [BF, torch.float32], ids=["bf16", "fp32mode"])
@pytest.mark.parametrize("C", mr.POOL_CHANNELS)
@pytest.mark.parametrize("geom", mr.POOL_GEOMS)
def test_maxpool_randn(fp32_mode, geom, C, dtype):
    """non-integer data: y exact; dx within 1 bf16 ulp of the fp64 sum rounded to bf16 (fp32 mode:
    1e-6 of the largest gradient, test_f32_pool_and_linear's tolerance)"""
    H, W, k, s, pad = geom
    x, dy = mr.pool_inputs(geom, C, integer=False)
    y_ref, dx_ref, _ = mr.maxpool_reference(x, dy, k, s, pad)
    y, dx = _pool_on_gpu(_pool_op(dtype, fp32_mode), x, dy, k, s, pad, dtype)
    assert torch.equal(y.to(F64), y_ref), "y"
    if dtype == BF:
        assert int(mr.bf16_ulp_diff(dx.contiguous(), dx_ref.to(BF)).max()) <= 1
    else:
        assert float((dx.to(F64) - dx_ref).abs().max() / dx_ref.abs().max()) < 1e-6


def test_maxpool_rejects_channels_not_a_multiple_of_8():
    from mi355x_dp.ops import max_pool2d
    x = torch.zeros(2, 12, 9, 9, dtype=BF, device=DEV).contiguous(memory_format=CL)
    with pytest.raises(RuntimeError, match="mi_maxpool_fwd"):
        max_pool2d(x, 3, 2, 1)
    torch.cuda.synchronize()


def _check_pool_images(x, y, dx, dy, images, k, s, pad):
    for n in images:
        y_ref, dx_ref, _ = mr.maxpool_reference(x[n:n + 1].cpu().to(F64), dy[n:n + 1].cpu().to(F64), k, s, pad)
        assert torch.equal(y[n:n + 1].cpu().to(F64), y_ref), f"y of image {n}"
        assert torch.equal(dx[n:n + 1].cpu().to(F64), dx_ref), f"dx of image {n}"


@pytest.mark.parametrize("dtype,shape", [(BF, (32, 64, 224)), (torch.float32, (11, 64, 112))], ids=["bf16", "fp32mode"])
def test_maxpool_second_grid_stride_trip(fp32_mode, dtype, shape):
    """3/2/1 with more forward work items than one pass of the capped grid (bf16: N P Q C / 8 =
    3,211,264; fp32: N P Q C = 2,207,744), the backward several passes.  Integer data, exact; the
    first image and the last two (second trip and beyond) are compared."""
    N, C, H = shape
    P = mr.pool_out(H, 3, 2, 1)
    assert N * P * P * (C // 8 if dtype == BF else C) > SWEEP
    g = torch.Generator(device=DEV).manual_seed(11)
    # built as NHWC and viewed as NCHW: channels_last without a second copy
    x = torch.randint(-3, 4, (N, H, H, C), dtype=torch.int8, device=DEV, generator=g).to(dtype).permute(0, 3, 1, 2)
    dy = torch.randint(-8, 9, (N, P, P, C), dtype=torch.int8, device=DEV, generator=g).to(dtype).permute(0, 3, 1, 2)
    x.requires_grad_()
    y = _pool_op(dtype, fp32_mode)(x, 3, 2, 1)
    y.backward(dy)
    try:
        _check_pool_images(x.detach(), y.detach(), x.grad, dy, (0, N - 2, N - 1), 3, 2, 1)
    finally:
        del x, y, dy
        torch.cuda.empty_cache()


def _gap_on_gpu(op, x, dy, dtype):
    xc = x.to(dtype).to(DEV).contiguous(memory_format=CL).requires_grad_()
    y = op(xc)
    assert y.dtype == dtype and y.shape == dy.shape
    y.backward(dy.to(dtype).to(DEV))
    return y.detach().cpu(), xc.grad.cpu()


@pytest.mark.parametrize("HW,C,N", mr.GAP_CASES + [mr.GAP_BWD_SWEEP_CASE])
def test_global_avg_pool_bf16(HW, C, N):
    """forward: |y - ref| <= 2^-8 |ref| + HW 2^-24 mean|x| per element (half a bf16 ulp plus the
    sequential fp32 sum); backward: dy / HW rounded to bf16, within 1 ulp.  The last case's backward
    covers 2,132,480 octets, more than one pass of the capped grid."""
    from mi355x_dp.ops import global_avg_pool
    x, dy = mr.gap_inputs(HW, C, N)
    ref, bound = mr.gap_forward_bound(x)
    y, dx = _gap_on_gpu(global_avg_pool, x, dy, BF)
    ratio = float(((y.to(F64) - ref).abs() / bound).max())
    dx_ref = (dy / HW).to(BF).view(N, C, 1, 1).expand(N, C, HW, 1)
    ulps = int(mr.bf16_ulp_diff(dx.contiguous(), dx_ref.contiguous()).max())
    print(f"gap HW={HW} C={C} N={N}: worst |y - ref| / bound {ratio:.3f}, dx max ulp distance {ulps}")
    assert ratio <= 1.0
    assert ulps <= 1


@pytest.mark.parametrize("HW,C,N", mr.GAP_CASES + [mr.GAP_BWD_SWEEP_CASE])
def test_global_avg_pool_fp32_mode(fp32_mode, HW, C, N):
    """fp32 mode against fp64, 1e-6 of the largest value (test_f32_pool_and_linear's tolerance)"""
    x, dy = mr.gap_inputs(HW, C, N, torch.float32)
    y, dx = _gap_on_gpu(fp32_mode.global_avg_pool, x, dy, torch.float32)
    ref = x.mean((2, 3))
    dx_ref = (dy / HW).view(N, C, 1, 1).expand(N, C, HW, 1)
    ey = float((y.to(F64) - ref).abs().max() / ref.abs().max())
    ex = float((dx.to(F64) - dx_ref).abs().max() / dx_ref.abs().max())
    print(f"gap fp32 HW={HW} C={C} N={N}: y rel err {ey:.2e}, dx rel err {ex:.2e}")
    assert ey < 1e-6 and ex < 1e-6


# ================================================================= 3. hard-label cross entropy
def _check_ce(lg, y, gout=2.0, what=""):
    """loss within 1e-4 max(1, |ref|) and gradient within 1e-2 per row (test_loss_mix_gpu's
    _check_loss, the gradient normalised row by row) of fp64 on the same rounded logits"""
    from mi355x_dp.ops import cross_entropy
    a = lg.to(DEV).requires_grad_()
    loss = cross_entropy(a, y.to(DEV))
    assert type(loss.grad_fn).__name__ == "_CrossEntropyBackward"  # the eps == 0 kernels, not loss.hip's
    (loss * gout).backward()
    ref_loss, ref_grad = mr.ce_reference(lg, y, gout)
    assert loss.dtype == torch.float32 and a.grad.dtype == lg.dtype and a.grad.shape == lg.shape
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(a.grad).all())
    err_l, err_g = abs(float(loss.detach()) - ref_loss), mr.row_rel_err(a.grad, ref_grad)
    print(f"ce {what}: loss {float(loss.detach()):.7f} ref {ref_loss:.7f} |d| {err_l:.2e} "
          f"worst row grad err {err_g:.2e}")
    assert err_l < 1e-4 * max(1.0, abs(ref_loss))
    assert err_g < 1e-2
    return loss.detach(), a.grad


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,C", mr.CE_SHAPES)
def test_cross_entropy_hard_labels(N, C, dtype):
    lg, y = mr.ce_inputs(N, C, dtype)
    _check_ce(lg, y, what=f"[{N}, {C}] {dtype}")


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_cross_entropy_extreme_and_constant_rows(dtype):
    """one logit at +80 and the rest at -80, the label on the +80 (loss 0) and off it (loss 160), in
    both orders; a constant row (loss log C); an ordinary row so the batch mean mixes magnitudes"""
    C = 10
    lg = torch.full((6, C), -80.0)
    lg[0, 2] = lg[1, 7] = lg[2, 0] = lg[3, C - 1] = 80.0
    y = torch.tensor([2, 3, C - 1, C - 1, 4, 0])  # row 1: label before the peak; row 2: after it
    lg[4] = 1.25
    lg[5] = torch.randn(C, generator=torch.Generator().manual_seed(0)) * 3
    loss, _ = _check_ce(lg.to(dtype), y, what=f"extreme rows {dtype}")
    const = torch.full((3, 257), -7.5)
    ref = float(torch.log(torch.tensor(257.0, dtype=F64)))
    loss, _ = _check_ce(const.to(dtype), torch.tensor([0, 256, 100]), what=f"constant rows {dtype}")
    assert abs(float(loss) - ref) < 1e-4 * ref


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
def test_cross_entropy_upstream_gradient_and_repeatability(dtype):
    lg, y = mr.ce_inputs(300, 1000, dtype)
    l1, g1 = _check_ce(lg, y, gout=2.0, what="gout 2")
    l2, g2 = _check_ce(lg, y, gout=2.0, what="gout 2 again")
    assert torch.equal(l1, l2) and torch.equal(g1, g2)  # bit-identical runs
    _, g0 = _check_ce(lg, y, gout=0.0, what="gout 0")
    assert not g0.any()


# ======================================================== 4. sgd_flat, cast_bf16, add_bf16, im2col
GUARD = 8


def _guarded(values, dtype=torch.float32, fill=7.0):
    whole = torch.full((GUARD + values.numel() + GUARD,), fill, dtype=dtype, device=DEV)
    view = whole[GUARD:GUARD + values.numel()]
    view.copy_(values)
    return whole, view


def _intact(whole, fill=7.0):
    return bool((whole[:GUARD] == fill).all()) and bool((whole[-GUARD:] == fill).all())


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("with_p16", [True, False], ids=["p16", "nop16"])
@pytest.mark.parametrize("cfg", mr.SGD_CONFIGS)
def test_sgd_flat_one_step(cfg, with_p16, grad_scale):
    """one step from identical fp32 state against the fp64 formula, per element within
    2^-21 (|p| + lr (1 + mu) (|g scale| + wd |p| + mu |buf|)) for p and for buf; the bf16 copy is the
    rounded master; momentum == 0 leaves the buffer alone.  The largest size takes the second trip
    of the grid-stride loop."""
    from mi355x_dp.ops import sgd_flat_
    momentum, dampening, wd, nesterov, first = cfg
    for n in mr.SGD_SIZES:
        g = torch.Generator().manual_seed(n % 1000)
        p0, gr, buf0 = (torch.randn(n, generator=g) for _ in range(3))
        p0[:n // 64] *= 1e-4  # parameters near zero: there the bound rests on its gradient term
        p_ref, buf_ref, bound = mr.sgd_reference(p0, gr, buf0, mr.SGD_LR, momentum, dampening, wd, nesterov, first,
                                                 grad_scale)
        (pw, p), (gw, gd), (bw, buf) = _guarded(p0), _guarded(gr), _guarded(buf0)
        p16w, p16 = _guarded(torch.zeros(n), BF) if with_p16 else (None, None)
        sgd_flat_(p, gd, buf, p16, mr.SGD_LR, momentum, dampening, wd, nesterov, first_step=first,
                  grad_scale=grad_scale)
        torch.cuda.synchronize()
        rp = float(((p.cpu().to(F64) - p_ref).abs() / bound).max())
        rb = float(((buf.cpu().to(F64) - buf_ref).abs() / bound).max())
        print(f"sgd {cfg} scale {grad_scale} n={n}: worst |p - ref| / bound {rp:.3f}, buf {rb:.3f}")
        assert rp <= 1.0, f"n={n}: p off by {rp:.2f} x the bound"
        assert rb <= 1.0, f"n={n}: buf off by {rb:.2f} x the bound"
        assert torch.equal(gd.cpu(), gr), "the gradient was written to"
        if not momentum:
            assert torch.equal(buf.cpu(), buf0), "momentum == 0 must not touch the buffer"
        if with_p16:
            assert torch.equal(p16, p.to(BF)), "bf16 copy differs from the master"
            assert _intact(p16w)
        assert _intact(pw) and _intact(gw) and _intact(bw), "wrote outside the n elements"


@pytest.mark.parametrize("n", mr.SGD_SIZES)
def test_cast_bf16_matches_torch(n):
    from mi355x_dp.ops import cast_bf16_
    src = torch.randn(n, generator=torch.Generator().manual_seed(n % 1000))
    whole, dst = _guarded(torch.zeros(n), BF)
    cast_bf16_(src.to(DEV), dst)
    assert torch.equal(dst.cpu(), src.to(BF)) and _intact(whole)


def test_cast_bf16_rounding_edges():
    """ties to even in both directions, signed zeros and infinities, overflow of the largest finite
    fp32 to inf, NaNs (also one whose payload sits only in the bits the cast drops) stay NaN"""
    from mi355x_dp.ops import cast_bf16_
    fmax = float(torch.finfo(torch.float32).max)
    inf = float("inf")
    vals = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8), 0.0, -0.0, inf, -inf, fmax, -fmax,
            1 + 2.0 ** -8 + 2.0 ** -20]
    want = [1.0, 1 + 2.0 ** -6, -1.0, -(1 + 2.0 ** -6), 0.0, -0.0, inf, -inf, inf, -inf, 1 + 2.0 ** -7]
    src = torch.tensor(vals + [float("nan"), 0.0], dtype=torch.float32)
    src.view(torch.int32)[-1] = 0x7F800001  # a NaN whose payload is in the low 16 bits only
    dst = torch.empty(src.numel(), dtype=BF, device=DEV)
    cast_bf16_(src.to(DEV), dst)
    dst = dst.cpu()
    expect = torch.tensor(want, dtype=F64).to(BF)
    assert torch.equal(expect.to(F64), torch.tensor(want, dtype=F64))  # the hand values are bf16 numbers
    assert torch.equal(dst[:len(want)].view(torch.int16), expect.view(torch.int16)), (dst, expect)
    assert bool(torch.isnan(dst[len(want):]).all())
    assert torch.equal(dst[:len(want)].view(torch.int16), src[:len(want)].to(BF).view(torch.int16))


@pytest.mark.parametrize("n", [8, 8 * 257, 8 * (SWEEP + 5)])
def test_add_bf16(n):
    """the fp32 sum of two bf16 vectors rounded to bf16; the largest size exceeds one pass of the grid"""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    g = torch.Generator(device=DEV).manual_seed(n % 1000)
    a = torch.randn(n, device=DEV, generator=g).to(BF)
    b = (torch.randn(n, device=DEV, generator=g) * 4).to(BF)
    whole, out = _guarded(torch.zeros(n), BF)
    _lib.call("mi_add_bf16", ptr(a), ptr(b), ptr(out), n, stream_of(a))
    assert torch.equal(out.cpu(), (a.cpu().float() + b.cpu().float()).to(BF)) and _intact(whole)
    with pytest.raises(RuntimeError, match="mi_add_bf16"):
        _lib.call("mi_add_bf16", ptr(a), ptr(b), ptr(out), 7, stream_of(a))


@pytest.mark.parametrize("N,dW", [(2, 0), (2, 3), (62, 0)], ids=["square", "wide", "sweep"])
@pytest.mark.parametrize("C,R,stride,pad,H", mr.IM2COL_GEOMS)
def test_im2col(C, R, stride, pad, H, N, dW):
    """pure data movement: equal to ``F.unfold`` permuted to k = (r S + s) C + c, exact zeros in the
    padding and for k >= R S C.  N = 62 at the stem's 7/2/3 on 30 x 30 is 2,120,400 elements, more
    than one pass of the grid."""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    W = H + dW
    P, Q = mr.pool_out(H, R, stride, pad), mr.pool_out(W, R, stride, pad)
    Kp = (R * R * C + 7) // 8 * 8
    x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(C + R + H)).to(BF)
    assert bool((x != 0).all())
    xc = x.to(DEV).contiguous(memory_format=CL)
    whole, col = _guarded(torch.zeros(N * P * Q * Kp), BF)
    col.fill_(5.0)
    _lib.call("mi_im2col", ptr(xc), ptr(col), N, H, W, C, R, R, stride, pad, P, Q, Kp, stream_of(xc))
    ref = mr.im2col_reference(x, R, R, stride, pad, Kp)
    assert torch.equal(col.cpu().to(F64).view(N * P * Q, Kp), ref) and _intact(whole)
