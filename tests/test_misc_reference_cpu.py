"""The host references of misc_reference.py, checked on their own terms before the GPU tests lean
on them: the hash replica's coverage of every (dy, dx, flip), the crop / flip composition against a
hand-worked example, the first-maximum rule of ``F.max_pool2d``'s indices, the share of tied windows
in the pooling inputs, and each formula against a second, independent evaluation."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import misc_reference as mr
from misc_reference import BF, F64

SEEDS = [0, 3, 17, 2 ** 31, 2 ** 32 - 1]


# ------------------------------------------------------------------------------------ augment
@pytest.mark.parametrize("seed", SEEDS)
def test_draw_covers_every_offset_and_flip(seed):
    """N = 2048 at pad = 4: all 9 * 9 * 2 = 162 (dy, dx, flip) occur, the rarest at least 4 times"""
    counts = {}
    for n in range(2048):
        d = mr.draw(seed, n, 4, True)
        counts[d] = counts.get(d, 0) + 1
    assert set(counts) == {(dy, dx, fl) for dy in range(-4, 5) for dx in range(-4, 5) for fl in (False, True)}
    assert min(counts.values()) >= 4, min(counts.values())


def test_draw_ranges_and_seed_wrap():
    for pad in (0, 1, 4):
        ds = [mr.draw(7, n, pad, True) for n in range(512)]
        assert {d[0] for d in ds} == set(range(-pad, pad + 1)) == {d[1] for d in ds}
        assert {d[2] for d in ds} == {False, True}  # the flip is drawn at pad = 0 too
        assert not any(mr.draw(7, n, pad, False)[2] for n in range(512))
    assert [mr.draw(2 ** 32 + 5, n, 4, True) for n in range(64)] == [mr.draw(5, n, 4, True) for n in range(64)]
    assert [mr.draw(5, n, 4, True) for n in range(64)] != [mr.draw(6, n, 4, True) for n in range(64)]
    assert mr.hash32(0) == 0 and all(0 <= mr.hash32(v) < 2 ** 32 for v in (1, 2 ** 31, 2 ** 32 - 1, 2 ** 32 + 1))


def test_compose_hand_example():
    """3 x 3, pad 1, dy = +1, dx = -1, flipped.  Padded to 5 x 5 the image sits in rows/columns 1-3;
    the crop starts at row 2, column 0:
        0 40 50          50 40  0
        0 70 80  flip -> 80 70  0      (the right column and the bottom row come from the padding)
        0  0  0           0  0  0"""
    img = torch.tensor([[10, 20, 30], [40, 50, 60], [70, 80, 90]], dtype=torch.uint8).view(3, 3, 1)
    out = mr.compose(img, 1, -1, True, 1, 2, (0.0,), (1.0,))
    want = torch.tensor([[50, 40, 0], [80, 70, 0], [0, 0, 0]], dtype=F64) / 255.0
    assert out.dtype == BF and out.shape == (2, 3, 3)
    assert torch.equal(out[0], want.to(BF)) and not out[1].any()
    # no flip: the crop itself; dy = -1, dx = +1: the opposite corner
    assert torch.equal(mr.compose(img, 1, -1, False, 1, 1, (0.0,), (1.0,))[0],
                       (torch.tensor([[0, 40, 50], [0, 70, 80], [0, 0, 0]], dtype=F64) / 255.0).to(BF))
    assert torch.equal(mr.compose(img, -1, 1, False, 1, 1, (0.0,), (1.0,))[0],
                       (torch.tensor([[0, 0, 0], [20, 30, 0], [50, 60, 0]], dtype=F64) / 255.0).to(BF))
    # normalisation and its border: (v / 255 - mean) / std inside, 0 (not -mean / std) outside
    out = mr.compose(img, 0, 1, False, 1, 1, (0.5,), (0.25,))
    assert float(out[0, 0, 2]) == 0.0
    assert float(out[0, 0, 0]) == float(torch.tensor((20 / 255 - 0.5) / 0.25, dtype=F64).to(BF))


def test_reference_without_crop_is_the_host_fallback():
    """pad = 0, flip off: the plain normalisation ``augment`` computes for host tensors (its CPU
    branch applies no crop and no flip at any setting)"""
    from mi355x_dp.ops import augment
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (4, 9, 11, 3), dtype=torch.uint8, generator=g)
    mean, std = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)
    ref = mr.augment_reference(u8, 3, mean, std, 0, False, 3)
    host = augment(u8, 3, mean, std, pad=0, flip=False, seed=3)
    assert int(mr.bf16_ulp_diff(host.to(BF), ref).max()) <= 1
    assert torch.equal(augment(u8, 3, mean, std, pad=4, flip=True, seed=3), host)


def test_position_code_round_trip():
    """decode_positions reads back the draws the reference applied, all 162 among them"""
    ref = mr.augment_reference(mr.position_coded(2048), 1, mr.POS_MEAN, mr.POS_STD, 4, True, 17)
    assert torch.equal(ref[5].float(), ref[5].float().round())  # the code survives normalisation and bf16
    got = mr.decode_positions(ref, 4)
    assert got == [mr.draw(17, n, 4, True) for n in range(2048)]
    assert len(set(got)) == 162


def test_bf16_ulp_diff():
    a = torch.tensor([1.0, 1.0, -1.0, 0.0, 2.0 ** -126], dtype=BF)
    b = torch.tensor([1.0078125, 0.99609375, -1.0078125, -0.0, -(2.0 ** -126)], dtype=BF)
    assert mr.bf16_ulp_diff(a, b).tolist() == [1, 1, 1, 0, 2 * 0x0080]


# ----------------------------------------------------------------------------------- max pool
@pytest.mark.parametrize("C", mr.POOL_CHANNELS)
@pytest.mark.parametrize("geom", mr.POOL_GEOMS)
def test_pool_reference_first_max_and_tie_share(geom, C):
    H, W, k, s, pad = geom
    x, dy = mr.pool_inputs(geom, C, integer=True)
    assert torch.equal(x.to(BF).to(F64), x) and torch.equal(dy.to(BF).to(F64), dy)
    y, dx, idx = mr.maxpool_reference(x, dy, k, s, pad)
    # torch's indices are the first maximum in scan order, ties included
    assert torch.equal(idx, mr.first_max_indices(x, k, s, pad))
    share = mr.tie_share(x, k, s, pad)
    print(f"{geom} C={C}: {100 * share:.0f} % of windows hold a tie")
    assert share >= 0.15
    # the scatter is autograd's gradient, and bf16 holds it exactly
    xr = x.clone().requires_grad_()
    F.max_pool2d(xr, k, s, pad).backward(dy)
    assert torch.equal(dx, xr.grad)
    assert float(dx.abs().max()) < 256 and torch.equal(dx.to(BF).to(F64), dx)


def test_pool_geometries_hold_the_cases_they_are_listed_for():
    geoms = mr.POOL_GEOMS
    assert any(k == s and pad == 0 for _, _, k, s, pad in geoms)       # non-overlapping
    assert any(s == 1 for _, _, k, s, pad in geoms)                    # stride 1
    assert any(k > 2 * s for _, _, k, s, pad in geoms)                 # three windows per axis over a pixel
    assert any(s < k <= 2 * s and s > 1 for _, _, k, s, pad in geoms)  # two
    assert any(pad == 0 and k > s for _, _, k, s, pad in geoms)
    assert any(H != W for H, W, _, _, _ in geoms)
    assert any(H < 2 * k for H, _, k, _, _ in geoms)
    # a last row that no window covers: (P - 1) s - pad + k - 1 < H - 1
    assert any((mr.pool_out(H, k, s, pad) - 1) * s - pad + k - 1 < H - 1 for H, _, k, s, pad in geoms)


# ----------------------------------------------------------------------- global average pool
@pytest.mark.parametrize("HW,C,N", mr.GAP_CASES)
def test_gap_bound_holds_for_a_sequential_fp32_sum(HW, C, N):
    """the bound admits what it is derived for: fp32 accumulation in order, times fp32 1 / HW,
    rounded to bf16"""
    x, _ = mr.gap_inputs(HW, C, N)
    ref, bound = mr.gap_forward_bound(x)
    acc = np.cumsum(x.reshape(N, C, HW).numpy().astype(np.float32), axis=2, dtype=np.float32)[:, :, -1]
    y = torch.from_numpy(acc * np.float32(1.0 / HW)).to(BF).to(F64)
    assert bool(((y - ref).abs() <= bound).all())
    if C % 8 == 0 and C != 2048:
        assert (N * C // 8) % 256 != 0


# ---------------------------------------------------------------------------- cross entropy
def test_ce_reference_and_row_error():
    lg = torch.full((4, 10), 1.5)
    y = torch.tensor([0, 9, 3, 3])
    loss, grad = mr.ce_reference(lg, y)
    assert abs(loss - math.log(10)) < 1e-12
    want = torch.full((4, 10), 0.1, dtype=F64) - F.one_hot(y, 10)
    assert torch.allclose(grad, want / 4, atol=1e-15)
    _, g2 = mr.ce_reference(lg, y, gout=2.0)
    assert torch.allclose(g2, 2 * grad, atol=1e-15)
    # one row of 1e-6 magnitude that is entirely wrong: invisible batch-wide, 2.0 per row
    ref = torch.ones(3, 5, dtype=F64)
    ref[1] *= 1e-6
    got = ref.clone()
    got[1] = -got[1]
    assert float((got - ref).abs().max() / ref.abs().max()) < 1e-5
    assert mr.row_rel_err(got, ref) == pytest.approx(2.0)
    assert mr.row_rel_err(torch.zeros(2, 3), torch.full((2, 3), 1e-70, dtype=F64)) < 1e-30
    for N, C in mr.CE_SHAPES:
        _, yy = mr.ce_inputs(N, C, torch.float32)
        assert int(yy[0]) == 0 and int(yy[-1]) == C - 1 and 0 <= int(yy.min()) and int(yy.max()) < C


# --------------------------------------------------------------------------------- flat SGD
@pytest.mark.parametrize("cfg", mr.SGD_CONFIGS)
def test_sgd_reference_is_torch_sgd(cfg):
    """two steps of the reference = two steps of ``torch.optim.SGD`` in fp64 (same fp32-rounded
    scalars); step one is the first step unless the configuration says it is a later one"""
    momentum, dampening, wd, nesterov, first = cfg
    g = torch.Generator().manual_seed(5)
    p0 = torch.randn(1000, generator=g)
    grads = [torch.randn(1000, generator=g) for _ in range(2)]
    ref = torch.nn.Parameter(p0.to(F64))
    opt = torch.optim.SGD([ref], lr=mr.f32(mr.SGD_LR), momentum=mr.f32(momentum), dampening=mr.f32(dampening),
                          weight_decay=mr.f32(wd), nesterov=nesterov)
    p, buf = p0.to(F64), torch.zeros(1000, dtype=F64)
    for step, gr in enumerate(grads):
        ref.grad = gr.to(F64) * 0.125
        opt.step()
        p, buf, _ = mr.sgd_reference(p, gr, buf, mr.SGD_LR, momentum, dampening, wd, nesterov, step == 0, 0.125)
        assert torch.allclose(p, ref.detach(), rtol=1e-14, atol=1e-15)
    if momentum:
        assert torch.allclose(buf, opt.state[ref]["momentum_buffer"], rtol=1e-14, atol=1e-15)


@pytest.mark.parametrize("grad_scale", [1.0, 0.125])
@pytest.mark.parametrize("cfg", mr.SGD_CONFIGS)
def test_sgd_bound_admits_the_fp32_host_branch(cfg, grad_scale):
    """``sgd_flat_``'s host branch, plain fp32 without fused multiply-adds, stays inside the bound
    the kernel is held to: the bound is attainable in fp32 arithmetic"""
    from mi355x_dp.ops import sgd_flat_
    momentum, dampening, wd, nesterov, first = cfg
    g = torch.Generator().manual_seed(6)
    n = 200_003
    p, gr, buf = (torch.randn(n, generator=g) for _ in range(3))
    p[:1000] *= 1e-4  # parameters near zero: there the bound rests on its gradient term
    p_ref, buf_ref, bound = mr.sgd_reference(p, gr, buf, mr.SGD_LR, momentum, dampening, wd, nesterov, first,
                                             grad_scale)
    buf0, p16 = buf.clone(), torch.empty(n, dtype=BF)
    sgd_flat_(p, gr, buf, p16, mr.SGD_LR, momentum, dampening, wd, nesterov, first_step=first,
              grad_scale=grad_scale)
    rp = float(((p.to(F64) - p_ref).abs() / bound).max())
    rb = float(((buf.to(F64) - buf_ref).abs() / bound).max())
    print(f"{cfg} scale {grad_scale}: worst |p - ref| / bound {rp:.3f}, buf {rb:.3f}")
    assert rp <= 1.0 and rb <= 1.0
    assert torch.equal(p16, p.to(BF))
    if not momentum:
        assert torch.equal(buf, buf0)


# ----------------------------------------------------------------------------------- im2col
def test_im2col_reference_against_loops():
    C, R, stride, pad, H = 3, 3, 2, 1, 5
    W, Kp, N = H + 1, 32, 2
    x = torch.arange(N * C * H * W, dtype=F64).view(N, C, H, W) + 1
    col = mr.im2col_reference(x, R, R, stride, pad, Kp)
    P, Q = mr.pool_out(H, R, stride, pad), mr.pool_out(W, R, stride, pad)
    assert col.shape == (N * P * Q, Kp)
    for n in range(N):
        for p in range(P):
            for q in range(Q):
                row = col[(n * P + p) * Q + q]
                for r in range(R):
                    for s in range(R):
                        ih, iw = p * stride - pad + r, q * stride - pad + s
                        for c in range(C):
                            inside = 0 <= ih < H and 0 <= iw < W
                            assert float(row[(r * R + s) * C + c]) == (float(x[n, c, ih, iw]) if inside else 0.0)
                assert not row[R * R * C:].any()
