"""RandomResizedCrop / RandomErasing / centre crop without a GPU: the host draws of
``data.crops.BatchCropper`` and the host path of ``ops.augment_resized`` against the fp64 reference."""
import numpy as np
import pytest
import torch

import resized_crop_reference as R
from mi355x_dp.data.crops import BatchCropper, GeoParams, fallback_crop
from mi355x_dp.data.mix import BatchMixer, MixParams
from mi355x_dp.ops import augment, augment_resized

MEAN, STD = R.MEAN, R.STD


def _geo(crop, flip, erase):
    return GeoParams(torch.tensor(np.asarray(crop), dtype=torch.int32).view(-1, 4),
                     torch.tensor(np.asarray(flip), dtype=torch.int32),
                     torch.tensor(np.asarray(erase), dtype=torch.int32).view(-1, 4))


# ------------------------------------------------------------------------------------- draws
def test_host_params_are_a_pure_function_of_seed_rank_step():
    c = BatchCropper(24, erase_prob=0.5, seed=3, rank=1, device="cpu")
    a, b = c.host_params(7, 64, 37, 53), c.host_params(7, 64, 37, 53)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    assert all(u.dtype == np.int32 for u in a) and a[0].shape == (64, 4) and a[1].shape == (64,) and a[2].shape == (64, 4)
    other_step = c.host_params(8, 64, 37, 53)
    other_rank = BatchCropper(24, erase_prob=0.5, seed=3, rank=2, device="cpu").host_params(7, 64, 37, 53)
    other_seed = BatchCropper(24, erase_prob=0.5, seed=4, rank=1, device="cpu").host_params(7, 64, 37, 53)
    for o in (other_step, other_rank, other_seed):
        assert not np.array_equal(a[0], o[0]) and not np.array_equal(a[1], o[1])


def test_stream_is_apart_from_the_mixers():
    """Same (seed, rank, step): the cropper's first uniforms are not the mixer's."""
    from mi355x_dp.data import crops
    rng_m = np.random.default_rng(np.random.SeedSequence([5, 0, 11]))
    rng_c = np.random.default_rng(np.random.SeedSequence([5, 0, 11, crops.TAG]))
    assert not np.array_equal(rng_m.random(8), rng_c.random(8))
    # and through the public draws: per-image crop rows against per-image CutMix centres
    N, S = 256, 64
    crop, _, _ = BatchCropper(S, seed=5, device="cpu").host_params(11, N, S, S)
    _, _, box = BatchMixer(0.0, 1.0, per_sample=True, seed=5, device="cpu").host_params(11, N, S, S)
    cy_crop = crop[:, 0] + crop[:, 2] / 2.0
    cy_box = (box[:, 0] + box[:, 1]) / 2.0
    r = np.corrcoef(cy_crop, cy_box)[0, 1]
    assert abs(r) < 5.0 / np.sqrt(N), r  # independent: |r| ~ 1 / sqrt(N)


@pytest.mark.parametrize("Hs,Ws", [(37, 53), (224, 224)])
def test_boxes_lie_inside_and_respect_scale_and_ratio(Hs, Ws):
    """w = round(w*), h = round(h*) with w* h* = area in scale * Hs * Ws and w* / h* in ratio, so
    |w - w*|, |h - h*| <= 1/2: the box passes when the intervals [w - 1/2, w + 1/2] x [h - 1/2,
    h + 1/2] can hold such a pair.  The fallback box (whole image, ratio clamped) passes it too."""
    scale, ratio = (0.08, 1.0), (3 / 4, 4 / 3)
    c = BatchCropper(16, scale=scale, ratio=ratio, device="cpu")
    crop = np.concatenate([c.host_params(s, 500, Hs, Ws)[0] for s in range(4)]).astype(np.float64)  # 2,000 draws
    top, left, h, w = crop.T
    assert (top >= 0).all() and (left >= 0).all() and (h >= 1).all() and (w >= 1).all()
    assert (top + h <= Hs).all() and (left + w <= Ws).all()
    A = Hs * Ws
    assert ((w + .5) * (h + .5) >= scale[0] * A).all() and ((w - .5) * (h - .5) <= scale[1] * A).all()
    assert ((w + .5) / (h - .5) >= ratio[0]).all() and ((w - .5) / (h + .5) <= ratio[1]).all()
    assert len(np.unique(crop, axis=0)) > 1000  # really random
    assert len(np.unique(top)) > Hs // 2 and len(np.unique(left)) > Ws // 2


def test_fallback_is_the_clamped_central_crop():
    c = BatchCropper(16, scale=(1.0, 1.0), ratio=(5.0, 6.0), device="cpu")
    crop, _, _ = c.host_params(0, 32, 40, 40)  # w = round(sqrt(1600 r)) > 40 on every try
    assert fallback_crop(40, 40, (5.0, 6.0)) == (16, 0, 8, 40)
    assert (crop == np.array([16, 0, 8, 40])).all()
    assert fallback_crop(10, 100, (0.75, 4 / 3)) == (0, 43, 10, 13) and fallback_crop(37, 41, (0.75, 4 / 3)) == (0, 0, 37, 41)


def test_erase_prob_zero_and_one():
    Ho, Wo = 24, 40
    off = BatchCropper((Ho, Wo), erase_prob=0.0, device="cpu").host_params(1, 500, 32, 32)[2]
    assert (off == 0).all()
    on = BatchCropper((Ho, Wo), erase_prob=1.0, device="cpu").host_params(1, 500, 32, 32)[2].astype(np.float64)
    y0, y1, x0, x1 = on.T
    h, w = y1 - y0, x1 - x0
    assert (y0 >= 0).all() and (x0 >= 0).all() and (y1 <= Ho).all() and (x1 <= Wo).all()
    # defaults (0.02..0.33 of the area, ratio 0.3..3.3) nearly always fit in ten tries
    drawn = (h > 0) & (w > 0)
    assert drawn.mean() > 0.99 and (h[drawn] < Ho).all() and (w[drawn] < Wo).all()
    A = Ho * Wo  # the rounding margins of the crop test; here h is the side that takes the aspect
    assert ((w + .5) * (h + .5) >= 0.02 * A)[drawn].all() and ((w - .5) * (h - .5) <= 0.33 * A)[drawn].all()
    assert ((h + .5) / (w - .5) >= 0.3)[drawn].all() and ((h - .5) / (w + .5) <= 3.3)[drawn].all()
    # a box that can never fit (area = the whole output): no box
    never = BatchCropper((Ho, Wo), erase_prob=1.0, erase_scale=(1.0, 1.0), erase_ratio=(1.0, 1.0), device="cpu")
    assert (never.host_params(1, 50, 32, 32)[2] == 0).all()
    half = BatchCropper((Ho, Wo), erase_prob=0.5, device="cpu").host_params(1, 2000, 32, 32)[2]
    frac = ((half[:, 1] > half[:, 0]) & (half[:, 3] > half[:, 2])).mean()
    assert abs(frac - 0.5) < 5 * np.sqrt(0.25 / 2000)  # five standard deviations of the binomial
    flips = BatchCropper(8, flip_prob=0.5, device="cpu").host_params(1, 2000, 32, 32)[1]
    assert set(np.unique(flips)) == {0, 1} and abs(flips.mean() - 0.5) < 5 * np.sqrt(0.25 / 2000)
    assert (BatchCropper(8, flip_prob=0.0, device="cpu").host_params(1, 64, 32, 32)[1] == 0).all()


def test_upload_checks_the_boxes_and_returns_views_of_one_buffer():
    c = BatchCropper(16, device="cpu")
    crop, flip, erase = c.host_params(0, 4, 37, 53)
    g = c.upload(crop, flip, erase, 37, 53)
    assert isinstance(g, GeoParams) and g.crop.dtype == torch.int32
    assert g.crop.tolist() == crop.tolist() and g.flip.tolist() == flip.tolist() and g.erase.tolist() == erase.tolist()
    assert g.crop.is_contiguous() and g.flip.is_contiguous() and g.erase.is_contiguous()
    p = c.params(0, 4, 37, 53)
    assert p.crop.tolist() == crop.tolist()
    for bad in ([-1, 0, 5, 5], [0, 0, 38, 5], [30, 0, 8, 5], [0, 50, 5, 4], [0, 0, 0, 5]):
        b = crop.copy()
        b[2] = bad
        with pytest.raises(ValueError):
            c.upload(b, flip, erase, 37, 53)
    for bad in ([0, 17, 0, 4], [-1, 4, 0, 4], [5, 4, 0, 4], [0, 4, 3, 17]):
        e = erase.copy()
        e[1] = bad
        with pytest.raises(ValueError):
            c.upload(crop, flip, e, 37, 53)
    with pytest.raises(ValueError):
        c.upload(crop[:3], flip, erase, 37, 53)


def test_center_params():
    c = BatchCropper(24, device="cpu")
    g = c.center_params(3, 32, 32, crop_pct=0.875)
    assert g.crop.tolist() == [[2, 2, 28, 28]] * 3 and g.flip.tolist() == [0] * 3 and g.erase.tolist() == [[0] * 4] * 3
    assert c.center_params(3, 32, 32, crop_pct=0.875) is g  # cached
    assert c.center_params(2, 37, 53).crop.tolist() == [[0, 8, 37, 37]] * 2
    assert c.center_params(2, 37, 53, crop_pct=0.5).crop.tolist() == [[9, 17, 18, 18]] * 2  # round(18.5) = 18 (half to even)
    wide = BatchCropper((16, 24), device="cpu")  # output aspect 3:2
    assert wide.center_params(1, 37, 53).crop.tolist() == [[1, 0, 35, 53]]  # full width, height 53 * 2 / 3 = 35.33
    assert wide.center_params(1, 53, 37).crop.tolist() == [[14, 0, 25, 37]]  # 37 * 2 / 3 = 24.67
    assert wide.center_params(1, 20, 90).crop.tolist() == [[0, 30, 20, 30]]  # full height


# ------------------------------------------------------------------------------------- host path
@pytest.mark.parametrize("s,c,f", R.CASE_IDS)
def test_host_path_matches_reference(s, c, f):
    u8, size, C, cout, crop, flip, erase, ref = R.case(s, c, f)
    x = augment_resized(torch.from_numpy(u8.copy()), size, cout, MEAN[:C], STD[:C], _geo(crop, flip, erase))
    assert x.dtype == torch.float32 and x.shape == (R.N, cout) + tuple(size)
    ex = R.excess(x.numpy(), ref, rel=0.0)
    print(f"case {s} {c} {f}: max |out - ref| {np.abs(x.numpy() - ref).max():.3e}, excess {ex:.3e}")
    assert ex <= 0
    assert (x[1] == x[1][:, :1, :1]).all()  # the 1 x 1 box: every output pixel is that pixel


def test_host_path_erase_and_mix_match_reference():
    u8, size, C, cout, crop, flip, _, _ = R.case(1, 0, 0)
    Ho, Wo = size
    erase = np.array([[0, 0, 0, 0], [0, Ho, 0, Wo], [-3, 9, 20, 99], [5, 12, 3, 9], [7, 7, 0, 5]], np.int32)
    partner = np.array([4, 0, 7, 2, 3], np.int32)
    lam = np.array([0.3, 0.0, 0.5, 1.0, 0.7], np.float32)
    box = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [2, 9, 3, 8], [0, 0, 0, 0], [-5, 20, 10, 70]], np.int32)
    labels = np.array([3, 1, 4, 1, 5])
    ref = R.resample(u8, size, cout, MEAN, STD, crop, flip, erase)
    x = augment_resized(torch.from_numpy(u8.copy()), size, cout, MEAN, STD, _geo(crop, flip, erase))
    assert R.excess(x.numpy(), ref, rel=0.0) <= 0
    assert (x[1] == 0).all() and (x[2][:, :9, 20:] == 0).all() and (x[2][:, 9:] != 0).any()
    want, ya, yb, lo = R.mix(ref, labels, partner, lam, box)
    mp = MixParams(torch.from_numpy(partner), torch.from_numpy(lam), torch.from_numpy(box))
    xm, t = augment_resized(torch.from_numpy(u8.copy()), size, cout, MEAN, STD, _geo(crop, flip, erase), mix=mp,
                            labels=torch.from_numpy(labels))
    assert R.excess(xm.numpy(), want, rel=0.0) <= 0
    assert t.y_a.tolist() == ya.tolist() and t.y_b.tolist() == yb.tolist()
    assert np.array_equal(t.lam.numpy(), lo)


def test_host_path_clips_wild_boxes():
    """A crop reaching outside the source is clipped into it (height and width at least 1), as on
    the device: a uniform image then gives the uniform value, whatever the box."""
    u8 = torch.full((4, 9, 7, 3), 51, dtype=torch.uint8)
    crop = [[-4, -4, 5, 5], [0, 0, 100, 100], [20, 30, 2, 2], [3, 2, -7, 0]]
    x = augment_resized(u8, (5, 11), 3, MEAN, STD, _geo(crop, [0, 1, 0, 1], np.zeros((4, 4))))
    want = augment(u8, 3, MEAN, STD)[:, :, :1, :1]
    assert torch.allclose(x, want.expand_as(x), atol=1e-6, rtol=0)


def test_identity_geometry_equals_augment_host_path():
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (3, 9, 7, 3), dtype=torch.uint8, generator=g)
    geo = _geo([[0, 0, 9, 7]] * 3, [0] * 3, np.zeros((3, 4)))
    x = augment_resized(u8, (9, 7), 8, MEAN, STD, geo)
    assert torch.equal(x[:, :3], augment(u8, 8, MEAN, STD)) and (x[:, 3:] == 0).all()
    mixer = BatchMixer(per_sample=True, seed=1, device="cpu")
    mp = mixer.params(0, 3, 9, 7)
    labels = torch.tensor([2, 0, 1])
    from mi355x_dp.ops import augment_mix
    xm, t = augment_resized(u8, (9, 7), 3, MEAN, STD, geo, mix=mp, labels=labels)
    xr, tr = augment_mix(u8, labels, 3, MEAN, STD, mp)
    assert torch.equal(xm, xr) and all(torch.equal(a, b) for a, b in zip(t, tr))


def test_argument_checks():
    u8 = torch.zeros((2, 4, 4, 3), dtype=torch.uint8)
    geo = _geo([[0, 0, 4, 4]] * 2, [0, 0], np.zeros((2, 4)))
    mp = MixParams(torch.zeros(2, dtype=torch.int32), torch.ones(2), torch.zeros((2, 4), dtype=torch.int32))
    with pytest.raises(ValueError):
        augment_resized(u8, 4, 3, MEAN, STD, geo, mix=mp)  # mix without labels
    with pytest.raises(ValueError):
        augment_resized(u8, 4, 3, MEAN, STD, geo, labels=torch.zeros(2, dtype=torch.int64))
