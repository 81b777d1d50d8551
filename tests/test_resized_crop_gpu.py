"""The fused crop-box + bilinear resample + erase (+ Mixup / CutMix) input pass (resample.hip) on the
GPU, against the fp64 reference of resized_crop_reference.py under its derived rule
|out - ref| <= 2^-8 |ref| + 1e-5, and bit for bit against ``augment`` / ``augment_mix`` where the
geometry is the identity."""
import numpy as np
import pytest
import torch

import resized_crop_reference as R
from mi355x_dp.data.crops import BatchCropper, GeoParams
from mi355x_dp.data.mix import MixParams
from mi355x_dp.ops import MixedTarget, augment, augment_mix, augment_resized

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
MEAN, STD = R.MEAN, R.STD


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mi355x_dp.ops import _lib
    _lib.load(True)  # fail loudly if the extension is missing


def _geo(crop, flip, erase):
    return GeoParams(torch.tensor(np.asarray(crop), dtype=torch.int32, device="cuda").view(-1, 4),
                     torch.tensor(np.asarray(flip), dtype=torch.int32, device="cuda"),
                     torch.tensor(np.asarray(erase), dtype=torch.int32, device="cuda").view(-1, 4))


def _mixp(partner, lam, box):
    return MixParams(torch.tensor(np.asarray(partner), dtype=torch.int32, device="cuda"),
                     torch.tensor(np.asarray(lam), dtype=torch.float32, device="cuda"),
                     torch.tensor(np.asarray(box), dtype=torch.int32, device="cuda").view(-1, 4))


def _check(x, ref, what):
    out = x.float().cpu().numpy()
    ex = R.excess(out, ref)
    print(f"{what}: max |out - ref| {np.abs(out - ref).max():.3e}, max excess over the rule {ex:.3e}")
    assert ex <= 0, what


# ------------------------------------------------------------------------------------- 1. reference
@pytest.mark.parametrize("s,c,f", R.CASE_IDS)
def test_matches_reference(s, c, f):
    u8, size, C, cout, crop, flip, erase, ref = R.case(s, c, f)
    x = augment_resized(torch.from_numpy(u8.copy()).cuda(), size, cout, MEAN[:C], STD[:C], _geo(crop, flip, erase))
    assert x.dtype == BF and x.shape == (R.N, cout) + tuple(size) and x.is_contiguous(memory_format=CL)
    _check(x, ref, f"case {s} {c} {f}")
    assert (x[:, C:] == 0).all()
    assert (x[1] == x[1][:, :1, :1]).all()  # the 1 x 1 box: every output pixel is that pixel


# ------------------------------------------------------------------------------------- 2. identity
N_, H_, W_ = 5, 9, 11
PARTNER = [4, 0, 1, 2, 3]
MIX_LAM = [0.3, 0.0, 1.0, 0.5, 0.9]
MIX_BOX = [[0, 0, 0, 0], [3, 3, 2, 8], [0, 0, 0, 0], [5, 9, 8, 11], [-3, 4, 6, 20]]


@pytest.fixture(scope="module")
def small():
    g = torch.Generator(device="cuda").manual_seed(1)
    u8 = torch.randint(0, 256, (N_, H_, W_, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.tensor([3, 1, 4, 1, 5], device="cuda")
    ident = _geo([[0, 0, H_, W_]] * N_, [0] * N_, np.zeros((N_, 4)))
    return u8, labels, ident


@pytest.mark.parametrize("cout", [3, 8])
def test_identity_equals_augment_bit_for_bit(small, cout):
    u8, labels, ident = small
    x = augment_resized(u8, (H_, W_), cout, MEAN, STD, ident)
    assert torch.equal(x, augment(u8, cout, MEAN, STD, pad=0, flip=False))
    mp = _mixp(PARTNER, MIX_LAM, MIX_BOX)
    xm, t = augment_resized(u8, (H_, W_), cout, MEAN, STD, ident, mix=mp, labels=labels)
    xr, tr = augment_mix(u8, labels, cout, MEAN, STD, mp, pad=0, flip=False)
    assert torch.equal(xm, xr)
    assert torch.equal(t.y_a, tr.y_a) and torch.equal(t.y_b, tr.y_b) and torch.equal(t.lam, tr.lam)
    assert not torch.equal(xm, x)  # the mixing did something


# ------------------------------------------------------------------------------------- 3. erase
def _case_with(erase):
    u8, size, C, cout, crop, flip, _, _ = R.case(1, 0, 0)  # 32 x 32 -> 40 x 24, 3 -> 8 channels
    erase = np.asarray(erase, np.int32)
    return torch.from_numpy(u8.copy()).cuda(), size, cout, crop, flip, erase, R.resample(u8, size, cout, MEAN, STD, crop,
                                                                                       flip, erase)


ERASE = [[0, 0, 0, 0],      # empty
         [0, 40, 0, 24],    # the whole image
         [-3, 9, 20, 99],   # clipped by the border: rows 0..9, columns 20..24
         [5, 12, 3, 9],     # interior
         [7, 7, 0, 5]]      # empty (no rows)


def test_erase():
    u8, size, cout, crop, flip, erase, ref = _case_with(ERASE)
    x = augment_resized(u8, size, cout, MEAN, STD, _geo(crop, flip, erase))
    _check(x, ref, "erase")
    plain = augment_resized(u8, size, cout, MEAN, STD, _geo(crop, flip, np.zeros((5, 4))))
    assert torch.equal(x[0], plain[0]) and torch.equal(x[4], plain[4])
    assert (x[1] == 0).all()
    inside = torch.zeros(size, dtype=torch.bool, device="cuda")
    inside[:9, 20:] = True
    assert (x[2][:, inside] == 0).all() and torch.equal(x[2][:, ~inside], plain[2][:, ~inside])
    inside = torch.zeros(size, dtype=torch.bool, device="cuda")
    inside[5:12, 3:9] = True
    assert (x[3][:, inside] == 0).all() and torch.equal(x[3][:, ~inside], plain[3][:, ~inside])


def test_erased_partner_shows_through_as_zero():
    u8, size, cout, crop, flip, erase, ref = _case_with(ERASE)
    labels = torch.tensor([3, 1, 4, 1, 5], device="cuda")
    partner, lam = [1, 3, 3, 2, 0], [0.25, 0.0, 0.5, 0.5, 1.0]
    box = [[0, 0, 0, 0], [0, 0, 0, 0], [2, 20, 1, 20], [0, 0, 0, 0], [0, 0, 0, 0]]
    want, ya, yb, lo = R.mix(ref, labels.cpu().numpy(), partner, lam, box)
    x, t = augment_resized(u8, size, cout, MEAN, STD, _geo(crop, flip, erase), mix=_mixp(partner, lam, box),
                           labels=labels)
    _check(x, want, "erase + mix")
    solo = augment_resized(u8, size, cout, MEAN, STD, _geo(crop, flip, erase))
    # image 0 blends with the fully erased image 1: lam * a + (1 - lam) * 0, one bf16 rounding of 0.25 a (exact)
    assert torch.equal(x[0].float(), 0.25 * solo[0].float())
    # image 1 at lam 0 is its partner alone, erased interior included
    assert torch.equal(x[1], solo[3]) and (x[1][:, 5:12, 3:9] == 0).all()
    # image 2 pastes image 3 in the box: image 3's erased pixels arrive as zeros
    assert (x[2][:, 5:12, 3:9] == 0).all() and torch.equal(x[2][:, 2:20, 1:20], solo[3][:, 2:20, 1:20])
    assert t.y_a.tolist() == ya.tolist() and t.y_b.tolist() == yb.tolist() and np.array_equal(t.lam.cpu().numpy(), lo)


# ------------------------------------------------------------------------------------- 4. mix with resize
@pytest.mark.parametrize("s,c", [(0, 0), (1, 1), (2, 0), (2, 2)])
def test_mix_with_resize(s, c):
    u8, size, C, cout, crop, flip, erase, ref = R.case(s, c, 0)  # five boxes, flips 0 1 0 1 1: partners differ in both
    Ho, Wo = size
    labels = np.array([3, 1, 4, 1, 5])
    partner = [1, 2, 3, 9, -1]            # 9 and -1: outside [0, N), no mixing
    lam = [0.0, 1.0, 0.3, 0.5, 0.5]
    cut = [[1, Ho - 1, 2, Wo + 7], [0, 0, 0, 0], [0, 0, 0, 0], [0, 3, 0, 3], [0, 0, 0, 0]]
    for name, box in (("mixup", np.zeros((5, 4), np.int32)), ("cutmix", cut)):
        want, ya, yb, lo = R.mix(ref, labels, partner, lam, box)
        x, t = augment_resized(torch.from_numpy(u8.copy()).cuda(), size, cout, MEAN[:C], STD[:C], _geo(crop, flip, erase),
                               mix=_mixp(partner, lam, box), labels=torch.from_numpy(labels).cuda())
        _check(x, want, f"{name} {s} {c}")
        assert t.y_a.tolist() == ya.tolist() and t.y_b.tolist() == yb.tolist()
        assert np.array_equal(t.lam.cpu().numpy(), lo), name
        solo = augment_resized(torch.from_numpy(u8.copy()).cuda(), size, cout, MEAN[:C], STD[:C], _geo(crop, flip, erase))
        assert torch.equal(x[3], solo[3]) and torch.equal(x[4], solo[4])  # partner out of range: untouched
        assert torch.equal(x[1], solo[1])                                  # lam 1: the image alone
        if name == "mixup":
            assert torch.equal(x[0], solo[1])                              # lam 0: the partner alone


# ------------------------------------------------------------------------------------- 5. clipping
def test_wild_crop_boxes_stay_inside_the_image():
    """The source is a slice in the middle of one larger allocation whose surroundings are 255 while
    the images are 0; the boxes reach outside the images.  A tap outside the image would read a
    255 (or, past the batch, still this allocation): every output must be the normalized 0."""
    N, Hs, Ws, C = 4, 9, 7, 3
    big = torch.full((N + 8, Hs, Ws, C), 255, dtype=torch.uint8, device="cuda")
    big[4:4 + N] = 0
    u8 = big[4:4 + N]
    crop = torch.tensor([[-4, -5, 6, 6], [0, 0, 100, 90], [-3, 2, 40, 3], [5, -2, 9, 30]], dtype=torch.int32, device="cuda")
    for flips in ([0, 0, 0, 0], [1, 1, 1, 1]):
        geo = GeoParams(crop, torch.tensor(flips, dtype=torch.int32, device="cuda"),
                        torch.zeros((N, 4), dtype=torch.int32, device="cuda"))
        for size in ((5, 11), (9, 7), (20, 3)):
            x = augment_resized(u8, size, 8, MEAN, STD, geo)
            zero = augment(torch.zeros((1, 1, 1, C), dtype=torch.uint8, device="cuda"), 8, MEAN, STD, pad=0, flip=False)
            assert torch.equal(x, zero.expand_as(x)), (flips, size)


# ------------------------------------------------------------------------------------- 6. guards
@pytest.mark.parametrize("shape,size,cout", [((65536, 1, 1, 1), (1, 1), 1),     # N above 65535
                                             ((1, 16385, 1, 1), (1, 1), 1),     # Hs above 16384
                                             ((1, 1, 16385, 1), (1, 1), 1),     # Ws
                                             ((1, 1, 1, 1), (16385, 1), 1),     # Ho
                                             ((1, 1, 1, 1), (1, 16385), 1),     # Wo
                                             ((1, 1, 1, 1), (0, 1), 1),         # Ho below 1
                                             ((2, 4, 4, 3), (4, 4), 2)])        # Cout < C
def test_refused_shapes_launch_nothing(shape, size, cout):
    N, C = shape[0], shape[3]
    u8 = torch.zeros(shape, dtype=torch.uint8, device="cuda")
    geo = GeoParams(torch.ones((N, 4), dtype=torch.int32, device="cuda"), torch.zeros(N, dtype=torch.int32, device="cuda"),
                    torch.zeros((N, 4), dtype=torch.int32, device="cuda"))
    out = torch.full((N, cout) + tuple(size), 7.0, dtype=BF, device="cuda").contiguous(memory_format=CL)
    with pytest.raises(RuntimeError):
        augment_resized(u8, size, cout, MEAN[:C], STD[:C], geo, out=out)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


def test_empty_batch_is_refused():
    u8 = torch.zeros((0, 4, 4, 3), dtype=torch.uint8, device="cuda")
    geo = GeoParams(torch.ones((0, 4), dtype=torch.int32, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda"),
                    torch.zeros((0, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError):
        augment_resized(u8, 4, 3, MEAN, STD, geo)


def test_argument_checks():
    u8 = torch.zeros((2, 4, 4, 3), dtype=torch.uint8, device="cuda")
    geo = _geo([[0, 0, 4, 4]] * 2, [0, 0], np.zeros((2, 4)))
    with pytest.raises(ValueError):
        augment_resized(u8, 4, 3, MEAN, STD, GeoParams(geo.crop.long(), geo.flip, geo.erase))
    with pytest.raises(ValueError):
        augment_resized(u8, 4, 3, MEAN, STD, GeoParams(geo.crop, geo.flip.cpu(), geo.erase))
    with pytest.raises(ValueError):
        augment_resized(u8, 4, 3, MEAN, STD, geo, out=torch.empty((2, 3, 4, 4), dtype=BF, device="cuda"))  # not channels_last
    with pytest.raises(ValueError):
        augment_resized(u8, 4, 3, MEAN, STD, geo, mix=_mixp([0, 1], [1.0, 1.0], np.zeros((2, 4))))  # no labels


# ------------------------------------------------------------------------------------- 7. repeatability
def test_repeatable():
    u8, size, C, cout, crop, flip, erase, _ = R.case(2, 0, 1)
    d, geo = torch.from_numpy(u8.copy()).cuda(), _geo(crop, flip, ERASE)
    mp, labels = _mixp(PARTNER, MIX_LAM, MIX_BOX), torch.tensor([3, 1, 4, 1, 5], device="cuda")
    x1, t1 = augment_resized(d, size, cout, MEAN, STD, geo, mix=mp, labels=labels)
    x2, t2 = augment_resized(d, size, cout, MEAN, STD, geo, mix=mp, labels=labels)
    assert torch.equal(x1, x2) and all(torch.equal(a, b) for a, b in zip(t1, t2))


# ------------------------------------------------------------------------------------- 8. graph capture
def test_graph_replay_sees_new_parameters():
    """One call captured over static ``out`` / ``target`` and the cropper's and a mixer's persistent
    parameter buffers: uploading new parameters and replaying equals the eager call on them."""
    u8, size, C, cout, crop, flip, erase, _ = R.case(1, 0, 0)
    d, labels = torch.from_numpy(u8.copy()).cuda(), torch.tensor([3, 1, 4, 1, 5], device="cuda")
    cropper = BatchCropper(size, erase_prob=0.7, seed=4, device="cuda")
    hosts = [cropper.host_params(s, R.N, 32, 32) for s in (0, 1)]
    mixes = [(PARTNER, MIX_LAM, MIX_BOX), ([1, 2, 3, 4, 0], [0.6, 0.5, 0.0, 1.0, 0.2], np.zeros((5, 4)))]
    eager = []
    for h, m in zip(hosts, mixes):
        x, t = augment_resized(d, size, cout, MEAN, STD, _geo(*h), mix=_mixp(*m), labels=labels)
        eager.append((x.clone(), [v.clone() for v in t]))
    assert not torch.equal(eager[0][0], eager[1][0])
    geo = cropper.upload(*hosts[0], 32, 32)  # the persistent buffer: later uploads rewrite it in place
    mp = _mixp(*mixes[0])
    out = torch.zeros((R.N, cout) + tuple(size), dtype=BF, device="cuda").contiguous(memory_format=CL)
    tgt = MixedTarget(torch.zeros(R.N, dtype=torch.int64, device="cuda"), torch.zeros(R.N, dtype=torch.int64, device="cuda"),
                      torch.zeros(R.N, device="cuda"))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as torch's capture recipe
        augment_resized(d, size, cout, MEAN, STD, geo, mix=mp, labels=labels, out=out, target=tgt)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        augment_resized(d, size, cout, MEAN, STD, geo, mix=mp, labels=labels, out=out, target=tgt)
    for h, m, (x_e, t_e) in zip(hosts, mixes, eager):
        g2 = cropper.upload(*h, 32, 32)
        assert g2.crop.data_ptr() == geo.crop.data_ptr()
        for dst, src in zip(mp, _mixp(*m)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, x_e) and all(torch.equal(a, b) for a, b in zip(tgt, t_e))


# ------------------------------------------------------------------------------------- 9. end to end
def test_batch_cropper_end_to_end():
    Hs, Ws, size, N = 37, 53, (16, 24), 4
    rng = np.random.default_rng(9)
    u8 = rng.integers(0, 256, (N, Hs, Ws, 3), dtype=np.uint8)
    d = torch.from_numpy(u8).cuda()
    cropper = BatchCropper(size, erase_prob=0.5, seed=2, rank=1, device="cuda")
    seen = []
    for step in range(3):
        crop, flip, erase = cropper.host_params(step, N, Hs, Ws)
        geo = cropper.params(step, N, Hs, Ws)
        assert geo.crop.tolist() == crop.tolist() and geo.flip.tolist() == flip.tolist()
        assert geo.erase.tolist() == erase.tolist()
        x = augment_resized(d, size, 8, MEAN, STD, geo)
        _check(x, R.resample(u8, size, 8, MEAN, STD, crop, flip, erase), f"cropper step {step}")
        seen.append(crop.tolist())
    assert seen[0] != seen[1] != seen[2]
    ev = cropper.center_params(N, Hs, Ws, crop_pct=0.875)
    box = cropper.center_box(Hs, Ws, 0.875)
    x = augment_resized(d, size, 8, MEAN, STD, ev)
    _check(x, R.resample(u8, size, 8, MEAN, STD, [box] * N, [0] * N, np.zeros((N, 4), np.int32)), "centre crop")
