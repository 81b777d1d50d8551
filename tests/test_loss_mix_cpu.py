"""Label smoothing / soft targets / Mixup-CutMix without a GPU: the CPU paths of ``cross_entropy`` for
its three target forms against ``F.cross_entropy`` in fp64 on dense targets, and the host-side
parameter source ``BatchMixer`` (purity in (seed, rank, step), the CutMix box rule, the switches)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mi355x_dp.data.mix import BatchMixer, MixParams, cutmix_box
from mi355x_dp.ops import MixedTarget, augment_mix, cross_entropy

N, C = 5, 10


def _problem():
    g = torch.Generator().manual_seed(0)
    lg = torch.randn(N, C, generator=g) * 3
    ya = torch.randint(0, C, (N,), generator=g)
    yb = torch.randint(0, C, (N,), generator=g)
    yb[2] = ya[2]
    lam = torch.tensor([0.0, 1.0, 0.3, 0.75, 0.5])
    return lg, ya, yb, lam


def _dense64(ya, yb, lam):
    lam = lam.double().unsqueeze(1)
    return lam * F.one_hot(ya, C).double() + (1 - lam) * F.one_hot(yb, C).double()


def _check(lg, target, dense64, eps):
    a = lg.clone().requires_grad_()
    loss = cross_entropy(a, target, label_smoothing=eps)
    loss.backward()
    r = lg.double().requires_grad_()
    ref = F.cross_entropy(r, dense64, label_smoothing=eps)
    ref.backward()
    assert abs(float(loss.detach()) - float(ref.detach())) < 1e-5 * max(1.0, abs(float(ref.detach())))
    assert torch.allclose(a.grad.double(), r.grad, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_cpu_hard_labels(eps):
    lg, ya, _, _ = _problem()
    _check(lg, ya, F.one_hot(ya, C).double(), eps)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_cpu_mixed_target(eps):
    lg, ya, yb, lam = _problem()
    _check(lg, MixedTarget(ya, yb, lam), _dense64(ya, yb, lam), eps)


@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_cpu_dense_target(eps):
    lg, ya, yb, lam = _problem()
    t = _dense64(ya, yb, lam)
    t[1] *= 0.5  # rows need not sum to one
    _check(lg, t.float(), t.float().double(), eps)
    _check(lg, t.bfloat16(), t.bfloat16().double(), eps)


def test_default_is_hard_label_path():
    lg, ya, _, _ = _problem()
    assert torch.equal(cross_entropy(lg, ya), cross_entropy(lg, ya, label_smoothing=0.0))
    assert torch.equal(cross_entropy(lg, ya), F.cross_entropy(lg, ya))


# ------------------------------------------------------------------------------- BatchMixer
H, W = 24, 32


def _same(p, q):
    return all(np.array_equal(a, b) for a, b in zip(p, q))


@pytest.mark.parametrize("per_sample", [False, True])
def test_params_are_a_pure_function_of_seed_rank_step(per_sample):
    m = BatchMixer(seed=3, rank=1, per_sample=per_sample, device="cpu")
    first = m.host_params(7, 8, H, W)
    for s in (0, 1, 2, 9):  # other calls in between
        m.host_params(s, 8, H, W)
        m.params(s, 8, H, W)
    assert _same(first, m.host_params(7, 8, H, W))
    assert _same(first, BatchMixer(seed=3, rank=1, per_sample=per_sample, device="cpu").host_params(7, 8, H, W))
    assert not _same(first, m.host_params(8, 8, H, W))
    assert not _same(first, BatchMixer(seed=3, rank=2, per_sample=per_sample, device="cpu").host_params(7, 8, H, W))
    assert not _same(first, BatchMixer(seed=4, rank=1, per_sample=per_sample, device="cpu").host_params(7, 8, H, W))
    dev = m.params(7, 8, H, W)
    assert isinstance(dev, MixParams)
    assert dev.partner.dtype == torch.int32 and dev.lam.dtype == torch.float32 and dev.box.dtype == torch.int32
    assert dev.box.shape == (8, 4)
    assert _same(first, (dev.partner.numpy(), dev.lam.numpy(), dev.box.numpy()))


def _box_rule(lam, cy, cx):
    """The issue's formula, written out independently of mix.py."""
    cut_h = int(0.5 * math.sqrt(1.0 - lam) * H)
    cut_w = int(0.5 * math.sqrt(1.0 - lam) * W)
    y0, y1 = np.clip([cy - cut_h, cy + cut_h], 0, H)
    x0, x1 = np.clip([cx - cut_w, cx + cut_w], 0, W)
    return (int(y0), int(y1), int(x0), int(x1)), 1.0 - (y1 - y0) * (x1 - x0) / (H * W)


@pytest.mark.parametrize("lam,cy,cx,what", [
    (0.5, 12, 16, "interior"),
    (0.5, 1, 16, "clipped at the top"),
    (0.5, H - 1, 16, "clipped at the bottom"),
    (0.5, 12, 2, "clipped at the left"),
    (0.5, 12, W - 1, "clipped at the right"),
    (0.3, 0, 0, "clipped at a corner"),
    (0.0, 12, 16, "full image"),
    (0.999, 12, 16, "zero area"),
    (1.0, 5, 5, "zero area at lam 1"),
])
def test_cutmix_box_rule(lam, cy, cx, what):
    box, lam_adj = cutmix_box(lam, cy, cx, H, W)
    ref_box, ref_lam = _box_rule(lam, cy, cx)
    assert box == ref_box, what
    assert abs(lam_adj - ref_lam) < 1e-6, what
    y0, y1, x0, x1 = box
    assert 0 <= y0 <= y1 <= H and 0 <= x0 <= x1 <= W
    if what.startswith("zero area"):
        assert (y1 - y0) * (x1 - x0) == 0 and lam_adj == 1.0
    if what == "full image":
        assert box == (0, H, 0, W) and lam_adj == 0.0
    if "clipped" in what:
        assert (y1 - y0) * (x1 - x0) < (2 * int(0.5 * math.sqrt(1 - lam) * H)) * (2 * int(0.5 * math.sqrt(1 - lam) * W))


def test_drawn_boxes_follow_the_rule():
    """Every CutMix draw: the box is inside the image and lam is the clipped-area lam."""
    m = BatchMixer(mixup_alpha=0.0, cutmix_alpha=1.0, per_sample=True, seed=5, device="cpu")
    partner, lam, box = m.host_params(0, 256, H, W)
    assert sorted(partner.tolist()) == list(range(256))  # a permutation
    y0, y1, x0, x1 = box.T
    assert (0 <= y0).all() and (y0 <= y1).all() and (y1 <= H).all()
    assert (0 <= x0).all() and (x0 <= x1).all() and (x1 <= W).all()
    area = (y1 - y0) * (x1 - x0)
    assert np.array_equal(lam, (np.float32(1) - area.astype(np.float32) / np.float32(H * W)))
    assert (area > 0).any() and ((y0 == 0) | (y1 == H) | (x0 == 0) | (x1 == W)).any()


def test_batch_mode_rolls_and_shares_one_draw():
    m = BatchMixer(seed=1, device="cpu")
    seen_mixup = seen_cutmix = False
    for step in range(32):
        partner, lam, box = m.host_params(step, 6, H, W)
        assert partner.tolist() == [5, 0, 1, 2, 3, 4]
        assert (lam == lam[0]).all() and (box == box[0]).all()
        cut = (box[0, 1] - box[0, 0]) * (box[0, 3] - box[0, 2]) > 0
        seen_cutmix |= bool(cut)
        seen_mixup |= (not cut) and lam[0] < 1
    assert seen_mixup and seen_cutmix


def test_prob_zero_is_identity():
    for per_sample in (False, True):
        m = BatchMixer(prob=0.0, per_sample=per_sample, device="cpu")
        for step in range(4):
            _, lam, box = m.host_params(step, 8, H, W)
            assert (lam == 1).all() and not box.any()


def test_alpha_zero_disables_a_mode():
    only_mixup = BatchMixer(mixup_alpha=0.4, cutmix_alpha=0.0, per_sample=True, device="cpu")
    only_cutmix = BatchMixer(mixup_alpha=0.0, cutmix_alpha=1.0, per_sample=True, device="cpu")
    neither = BatchMixer(mixup_alpha=0.0, cutmix_alpha=0.0, per_sample=True, device="cpu")
    for step in range(4):
        _, lam, box = only_mixup.host_params(step, 64, H, W)
        assert not box.any() and (lam < 1).any()
        _, lam, box = only_cutmix.host_params(step, 64, H, W)
        area = (box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2])
        assert ((area > 0) | (lam == 1)).all() and (area > 0).any()  # never a blend
        _, lam, box = neither.host_params(step, 64, H, W)
        assert (lam == 1).all() and not box.any()


def test_out_of_range_partner_raises():
    m = BatchMixer(device="cpu")
    lam, box = np.ones(4, np.float32), np.zeros((4, 4), np.int32)
    m.upload(np.array([3, 0, 1, 2]), lam, box)
    with pytest.raises(ValueError):
        m.upload(np.array([3, 0, 1, 4]), lam, box)
    with pytest.raises(ValueError):
        m.upload(np.array([-1, 0, 1, 2]), lam, box)


def test_augment_mix_cpu_path():
    """Host tensors take the PyTorch path: normalize, then the same mixing rule and target."""
    g = torch.Generator().manual_seed(0)
    u8 = torch.randint(0, 256, (3, 4, 6, 3), dtype=torch.uint8, generator=g)
    labels = torch.tensor([4, 7, 9])
    mean, std = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)
    p = MixParams(torch.tensor([2, 0, 1], dtype=torch.int32), torch.tensor([0.25, 1.0, 0.9]),
                  torch.tensor([[0, 0, 0, 0], [0, 0, 0, 0], [1, 3, 2, 9]], dtype=torch.int32))
    x, t = augment_mix(u8, labels, 3, mean, std, p)
    base = (u8.float().div(255).permute(0, 3, 1, 2) - torch.tensor(mean).view(1, 3, 1, 1)) / torch.tensor(std).view(1, 3, 1, 1)
    assert torch.allclose(x[0], 0.25 * base[0] + 0.75 * base[2], atol=1e-6)
    assert torch.allclose(x[1], base[1], atol=1e-6)
    ref2 = base[2].clone()
    ref2[:, 1:3, 2:6] = base[1][:, 1:3, 2:6]
    assert torch.allclose(x[2], ref2, atol=1e-6)
    assert t.y_a.tolist() == [4, 7, 9] and t.y_b.tolist() == [9, 4, 7]
    assert torch.allclose(t.lam, torch.tensor([0.25, 1.0, 1 - 8 / 24]))
