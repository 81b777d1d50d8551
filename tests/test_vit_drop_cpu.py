"""Dropout / stochastic depth of the ViT without a GPU: the Philox known answers of the reference
helper, the per-layer schedule, the state_dict layout, the CPU (torch RNG) stochastic depth, argument
checks and the checkpoint round trip of the drop state."""
import numpy as np
import pytest
import torch

import drop_reference as R


def _vit(**kw):
    from mi355x_dp.models.vit import VisionTransformer
    return VisionTransformer(image_size=32, patch_size=16, num_layers=3, num_heads=1, hidden_dim=64, mlp_dim=128,
                             num_classes=10, **kw)


@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10([np.array([c]) for c in ctr], key)
    assert tuple(int(w[0]) for w in got) == want


def test_reference_mask_layout():
    """keep fraction near 1 - p, multiplier 65536 / (65536 - thr), expectation exactly 1 over the
    65536 draws, and the row mask constant over a sample's rows"""
    assert R.threshold(0.1) == 6554 and R.threshold(0.5) == 32768 and R.threshold(0.0) == 0
    m = R.element_mask(64, 256, 0.1, seed=7, rank=0, step=1, st=R.site(0, R.KIND_ATTN_DROP))
    kept = m != 0
    assert abs(kept.mean() - 0.9) < 0.02   # 16384 draws: sigma = 0.0023
    assert np.all(m[kept] == np.float32(65536.0) / np.float32(65536 - 6554))
    assert (65536 - 6554) * float(np.float32(65536.0) / np.float32(65536 - 6554)) / 65536 == pytest.approx(1.0, abs=1e-7)
    r = R.row_mask(37 * 9, 8, 9, 0.5, seed=7, rank=0, step=1, st=R.site(0, R.KIND_ATTN_PATH))
    assert np.all(r.reshape(37, 9 * 8) == r.reshape(37, 9 * 8)[:, :1])
    assert 0 < (r[::9, 0] == 0).sum() < 37
    # every input of the counter matters
    base = dict(seed=7, rank=0, step=1, st=3)
    a = R.sample_mask(64, 0.5, **base)
    for k, v in (("seed", 8), ("rank", 1), ("step", 2), ("st", 4)):
        assert not np.array_equal(a, R.sample_mask(64, 0.5, **{**base, k: v})), k
    assert np.array_equal(a, R.sample_mask(64, 0.5, **base))


def test_stochastic_depth_schedule():
    from mi355x_dp.models.vit import VisionTransformer, vit_b_16
    m = _vit(stochastic_depth_prob=0.2)
    ps = [b.stochastic_depth_prob for b in m.encoder.layers]
    assert ps == pytest.approx([0.0, 0.1, 0.2])
    assert [b.layer_index for b in m.encoder.layers] == [0, 1, 2]
    one = VisionTransformer(image_size=32, patch_size=16, num_layers=1, num_heads=1, hidden_dim=64, mlp_dim=128,
                            stochastic_depth_prob=0.3)
    assert one.encoder.layers[0].stochastic_depth_prob == pytest.approx(0.3)
    b16 = vit_b_16(stochastic_depth_prob=0.1, dropout=0.1)
    assert [b.stochastic_depth_prob for b in b16.encoder.layers] == pytest.approx([0.1 * l / 11 for l in range(12)])
    assert all(b.dropout.p == 0.1 for b in b16.encoder.layers)
    assert all(b.drop_state is b16.drop_state for b in b16.encoder.layers)


def test_state_dict_keys_unchanged():
    plain = _vit()
    drop = _vit(dropout=0.1, stochastic_depth_prob=0.2)
    assert list(drop.state_dict().keys()) == list(plain.state_dict().keys())
    assert not any("drop" in k for k in drop.state_dict())
    plain.load_state_dict(drop.state_dict())


@pytest.mark.parametrize("kw", [dict(stochastic_depth_prob=1.0), dict(stochastic_depth_prob=-0.1), dict(dropout=1.0),
                                dict(dropout=-0.5), dict(stochastic_depth_prob=float("nan"))])
def test_probability_range(kw):
    from mi355x_dp.models.vit import EncoderBlock
    from mi355x_dp.ops import transformer as Tm
    with pytest.raises(ValueError):
        _vit(**kw)
    with pytest.raises(ValueError):
        EncoderBlock(1, 64, 128, **kw)
    with pytest.raises(ValueError):
        Tm.drop_threshold(next(iter(kw.values())))


def test_drop_threshold_matches_reference():
    from mi355x_dp.ops import transformer as Tm
    for p in (0.0, 0.05, 0.1, 0.2, 0.5, 0.75, 0.999):
        assert Tm.drop_threshold(p) == R.threshold(p)


def test_cpu_stochastic_depth_rows():
    """eval: identity (the block equals a block without the argument); training: each sample's
    branch contribution is 0 or the undropped one scaled by 1 / (1 - p)"""
    from mi355x_dp.models.vit import EncoderBlock
    p = 0.5
    torch.manual_seed(3)
    blk = EncoderBlock(1, 64, 128, stochastic_depth_prob=p)
    ref = EncoderBlock(1, 64, 128)
    ref.load_state_dict(blk.state_dict())
    x = torch.randn(64, 5, 64)
    blk.eval(), ref.eval()
    with torch.no_grad():
        assert torch.equal(blk(x), ref(x))
        # the two branches, undropped
        a = ref.self_attention(ref.ln_1(x))
        blk.train()
        torch.manual_seed(11)
        z = blk(x)
        # branch 1: y = x + m1 * a, m1 in {0, 1 / (1 - p)} per sample; recover it from the output by
        # trying both values per sample
        scale = 1.0 / (1.0 - p)
        seen = set()
        for b in range(x.shape[0]):
            ok = False
            for m1 in (0.0, scale):
                y = x[b] + m1 * a[b]
                f = ref.mlp(ref.ln_2(y[None]))[0]
                for m2 in (0.0, scale):
                    if torch.allclose(z[b], y + m2 * f, atol=1e-5):
                        ok = True
                        seen.add((m1, m2))
            assert ok, b
        assert len(seen) == 4   # 64 samples at p = 0.5: all four combinations occur
        # torch's RNG drives it: the same seed repeats, another differs
        torch.manual_seed(11)
        assert torch.equal(blk(x), z)
        assert not torch.equal(blk(x), z)


def test_drop_state_host():
    from mi355x_dp.ops import transformer as Tm
    s = Tm.DropState(seed=0x123456789abcdef0, rank=3)
    assert (s.seed, s.rank, s.step) == (0x123456789abcdef0, 3, 0)
    s.advance()
    s.advance()
    assert s.step == 2
    s.step = 40
    assert s.state_dict() == {"seed": 0x123456789abcdef0, "rank": 3, "step": 40}
    t = Tm.DropState(rank=5)
    t.load_state_dict(s.state_dict())
    assert (t.seed, t.rank, t.step) == (0x123456789abcdef0, 5, 40)   # the rank stays the process's own
    t.reseed(9, rank=1)
    assert (t.seed, t.rank, t.step) == (9, 1, 0)
    assert Tm.DropState().rank == 0   # no process group
    with pytest.raises(ValueError):
        Tm.DropState(rank=65536)


def test_checkpoint_round_trip(tmp_path):
    from mi355x_dp.utils.checkpoint import load_checkpoint, save_checkpoint
    m = _vit(dropout=0.1, stochastic_depth_prob=0.2)
    m.drop_state.reseed(1234)
    m.drop_state.step = 17
    path = str(tmp_path / "ckpt.pt")
    save_checkpoint(path, m, step=5)
    m2 = _vit(dropout=0.1, stochastic_depth_prob=0.2)
    assert m2.drop_state.step == 0
    info = load_checkpoint(path, m2)
    assert info["step"] == 5
    assert (m2.drop_state.seed, m2.drop_state.step) == (1234, 17)
    for (k, a), (_, b) in zip(m.state_dict().items(), m2.state_dict().items()):
        assert torch.equal(a, b), k
    # a model without the state loads the same file; a checkpoint without it leaves the state alone
    m3 = torch.nn.Linear(2, 2)
    m3.load_state_dict = lambda sd: None
    load_checkpoint(path, m3)
