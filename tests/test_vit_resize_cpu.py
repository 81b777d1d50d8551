"""interpolate_embeddings: a ViT state dict's position embedding resized to another resolution."""
import pytest
import torch

D = 32


def _model(image_size):
    from mi355x_dp.models.vit import VisionTransformer
    torch.manual_seed(0)
    return VisionTransformer(image_size=image_size, patch_size=16, num_layers=1, num_heads=2, hidden_dim=D,
                             mlp_dim=64, num_classes=5)


def test_same_size_is_unchanged():
    from mi355x_dp.models import interpolate_embeddings
    state = _model(64).state_dict()
    out = interpolate_embeddings(64, 16, state)
    assert out is not state
    assert torch.equal(out["encoder.pos_embedding"], state["encoder.pos_embedding"])


@pytest.mark.parametrize("mode", ["bicubic", "bilinear"])
def test_resized_grid(mode):
    from mi355x_dp.models.vit import interpolate_embeddings
    state = _model(64).state_dict()
    pos = state["encoder.pos_embedding"].clone()
    out = interpolate_embeddings(96, 16, state, interpolation_mode=mode)
    new = out["encoder.pos_embedding"]
    assert torch.equal(state["encoder.pos_embedding"], pos)  # the input state is left alone
    assert tuple(new.shape) == (1, 1 + 36, D)
    assert torch.equal(new[:, 0], pos[:, 0])                 # class token row: bit-equal
    old_g, new_g = pos[0, 1:].view(4, 4, D), new[0, 1:].view(6, 6, D)
    for (a, b), (c, d) in zip(((0, 0), (0, 3), (3, 0), (3, 3)), ((0, 0), (0, 5), (5, 0), (5, 5))):
        assert float((new_g[c, d] - old_g[a, b]).abs().max()) < 1e-6  # align_corners=True
    for k, v in state.items():
        if k != "encoder.pos_embedding":
            assert out[k] is v


def test_constant_grid_stays_constant():
    from mi355x_dp.models.vit import interpolate_embeddings
    state = _model(64).state_dict()
    state["encoder.pos_embedding"] = torch.full((1, 17, D), 0.375)
    new = interpolate_embeddings(96, 16, state)["encoder.pos_embedding"]
    assert float((new - 0.375).abs().max()) < 1e-6


def test_resized_state_loads_strictly():
    from mi355x_dp.models.vit import interpolate_embeddings
    state = _model(64).state_dict()
    big = _model(96)
    with pytest.raises(RuntimeError):
        big.load_state_dict(state, strict=True)
    big.load_state_dict(interpolate_embeddings(96, 16, state), strict=True)
    assert tuple(big.encoder.pos_embedding.shape) == (1, 37, D)
