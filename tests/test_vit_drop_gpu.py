"""Dropout and stochastic depth inside the fused ViT encoder layer (csrc/kernels/philox.h, drop.hip,
the dropped GEMM epilogues) against the numpy mask reference of drop_reference.py."""
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import drop_reference as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SEED, STEP, RANK = 0x9E3779B97F4A7C15, (1 << 32) + 5, 3   # both 64-bit words and the rank in play


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mi355x_dp.ops import _lib
    _lib.load(True)
    torch.manual_seed(0)


@pytest.fixture(params=[0, 2], ids=["bm256", "bm224"])
def bm224(request):
    """the gemm256 NT kernel's row tile: 256 rows or forced 224 rows (as test_gemm256_gpu.py)"""
    from mi355x_dp.ops import _lib
    lib = _lib.load()
    lib.mi_set_g256_bm224(request.param)
    yield request.param
    lib.mi_set_g256_bm224(1)


def rel_err(a, b):
    a = a.detach().float()
    b = b.detach().float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(BF)


def block_of(seed=SEED, step=STEP):
    """a device state block [seed, step]"""
    s = seed - (1 << 64) if seed >= (1 << 63) else seed
    return torch.tensor([s, step], dtype=torch.int64, device="cuda")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def dev_mask(M, N, p_e=0.0, st_e=0, p_r=0.0, st_r=0, rps=1, seed=SEED, step=STEP, rank=RANK):
    from mi355x_dp.ops import transformer as Tm
    m = Tm.drop_mask(M, N, block_of(seed, step), rank, st_e, Tm.drop_threshold(p_e), st_r, Tm.drop_threshold(p_r), rps)
    torch.cuda.synchronize()
    return m


def ref_mask(M, N, p_e=0.0, st_e=0, p_r=0.0, st_r=0, rps=1, seed=SEED, step=STEP, rank=RANK):
    return torch.from_numpy(R.combined_mask(M, N, p_e, st_e, p_r, st_r, rps, seed, rank, step))


# ------------------------------------------------------------------ mi_drop_mask
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_drop_mask_elements_bit_equal(p):
    M, N = 333, 256
    got = dev_mask(M, N, p_e=p, st_e=R.site(2, R.KIND_MLP_DROP))
    want = ref_mask(M, N, p_e=p, st_e=R.site(2, R.KIND_MLP_DROP))
    assert torch.equal(bits(got), bits(want))
    assert 0 < int((want == 0).sum()) < M * N


def test_drop_mask_rows_bit_equal():
    B, T, N = 37, 9, 64
    got = dev_mask(B * T, N, p_r=0.5, st_r=R.site(1, R.KIND_ATTN_PATH), rps=T)
    want = ref_mask(B * T, N, p_r=0.5, st_r=R.site(1, R.KIND_ATTN_PATH), rps=T)
    assert torch.equal(bits(got), bits(want))
    per_sample = want.view(B, T * N)
    assert 0 < int((per_sample[:, 0] == 0).sum()) < B
    both = dev_mask(B * T, N, p_e=0.1, st_e=8, p_r=0.5, st_r=11, rps=T)
    assert torch.equal(bits(both), bits(ref_mask(B * T, N, p_e=0.1, st_e=8, p_r=0.5, st_r=11, rps=T)))


def test_drop_mask_depends_on_every_input():
    M, N = 333, 256
    base = dict(seed=SEED, step=STEP, rank=RANK, st_e=5)
    a = dev_mask(M, N, p_e=0.5, **base)
    assert torch.equal(bits(a), bits(dev_mask(M, N, p_e=0.5, **base)))
    for k, v in (("seed", SEED ^ (1 << 40)), ("rank", RANK + 1), ("step", STEP + 1), ("step", STEP ^ (1 << 32)),
                 ("st_e", 6)):
        assert not torch.equal(bits(a), bits(dev_mask(M, N, p_e=0.5, **{**base, k: v}))), k
    rows = dict(seed=SEED, step=STEP, rank=RANK, st_r=3, rps=9)
    r = dev_mask(M, N, p_r=0.5, **rows)
    for k, v in (("seed", SEED + 1), ("rank", 0), ("step", STEP - 1), ("st_r", 4)):
        assert not torch.equal(bits(r), bits(dev_mask(M, N, p_r=0.5, **{**rows, k: v}))), k


def test_drop_entry_points_refuse_bad_arguments():
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    lib = _lib.load()
    out = torch.empty(64, 64, device="cuda")
    blk = block_of()
    st = stream_of(out)
    assert lib.mi_drop_mask(ptr(out), 64, 64, ptr(blk), 65536, 0, 0, 0, 0, 1, st) != 0    # thr: p would be 1
    assert lib.mi_drop_mask(ptr(out), 64, 64, ptr(blk), 100, 65536, 0, 0, 0, 1, st) != 0  # site
    assert lib.mi_drop_mask(ptr(out), 64, 64, ptr(blk), 100, 0, 0, 0, 65536, 1, st) != 0  # rank
    assert lib.mi_drop_mask(ptr(out), 64, 60, ptr(blk), 100, 0, 0, 0, 0, 1, st) != 0      # N % 8
    assert lib.mi_drop_mask(ptr(out), 1 << 20, 1 << 15, ptr(blk), 100, 0, 0, 0, 0, 1, st) != 0  # M N / 8 >= 2^32
    assert lib.mi_drop_mask(ptr(out), 64, 64, ptr(None), 100, 0, 0, 0, 0, 1, st) != 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------ dropped GEMM epilogues
MASKS = {"element": dict(p_e=0.1, st_e=R.site(1, R.KIND_ATTN_DROP)),
         "row": dict(p_r=0.5, st_r=R.site(1, R.KIND_ATTN_PATH)),
         "both": dict(p_e=0.1, st_e=R.site(1, R.KIND_ATTN_DROP), p_r=0.5, st_r=R.site(1, R.KIND_ATTN_PATH))}


def gemm_drop(route, kind, a, w, bias, aux, rps, p_e=0.0, st_e=0, p_r=0.0, st_r=0):
    """route "epi": mi_gemm_nt_epi_drop (these shapes: the 128-tile kernels); "g256": the 256-wide kernel"""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops import transformer as Tm
    from mi355x_dp.ops._lib import ptr, stream_of
    M, K = a.shape
    N = w.shape[0]
    out = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    if kind == Tm.DROP_GELU:
        aux = torch.full((M, N), float("nan"), dtype=BF, device="cuda")
    _lib.call("mi_gemm_nt_epi_drop" if route == "epi" else "mi_gemm256_nt_drop", ptr(a), ptr(w), ptr(out), ptr(bias),
              ptr(aux), kind, M, N, K, K, K, N, ptr(block_of()), Tm.drop_threshold(p_e), st_e, Tm.drop_threshold(p_r),
              st_r, RANK, rps, stream_of(a))
    torch.cuda.synchronize()
    return (out, aux) if kind == Tm.DROP_GELU else out


def check_residual_drop(route, M, N, K, rps, mask):
    from mi355x_dp.ops import transformer as Tm
    a, w = rnd(M, K), rnd(N, K, scale=0.1)
    bias = torch.randn(N, device="cuda") * 0.1
    aux = rnd(M, N)
    v = Tm._gemm(a, w, bias).float()              # the epi-0 result: bf16(acc + bias)
    m = ref_mask(M, N, rps=rps, **mask).cuda()
    dropped = m == 0
    assert 0 < int(dropped.sum()) < M * N
    out = gemm_drop(route, Tm.DROP_RESIDUAL, a, w, bias, aux, rps, **mask)
    assert torch.equal(bits(out[dropped]), bits(aux[dropped]))       # bit-equal to aux where dropped
    ref = v * m + aux.float()
    kept_err = float((out.float() - ref)[~dropped].abs().max() / ref[~dropped].abs().max())
    print(f"residual-drop {route} {M}x{N}x{K}: kept rel err {kept_err:.3e}")
    assert kept_err < 2e-2
    # the dropped set itself: with aux = 0 the output is zero exactly where the mask (or v) is
    out0 = gemm_drop(route, Tm.DROP_RESIDUAL, a, w, bias, torch.zeros_like(aux), rps, **mask)
    return (out0 == 0) | (v == 0), dropped | (v == 0)


def check_gelu_drop(route, M, N, K):
    from mi355x_dp.ops import transformer as Tm
    mask = dict(p_e=0.1, st_e=R.site(1, R.KIND_GELU_DROP))
    a, w = rnd(M, K), rnd(N, K, scale=0.1)
    bias = torch.randn(N, device="cuda") * 0.1
    v = Tm._gemm(a, w, bias).float()
    m = ref_mask(M, N, **mask).cuda()
    dropped = m == 0
    assert 0 < int(dropped.sum()) < M * N
    out, u = gemm_drop(route, Tm.DROP_GELU, a, w, bias, None, 1, **mask)
    assert not bits(out[dropped]).any() and not bits(u[dropped]).any()   # +0 bit patterns
    x = v.clone().requires_grad_()
    g = F.gelu(x)
    g.backward(torch.ones_like(g))
    e_out = float((out.float() - g.detach() * m)[~dropped].abs().max() / (g.detach() * m)[~dropped].abs().max())
    e_u = float((u.float() - x.grad * m)[~dropped].abs().max() / (x.grad * m)[~dropped].abs().max())
    print(f"gelu-drop {route} {M}x{N}x{K}: kept rel err out {e_out:.3e} gelu' {e_u:.3e}")
    assert e_out < 2e-2 and e_u < 2e-2
    return u == 0, dropped


@pytest.mark.parametrize("mask", list(MASKS), ids=list(MASKS))
def test_residual_drop_128_tile(mask):
    got, want = check_residual_drop("epi", 333, 256, 192, 9, MASKS[mask])    # 333 = 37 samples x 9 rows
    assert torch.equal(got, want)


def test_gelu_drop_128_tile():
    got, want = check_gelu_drop("epi", 333, 256, 192)
    assert torch.equal(got, want)


@pytest.mark.parametrize("mask", list(MASKS), ids=list(MASKS))
def test_residual_drop_gemm256(mask, bm224):
    """the 256-wide kernel called directly, both row-tile heights; its dropped set is the reference's
    and the 128-tile route's at the same shape"""
    M, N, K = 1000, 776, 200
    torch.manual_seed(5)
    got, want = check_residual_drop("g256", M, N, K, 8, MASKS[mask])         # 125 samples x 8 rows
    assert torch.equal(got, want)
    torch.manual_seed(5)
    got128, want128 = check_residual_drop("epi", M, N, K, 8, MASKS[mask])
    assert torch.equal(got128, want128) and torch.equal(want128, want) and torch.equal(got, got128)


def test_gelu_drop_gemm256(bm224):
    M, N, K = 1000, 776, 200
    torch.manual_seed(6)
    got, want = check_gelu_drop("g256", M, N, K)
    assert torch.equal(got, want)
    torch.manual_seed(6)
    got128, _ = check_gelu_drop("epi", M, N, K)
    assert torch.equal(got, got128)


# ------------------------------------------------------------------ mi_drop_bwd
@pytest.mark.parametrize("mask", list(MASKS), ids=list(MASKS))
def test_drop_bwd_bit_equal(mask):
    from mi355x_dp.ops import transformer as Tm
    M, N, rps = 333, 256, 9
    kw = MASKS[mask]
    dz = rnd(M, N)
    d = Tm._Drop()
    d.snap, d.rank = block_of(), RANK
    out = Tm._drop_bwd(dz, d, kw.get("st_e", 0), Tm.drop_threshold(kw.get("p_e", 0.0)), kw.get("st_r", 0),
                       Tm.drop_threshold(kw.get("p_r", 0.0)), rps)
    torch.cuda.synchronize()
    m = ref_mask(M, N, rps=rps, **kw).cuda()
    assert torch.equal(bits(out), bits((dz.float() * m).to(BF)))
    assert torch.equal(bits(dev_mask(M, N, rps=rps, **kw)), bits(m))


# ------------------------------------------------------------------ the fused layer
B_, T_, D_, HEADS, MLP, LAYER = 3, 17, 128, 2, 256, 2


def _block(dropout, sd):
    from mi355x_dp.models.vit import EncoderBlock
    torch.manual_seed(1)
    blk = EncoderBlock(HEADS, D_, MLP, dropout=dropout, stochastic_depth_prob=sd, layer_index=LAYER)
    with torch.no_grad():  # non-trivial LN affine / biases
        for n, p in blk.named_parameters():
            if "ln" in n:
                p.add_(torch.randn_like(p) * 0.1)
            elif n.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.05)
    return blk


def _layer_masks(dropout, sd, seed, step, rank=0):
    """numpy masks of the layer's three dropped tensors at (seed, step), and the per-sample masks"""
    M = B_ * T_
    kw = dict(rows_per_sample=T_, seed=seed, rank=rank, step=step)
    m_attn = R.combined_mask(M, D_, dropout, R.site(LAYER, R.KIND_ATTN_DROP), sd, R.site(LAYER, R.KIND_ATTN_PATH), **kw)
    m_gelu = R.element_mask(M, MLP, dropout, seed, rank, step, R.site(LAYER, R.KIND_GELU_DROP))
    m_mlp = R.combined_mask(M, D_, dropout, R.site(LAYER, R.KIND_MLP_DROP), sd, R.site(LAYER, R.KIND_MLP_PATH), **kw)
    s_attn = R.sample_mask(B_, sd, seed, rank, step, R.site(LAYER, R.KIND_ATTN_PATH))
    s_mlp = R.sample_mask(B_, sd, seed, rank, step, R.site(LAYER, R.KIND_MLP_PATH))
    t = lambda a, n: torch.from_numpy(a).view(B_, T_, n)
    return t(m_attn, D_), t(m_gelu, MLP), t(m_mlp, D_), s_attn, s_mlp


def _pick_seed(sd, step):
    """first seed whose two branches each drop and keep a sample, with one sample dropped in both"""
    for seed in range(1, 4096):
        a = R.sample_mask(B_, sd, seed, 0, step, R.site(LAYER, R.KIND_ATTN_PATH)) == 0
        m = R.sample_mask(B_, sd, seed, 0, step, R.site(LAYER, R.KIND_MLP_PATH)) == 0
        if 0 < a.sum() < B_ and 0 < m.sum() < B_ and (a & m).any():
            return seed
    raise AssertionError("no seed")


def _ref_block(blk, x, masks):
    """the module's fp32 CPU path with the reference masks as the dropped branches' multipliers"""
    m_attn, m_gelu, m_mlp = masks
    y = x + blk.self_attention(blk.ln_1(x)) * m_attn
    h = F.gelu(blk.mlp[0](blk.ln_2(y))) * m_gelu
    return y + blk.mlp[3](h) * m_mlp


@pytest.mark.parametrize("dropout,sd", [(0.1, 0.0), (0.0, 0.5), (0.1, 0.5)], ids=["dropout", "path", "both"])
def test_encoder_layer_drop_matches_fp32(dropout, sd, monkeypatch):
    from mi355x_dp.ops import transformer as Tm
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    step = 7                                   # the block advances its state to 7 before it draws
    seed = _pick_seed(sd, step) if sd else 12345
    m_attn, m_gelu, m_mlp, s_attn, s_mlp = _layer_masks(dropout, sd, seed, step)
    if sd:
        assert 0 < (s_attn == 0).sum() < B_ and 0 < (s_mlp == 0).sum() < B_
    torch.manual_seed(2)
    x = (torch.randn(B_, T_, D_) * 0.5).to(BF).float()
    dz = (torch.randn(B_, T_, D_) * 0.1).to(BF).float()
    ref_blk = _block(dropout, sd).eval()       # eval: the module's own dropouts off, the masks explicit
    xr = x.clone().requires_grad_()
    zr = _ref_block(ref_blk, xr, (m_attn, m_gelu, m_mlp))
    zr.backward(dz)
    blk = _block(dropout, sd).cuda().train()
    blk.drop_state = Tm.DropState(seed=seed, rank=0)
    blk.drop_state.step = step - 1
    xg = x.cuda().to(BF).requires_grad_()
    zg = blk(xg)
    zg.backward(dz.cuda().to(BF))
    torch.cuda.synchronize()
    assert blk.drop_state.step == step
    errs = {"out": rel_err(zg.cpu(), zr), "dx": rel_err(xg.grad.cpu(), xr.grad)}
    print(f"layer dropout={dropout} sd={sd}: out {errs['out']:.3e} dx {errs['dx']:.3e}")
    assert errs["out"] < 3e-2
    assert errs["dx"] < 5e-2
    for (n, p), (_, pr) in zip(blk.named_parameters(), ref_blk.named_parameters()):
        assert p.grad is not None, n
        e = rel_err(p.grad.cpu(), pr.grad)
        print(f"  {n}: {e:.3e}")
        assert e < 6e-2, n
    if sd:
        both = np.nonzero((s_attn == 0) & (s_mlp == 0))[0]
        assert len(both) > 0
        for b in both:
            assert torch.equal(zg[b].cpu(), xg[b].detach().cpu())
            assert torch.equal(xg.grad[b].cpu(), dz[b].to(BF))


# ------------------------------------------------------------------ the model
def _vit(**kw):
    from mi355x_dp.models.vit import VisionTransformer
    torch.manual_seed(0)
    m = VisionTransformer(image_size=32, patch_size=16, num_layers=2, num_heads=1, hidden_dim=64, mlp_dim=128,
                          num_classes=10, **kw)
    with torch.no_grad():  # the zero-initialised head / class token would make the checks trivial
        m.heads.head.weight.normal_(std=0.2)
        m.class_token.normal_(std=0.5)
    return m


def test_vit_drop_trains_native(monkeypatch):
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    m = _vit(dropout=0.1, stochastic_depth_prob=0.2).cuda().train()
    x = torch.randn(8, 3, 32, 32, device="cuda")
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        out = m(x)
        F.cross_entropy(out.float(), torch.arange(8, device="cuda")).backward()
        torch.cuda.synchronize()
    assert not [w for w in rec if "scaled_dot_product_attention" in str(w.message)]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    assert m.drop_state.step == 1
    with torch.no_grad():
        a, b = m(x), m(x)                       # steps 2, 3: new masks every training forward
        assert not torch.equal(a, b)
        m.drop_state.step = 1
        assert torch.equal(m(x), a)             # step 2 again: the same bits
        m.drop_state.step = 1
        m.drop_state.reseed(99)
        m.drop_state.step = 1
        assert not torch.equal(m(x), a)
        # eval: the all-zero model's bits; training at all-zero: the bits of a model without the arguments
        zero = _vit(dropout=0.0, stochastic_depth_prob=0.0).cuda()
        plain = _vit().cuda()
        zero.load_state_dict(m.state_dict())
        plain.load_state_dict(m.state_dict())
        assert torch.equal(m.eval()(x), zero.eval()(x))
        assert torch.equal(zero.train()(x), plain.train()(x))
        assert zero.drop_state.step == 0        # inactive: no state traffic at all


def test_encoder_block_drop_graph_capture(monkeypatch):
    """forward + backward of the dropped block captured in one graph (single stream): every replay
    advances the device step and draws new masks, and equals the eager run at that step bit for bit
    (output and input gradient).  Warm-up, capture and the eager runs share one stream, so they use the
    same per-stream workspaces and schedules.  The parameter gradients of the LayerNorms and biases are
    fp32 sums whose order is not fixed (atomics): those are held to 1e-4 of the largest entry -- a
    reordered fp32 sum of B T = 51 terms moves by at most 51 x 2^-24 = 3e-6 of the terms' magnitude."""
    from mi355x_dp.ops import transformer as Tm
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    blk = _block(0.1, 0.5).cuda().train()
    blk.drop_state = Tm.DropState(seed=4242, rank=0)
    params = list(blk.parameters())
    x = (torch.randn(B_, T_, D_, device="cuda") * 0.5).to(BF)
    dz = (torch.randn(B_, T_, D_, device="cuda") * 0.1).to(BF)

    def step(xin):
        z = blk(xin)
        return (z,) + torch.autograd.grad(z, [xin] + params, dz)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as torch's capture recipe
        step(x.clone().requires_grad_())
    torch.cuda.current_stream().wait_stream(side)
    xs = x.clone().requires_grad_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        outs = step(xs)
    torch.cuda.synchronize()
    blk.drop_state.step = 10
    replays = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        replays.append([o.clone() for o in outs])
    assert blk.drop_state.step == 13
    assert not torch.equal(replays[0][0], replays[1][0]) and not torch.equal(replays[1][0], replays[2][0])
    assert not torch.equal(replays[0][0], replays[2][0])
    for k, rep in enumerate(replays):
        blk.drop_state.step = 10 + k
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            eager = step(x.clone().requires_grad_())
        torch.cuda.synchronize()
        assert torch.equal(rep[0], eager[0]) and torch.equal(rep[1], eager[1])
        for a, b in zip(rep[2:], eager[2:]):
            assert rel_err(a, b) < 1e-4
