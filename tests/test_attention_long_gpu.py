"""The slab-streaming attention kernels (csrc/kernels/attention.hip: mi_attn_fwd_long /
mi_attn_bwd_long, head dim 64, any T >= 1) against fp32 references, against the resident-operand
kernels where both apply, and for what they may touch, repeatability, refusals and graph capture.
Helpers and bounds as tests/test_transformer_gpu.py."""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mi355x_dp.ops import _lib
    _lib.load(True)
    torch.manual_seed(0)


def rel_err(a, b):
    a = a.detach().float()
    b = b.detach().float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device="cuda") * scale).to(BF)


def _fwd(name, qkv, o, lse, B, T, H):
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    _lib.call(name, ptr(qkv), ptr(o), ptr(lse), B, T, H, 0.125, stream_of(qkv))


def _bwd(name, qkv, o, do, lse, dvec, dqkv, B, T, H):
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    _lib.call(name, ptr(qkv), ptr(o), ptr(do), ptr(lse), ptr(dvec), ptr(dqkv), B, T, H, 0.125, stream_of(qkv))


def _run(suffix, qkv, do, B, T, H):
    """forward + backward through the C entry points into fresh buffers: (o, lse, dqkv)"""
    D = H * 64
    o = torch.empty(B * T, D, dtype=BF, device="cuda")
    lse = torch.empty(B * H * T, device="cuda")
    dvec = torch.empty(B * H * T, device="cuda")
    dqkv = torch.full((B * T, 3 * D), float("nan"), dtype=BF, device="cuda")
    _fwd("mi_attn_fwd" + suffix, qkv, o, lse, B, T, H)
    _bwd("mi_attn_bwd" + suffix, qkv, o, do, lse, dvec, dqkv, B, T, H)
    torch.cuda.synchronize()
    return o, lse, dqkv


@pytest.mark.parametrize("B,T,H", [(2, 257, 2), (1, 288, 1), (2, 512, 1), (1, 513, 2), (2, 577, 3), (1, 1025, 1),
                                   (1, 4097, 1)])
def test_long_attention_matches_fp32(B, T, H, monkeypatch):
    """Tm.attention above the resident kernels' 256 tokens against fp32 SDPA on the same
    bf16-rounded inputs, with test_attention_fwd_bwd's bounds.  STRICT_NATIVE makes a fallback an
    error, so the native pair is what is compared."""
    from mi355x_dp.ops import transformer as Tm
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    D = H * 64
    qkv = rnd(B * T, 3 * D, scale=1.5)
    do = rnd(B * T, D)
    x = qkv.clone().requires_grad_()
    o = Tm.attention(x, B, T, H)
    o.backward(do)
    xr = qkv.float().requires_grad_()
    q, k, v = xr.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    orf = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * T, D)
    orf.backward(do.float())
    e_o = rel_err(o, orf)
    dq, dr = x.grad.view(B * T, 3, D), xr.grad.view(B * T, 3, D)
    e_g = [rel_err(dq[:, i], dr[:, i]) for i in range(3)]
    print(f"T={T}: O {e_o:.2e}  dQ {e_g[0]:.2e}  dK {e_g[1]:.2e}  dV {e_g[2]:.2e}")
    assert torch.isfinite(x.grad.float()).all()
    assert e_o < 2e-2
    for e, name in zip(e_g, "qkv"):
        assert e < 4e-2, name


def test_long_attention_late_and_early_score_spikes(monkeypatch):
    """The forward's running max must be able to jump in any slab and to stay put for the rest: one
    query meets a dominant key in the last slab (score ~ +36 against ~ +-2: every earlier chunk is
    rescaled by e^-34), another in the first chunk (no later chunk raises the max).  Same reference
    and bounds as above."""
    from mi355x_dp.ops import transformer as Tm
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    B, T, H = 1, 577, 2
    D = H * 64
    qkv = rnd(B * T, 3 * D, scale=1.5)
    qkv[560, D:D + 64] = 2 * qkv[10, 0:64]             # head 0: key 560 (slab 4) = 2 x query 10
    qkv[3, D + 64:D + 128] = 2 * qkv[300, 64:128]      # head 1: key 3 (slab 0) = 2 x query 300
    do = rnd(B * T, D)
    x = qkv.clone().requires_grad_()
    o = Tm.attention(x, B, T, H)
    o.backward(do)
    xr = qkv.float().requires_grad_()
    q, k, v = xr.view(B, T, 3, H, 64).permute(2, 0, 3, 1, 4).unbind(0)
    p = torch.softmax(q @ k.transpose(-1, -2) * 0.125, -1)
    pd = p.detach()
    assert float(pd[0, 0, 10, 560]) > 0.999 and float(pd[0, 1, 300, 3]) > 0.999  # the spikes dominate
    orf = (p @ v).transpose(1, 2).reshape(B * T, D)
    orf.backward(do.float())
    assert rel_err(o, orf) < 2e-2
    assert rel_err(o[10, :64], orf[10, :64]) < 2e-2 and rel_err(o[300, 64:], orf[300, 64:]) < 2e-2
    dq, dr = x.grad.view(B * T, 3, D), xr.grad.view(B * T, 3, D)
    for i, name in enumerate("qkv"):
        assert rel_err(dq[:, i], dr[:, i]) < 4e-2, name


@pytest.mark.parametrize("B,T,H", [(2, 197, 12), (3, 17, 2), (2, 129, 1), (2, 256, 3), (4, 1, 1)])
def test_long_kernels_agree_with_resident(B, T, H):
    """At T <= 256 both kernel sets apply: same O, LSE and gradients to rounding (the long forward
    rescales per 64-key chunk like the 8-wave resident forward; the backward sums the same terms)."""
    D = H * 64
    qkv = rnd(B * T, 3 * D, scale=1.5)
    do = rnd(B * T, D)
    o_r, lse_r, g_r = _run("", qkv, do, B, T, H)
    o_l, lse_l, g_l = _run("_long", qkv, do, B, T, H)
    assert rel_err(o_l, o_r) < 1e-2
    assert float((lse_l - lse_r).abs().max()) < 1e-4
    g_l, g_r = g_l.view(B * T, 3, D), g_r.view(B * T, 3, D)
    for i, name in enumerate("qkv"):
        if float(g_r[:, i].float().abs().max()) < 1e-4:  # T == 1: dQ, dK are exactly zero
            assert float(g_l[:, i].float().abs().max()) < 1e-4, name
        else:
            assert rel_err(g_l[:, i], g_r[:, i]) < 1e-2, name


def _padded(t, tail, fill):
    """``t`` as the head of a longer buffer whose ``tail`` extra rows (elements, for 1-D) hold
    ``fill``: (view of the head, view of the tail)"""
    buf = torch.full((t.shape[0] + tail,) + tuple(t.shape[1:]), fill, dtype=t.dtype, device=t.device)
    buf[:t.shape[0]].copy_(t)
    return buf[:t.shape[0]], buf[t.shape[0]:]


def _bits(t):
    return t.view(torch.int16 if t.dtype == BF else torch.int32)


@pytest.mark.parametrize("B,T,H", [(2, 257, 2), (1, 577, 1)])
def test_long_kernels_stay_inside_their_rows(B, T, H):
    """Inputs followed by NaN rows, outputs followed by a sentinel tail: the tails keep their bits,
    every output is finite, and the results equal those of the unpadded run bit for bit."""
    D = H * 64
    qkv = rnd(B * T, 3 * D, scale=1.5)
    do = rnd(B * T, D)
    o_ref, lse_ref, g_ref = _run("_long", qkv, do, B, T, H)
    nan = float("nan")
    qkv_p, _ = _padded(qkv, 64, nan)
    do_p, _ = _padded(do, 64, nan)
    o, o_tail = _padded(torch.zeros_like(o_ref), 64, 1234.0)
    lse, lse_tail = _padded(torch.zeros_like(lse_ref), 1024, -7777.25)
    dvec, dvec_tail = _padded(torch.zeros_like(lse_ref), 1024, -7777.25)
    dqkv, g_tail = _padded(torch.zeros_like(g_ref), 64, 1234.0)
    tails = [o_tail, lse_tail, dvec_tail, g_tail]
    before = [_bits(t).clone() for t in tails]
    _fwd("mi_attn_fwd_long", qkv_p, o, lse, B, T, H)
    o_in, _ = _padded(o, 64, nan)  # the forward's output as a backward input, NaN rows behind it
    _bwd("mi_attn_bwd_long", qkv_p, o_in, do_p, lse, dvec, dqkv, B, T, H)
    torch.cuda.synchronize()
    for t, b in zip(tails, before):
        assert torch.equal(_bits(t), b)
    for t in (o, lse, dvec, dqkv):
        assert torch.isfinite(t.float()).all()
    assert torch.equal(o, o_ref) and torch.equal(lse, lse_ref) and torch.equal(dqkv, g_ref)


def test_long_kernels_deterministic():
    B, T, H = 2, 577, 3
    qkv = rnd(B * T, 3 * H * 64, scale=1.5)
    do = rnd(B * T, H * 64)
    a = _run("_long", qkv, do, B, T, H)
    b = _run("_long", qkv, do, B, T, H)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_long_kernels_refuse_out_of_range():
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    lib = _lib.load(True)
    tmax = int(lib.mi_attn_long_max_seq())
    assert tmax >= 8192
    qkv = rnd(257, 192)
    o = torch.empty(257, 64, dtype=BF, device="cuda")
    lse = torch.empty(257, device="cuda")
    for T in (0, tmax + 1):
        assert lib.mi_attn_fwd_long(ptr(qkv), ptr(o), ptr(lse), 1, T, 1, 0.125, stream_of(qkv)) != 0
    assert lib.mi_attn_fwd(ptr(qkv), ptr(o), ptr(lse), 1, 257, 1, 0.125, stream_of(qkv)) != 0
    assert int(lib.mi_attn_max_seq()) == 256
    torch.cuda.synchronize()


def test_vit_long_sequence_matches_cpu_fp32(monkeypatch):
    """A 272² ViT (290 tokens, head dim 64) trains all-native (STRICT_NATIVE) and matches the same
    module's fp32 CPU path, with the bounds of test_vit_native_matches_cpu_fp32."""
    from mi355x_dp.models.vit import VisionTransformer
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    torch.manual_seed(0)
    m = VisionTransformer(image_size=272, patch_size=16, num_layers=2, num_heads=2, hidden_dim=128, mlp_dim=256,
                          num_classes=10)
    with torch.no_grad():  # the zero-initialised head / class token would make the check trivial
        m.heads.head.weight.normal_(std=0.2)
        m.class_token.normal_(std=0.5)
    mc = copy.deepcopy(m)
    mg = m.cuda()
    x = torch.randn(2, 3, 272, 272)
    y = torch.arange(2) % 10
    out_g = mg(x.cuda())
    out_c = mc(x)
    assert rel_err(out_g.float().cpu(), out_c) < 5e-2
    F.cross_entropy(out_g.float(), y.cuda()).backward()
    F.cross_entropy(out_c, y).backward()
    for name in ("class_token", "encoder.pos_embedding", "conv_proj.weight", "conv_proj.bias", "encoder.ln.weight",
                 "encoder.ln.bias", "heads.head.weight"):
        gg = mg.get_parameter(name).grad
        gc = mc.get_parameter(name).grad
        assert gg is not None, name
        assert rel_err(gg.float().cpu(), gc) < 8e-2, (name, rel_err(gg.float().cpu(), gc))


def test_long_attention_graph_capture(monkeypatch):
    """Forward + backward captured in a graph replays to the eager bits: no host synchronisation
    and no allocation-dependent state in the long path."""
    from mi355x_dp.ops import transformer as Tm
    monkeypatch.setenv("MI355X_DP_STRICT_NATIVE", "1")
    B, T, H = 1, 300, 1
    qkv = rnd(B * T, 3 * H * 64, scale=1.5)
    do = rnd(B * T, H * 64)

    def step(x):
        o = Tm.attention(x, B, T, H)
        (g,) = torch.autograd.grad(o, x, do)
        return o, g
    o_e, g_e = step(qkv.clone().requires_grad_())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as torch's capture recipe
        step(qkv.clone().requires_grad_())
    torch.cuda.current_stream().wait_stream(side)
    xs = qkv.clone().requires_grad_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        o_c, g_c = step(xs)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(o_c, o_e) and torch.equal(g_c, g_e)
