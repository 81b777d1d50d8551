"""The slot-ring k-loop of the TN weight-gradient kernel (``mi_set_tn_stages(2)``) against the
one-stage loop (``mi_set_tn_stages(1)``): both accumulate the same 32-row chunks in the same order,
so every result must be bit-identical, and both must agree with fp32 PyTorch.

The shapes are the smallest that reach every ring state (fewer slots than the ring is deep, a
ragged last slot, the ring wrapping several times, all four tile shapes, partial tiles, gathered
taps with padding and stride, the last-arriver epilogue, the Linear and folded-BN variants); they
are not the workload's shapes."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16


@pytest.fixture(scope="module")
def lib():
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops import kernels  # noqa: F401
    return _lib.load(True)  # fail loudly if the extension is missing


def rel_err(a, b):
    a = a.detach().float()
    b = b.detach().float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def _both(lib, run):
    """run() once with the one-stage loop and once with the ring; the selection goes back to the
    environment / default afterwards"""
    out = {}
    try:
        for stages in (1, 2):
            lib.mi_set_tn_stages(stages)
            out[stages] = run()
            torch.cuda.synchronize()
    finally:
        lib.mi_set_tn_stages(0)
    return out[1], out[2]


def _conv_inputs(shape, seed):
    N, C, H, K, R, s, p = shape
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(N, C, H, H, device="cuda", generator=g).to(BF).contiguous(memory_format=CL)
    w = (torch.randn(K, C, R, R, device="cuda", generator=g) * (2.0 / (C * R * R)) ** 0.5).to(BF).float()
    w = w.contiguous(memory_format=CL)
    P = (H + 2 * p - R) // s + 1
    gy = torch.randn(N, K, P, P, device="cuda", generator=g).to(BF).contiguous(memory_format=CL)
    return x, w, gy


def _conv_wgrad(x, w0, gy, s, p):
    """weight gradient through conv2d's backward, into a fresh (zero) gradient"""
    from mi355x_dp.ops import conv2d
    w = w0.clone().requires_grad_(True)
    conv2d(x, w, None, s, p).backward(gy)
    return w.grad.float().clone()


def _conv_ref(x, w0, gy, s, p):
    wr = w0.clone().requires_grad_(True)
    F.conv2d(x.float(), wr, None, s, p).backward(gy.float())
    return wr.grad


CONV_SHAPES = [
    # N, C, H, K, R, stride, pad                reduction rows N*P*Q
    (1, 64, 5, 64, 1, 1, 0),     # 25: less than one slot
    (1, 64, 8, 64, 1, 1, 0),     # 64: two slots
    (2, 64, 7, 64, 1, 1, 0),     # 98: four slots, the last one ragged
    (8, 64, 28, 64, 1, 1, 0),    # 64x64 tile, split K
    (8, 64, 28, 256, 1, 1, 0),   # 128x64
    (8, 256, 28, 64, 1, 1, 0),   # 64x128
    (8, 128, 28, 128, 1, 1, 0),  # 128x128
    (3, 64, 17, 64, 3, 1, 1),    # gathered taps, rows crossing image boundaries
    (4, 128, 14, 128, 3, 2, 1),  # stride 2 with padding
    (4, 96, 14, 160, 1, 1, 0),   # M and N no multiples of the tile (C % 64 != 0: the im2col route, plain TN GEMM)
    (32, 512, 7, 512, 3, 1, 1),  # 144 tiles x 5 splits of 5 k-steps: the ring wraps (10 slots per split)
]


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_wgrad_ring_bit_identical(lib, shape):
    N, C, H, K, R, s, p = shape
    x, w0, gy = _conv_inputs(shape, 11)
    one, ring = _both(lib, lambda: _conv_wgrad(x, w0, gy, s, p))
    assert torch.equal(one, ring)
    err = rel_err(ring, _conv_ref(x, w0, gy, s, p))
    assert err < 1e-2, err


def test_conv_wgrad_gather_partial_tiles(lib):
    """the gathering (conv) instance itself with M and N no multiples of the tile: C = 96 reaches it
    only through the C ABI (conv2d sends C % 64 != 0 to im2col)"""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    shape = (4, 96, 14, 160, 3, 1, 1)
    N, C, H, K, R, s, p = shape
    x, w0, gy = _conv_inputs(shape, 12)

    def run():
        dw = torch.zeros(K, R, R, C, device="cuda")
        _lib.call("mi_conv2d_wgrad", ptr(x), ptr(gy), ptr(dw), N, H, H, C, K, R, R, s, p, H, H, stream_of(x))
        return dw

    one, ring = _both(lib, run)
    assert torch.equal(one, ring)
    err = rel_err(ring.permute(0, 3, 1, 2), _conv_ref(x, w0, gy, s, p))
    assert err < 1e-2, err


@pytest.mark.parametrize("shape", [
    (8, 128, 28, 128, 1, 1, 0),  # 98 splits: the reduce launch either way
    (32, 512, 7, 512, 3, 1, 1),  # 5 splits: the last-arriving split sums the slabs in the launch
])
def test_ring_last_arriver_epilogue(lib, shape):
    """the fused split-K reduction (fewer than 8 splits: the last arriver) with the ring, equal to
    the separate reduce launch and to the one-stage loop"""
    N, C, H, K, R, s, p = shape
    x, w0, gy = _conv_inputs(shape, 13)
    out = {}
    try:
        for fused in (0, 1, 1):
            lib.mi_set_tn_split_fused(fused)
            out.setdefault(fused, []).append(_both(lib, lambda: _conv_wgrad(x, w0, gy, s, p)))
    finally:
        lib.mi_set_tn_split_fused(0)
    (one0, ring0), (one1, ring1), (_, ring1b) = out[0][0], out[1][0], out[1][1]
    assert torch.equal(one0, ring0) and torch.equal(one1, ring1)
    assert torch.equal(ring1, ring0)   # last arriver == separate reduce
    assert torch.equal(ring1, ring1b)  # the arrival counters were left zeroed
    err = rel_err(ring1, _conv_ref(x, w0, gy, s, p))
    assert err < 1e-2, err


@pytest.mark.parametrize("T,N,K", [(200, 192, 320), (4096, 768, 768)])
@pytest.mark.parametrize("fused", [0, 1])
def test_linear_wgrad_bias_ring(lib, T, N, K, fused):
    """Linear weight + bias gradient (mi_gemm_tn_bias, the column-sum variant).  The weight gradient
    goes through the slabs and is bit-identical; the bias column sums of the splits are added with
    fp32 atomics in arrival order, with either loop, so they are held to the fp32 reference only
    (as in test_tn_bias_splitk_slabs)."""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    g = torch.Generator(device="cuda").manual_seed(7)
    dy = (torch.rand(T, N, device="cuda", generator=g) * 2 - 1).to(BF)
    x = (torch.rand(T, K, device="cuda", generator=g) * 2 - 1).to(BF)
    gw0 = torch.randn(N, K, device="cuda", generator=g)
    gb0 = torch.randn(N, device="cuda", generator=g)
    ref_w = gw0 + dy.float().t() @ x.float()
    ref_b = gb0 + dy.float().sum(0)

    def run():
        gw, gb = gw0.clone(), gb0.clone()
        _lib.call("mi_gemm_tn_bias", ptr(dy), ptr(x), ptr(gw), ptr(gb), N, K, T, N, K, K, stream_of(dy))
        return gw, gb

    try:
        lib.mi_set_tn_split_fused(fused)
        (gw1, gb1), (gw2, gb2) = _both(lib, run)
    finally:
        lib.mi_set_tn_split_fused(0)
    assert torch.equal(gw1, gw2)
    for gw, gb in ((gw1, gb1), (gw2, gb2)):
        assert rel_err(gw, ref_w) < 1e-4, rel_err(gw, ref_w)
        assert rel_err(gb, ref_b) < 1e-4, rel_err(gb, ref_b)


def test_linear_wgrad_plain_ring(lib):
    """mi_gemm_tn without the bias column sums, partial tiles in M and N"""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    T, N, K = 200, 192, 320
    g = torch.Generator(device="cuda").manual_seed(8)
    dy = (torch.rand(T, N, device="cuda", generator=g) * 2 - 1).to(BF)
    x = (torch.rand(T, K, device="cuda", generator=g) * 2 - 1).to(BF)

    def run():
        gw = torch.zeros(N, K, device="cuda")
        _lib.call("mi_gemm_tn", ptr(dy), ptr(x), ptr(gw), N, K, T, N, K, K, stream_of(dy))
        return gw

    one, ring = _both(lib, run)
    assert torch.equal(one, ring)
    assert rel_err(ring, dy.float().t() @ x.float()) < 1e-4


@pytest.mark.parametrize("shape", [(2, 13, 64, 64), (4, 28, 512, 128)])  # N, H, C, K: 64x64 and 128x128 tiles
def test_wgrad_fbb_ring(lib, shape):
    """folded BN backward weight gradient (two-source A, the input's column sums per split): ring
    against one-stage, and test_panel_gpu.py::test_wgrad_fbb's fp32 check"""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    N, H, C, K = shape
    g = torch.Generator(device="cuda").manual_seed(9)
    dz = torch.randn(N, K, H, H, device="cuda", generator=g).to(BF).contiguous(memory_format=CL)
    coef = torch.stack([torch.rand(K, device="cuda", generator=g) + 0.5,
                        torch.randn(K, device="cuda", generator=g) * 0.1,
                        torch.randn(K, device="cuda", generator=g) * 0.1]).contiguous()
    w = (torch.randn(K, C, 1, 1, device="cuda", generator=g) * (1.0 / K) ** 0.5).to(BF).contiguous(memory_format=CL)
    x = torch.relu(torch.randn(N, C, H, H, device="cuda", generator=g)).to(BF).contiguous(memory_format=CL)
    c = F.conv2d(x.float(), w.float()).to(BF)  # the forward conv's stored output
    dX = dz.float() * coef[0].view(1, K, 1, 1) + c.float() * coef[1].view(1, K, 1, 1) + coef[2].view(1, K, 1, 1)
    ref = torch.nn.grad.conv2d_weight(x.float(), (K, C, 1, 1), dX, 1, 0).permute(0, 2, 3, 1).contiguous()
    dw0 = torch.randn(K, 1, 1, C, device="cuda", generator=g)
    ws = torch.zeros(lib.mi_conv2d_wgrad_fbb_ws_floats(K, C), device="cuda")

    def run():
        dw = dw0.clone()
        _lib.call("mi_conv2d_wgrad_fbb", ptr(x), ptr(dz), ptr(w), ptr(coef), ptr(dw), ptr(ws), N, H, H, C, K,
                  stream_of(dz))
        torch.cuda.synchronize()
        assert float(ws[:(K + C) * C].abs().max()) == 0.0  # T and G re-zeroed
        return dw

    one, ring = _both(lib, run)
    assert torch.equal(one, ring)
    err = rel_err(ring - dw0, ref)
    assert err < 1e-2, err


def test_nol_wgrad_keeps_one_stage_loop(lib):
    """normalize-on-load rewrites its LDS tile in place and has no ring variant: with the ring
    selected it still runs (the one-stage loop) and gives the same bits"""
    from mi355x_dp.ops import _lib
    from mi355x_dp.ops._lib import ptr, stream_of
    N, C, H, K, R, s, p = 16, 64, 32, 64, 3, 1, 1
    g = torch.Generator(device="cuda").manual_seed(3)
    c = torch.randn(N, C, H, H, device="cuda", generator=g).to(BF).contiguous(memory_format=CL)
    scale = torch.rand(C, device="cuda", generator=g) + 0.5
    shift = torch.randn(C, device="cuda", generator=g) * 0.5
    y = torch.relu(c.float() * scale.view(1, C, 1, 1) + shift.view(1, C, 1, 1)).to(BF).contiguous(memory_format=CL)
    dy = torch.randn(N, K, H, H, device="cuda", generator=g).to(BF).contiguous(memory_format=CL)

    def run():
        dw = torch.zeros(K, R, R, C, device="cuda")
        rc = lib.mi_conv2d_wgrad_nol(ptr(c), ptr(dy), ptr(dw), ptr(scale), ptr(shift), N, H, H, C, K, R, R, s, p,
                                     H, H, stream_of(c))
        assert rc == 0, rc
        return dw

    one, ring = _both(lib, run)
    assert torch.equal(one, ring)
    dw_ref = torch.zeros(K, R, R, C, device="cuda")
    _lib.call("mi_conv2d_wgrad", ptr(y), ptr(dy), ptr(dw_ref), N, H, H, C, K, R, R, s, p, H, H, stream_of(c))
    torch.cuda.synchronize()
    assert rel_err(ring, dw_ref) < 1e-2
