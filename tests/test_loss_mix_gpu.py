"""Soft-target cross entropy (loss.hip) and the fused augmentation + Mixup / CutMix pass (mix.hip) on
the GPU.  The loss reference is ``F.cross_entropy`` in fp64 on the dense target; the mixing
reference is ``augment`` itself (same seed => same per-image crop / flip)."""
import pytest
import torch
import torch.nn.functional as F

from mi355x_dp.data.mix import BatchMixer, MixParams
from mi355x_dp.ops import MixedTarget, augment, augment_mix, cross_entropy

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16
MEAN, STD = (0.4914, 0.4822, 0.4465), (0.2023, 0.1994, 0.2010)


@pytest.fixture(scope="module", autouse=True)
def _native():
    from mi355x_dp.ops import _lib
    _lib.load(True)  # fail loudly if the extension is missing
    torch.manual_seed(0)


def rel_err(a, b):
    a = a.detach().float()
    b = b.detach().float()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-6))


def rel_l2(a, b):
    a = a.detach().float()
    b = b.detach().float()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


# ------------------------------------------------------------------------------------- loss
SHAPES = [(3, 10), (5, 1000), (2, 257)]  # fewer classes than threads, strided loop, its tail


def _logits(N, C, dtype):
    g = torch.Generator(device="cuda").manual_seed(N * 10007 + C)
    return (torch.randn(N, C, device="cuda", generator=g) * 3).to(dtype)


def _pair(N, C):
    g = torch.Generator(device="cuda").manual_seed(N + C)
    ya = torch.randint(0, C, (N,), device="cuda", generator=g)
    yb = (ya + 1 + torch.randint(0, C - 1, (N,), device="cuda", generator=g)) % C  # != ya
    yb[N - 1] = ya[N - 1]
    lam = torch.tensor([0.0, 1.0, 0.3, 0.6, 0.45][:N], device="cuda")
    return ya, yb, lam


def _dense64(ya, yb, lam, C):
    lam = lam.double().unsqueeze(1)
    return lam * F.one_hot(ya, C).double() + (1 - lam) * F.one_hot(yb, C).double()


def _check_loss(lg, target, dense64, eps):
    """loss within 1e-4 relative and gradient rel_err < 1e-2 of the fp64 reference (the tolerances of
    test_cross_entropy); the gradient comes back in the logits' dtype."""
    a = lg.clone().requires_grad_()
    loss = cross_entropy(a, target, label_smoothing=eps)
    (loss * 2).backward()
    r = lg.double().requires_grad_()
    ref = F.cross_entropy(r, dense64, label_smoothing=eps)
    (ref * 2).backward()
    ref = float(ref.detach())
    err_l, err_g = abs(float(loss.detach()) - ref), rel_err(a.grad, r.grad)
    print(f"loss {float(loss.detach()):.7f} ref {ref:.7f} |d| {err_l:.2e} grad rel_err {err_g:.2e}")
    assert loss.dtype == torch.float32 and a.grad.dtype == lg.dtype
    assert err_l < 1e-4 * max(1.0, abs(ref))
    assert err_g < 1e-2


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,C", SHAPES)
def test_pair_target(N, C, eps, dtype):
    ya, yb, lam = _pair(N, C)
    _check_loss(_logits(N, C, dtype), MixedTarget(ya, yb, lam), _dense64(ya, yb, lam, C), eps)


@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,C", SHAPES)
def test_hard_labels_with_smoothing(N, C, dtype):
    ya, _, _ = _pair(N, C)
    _check_loss(_logits(N, C, dtype), ya, F.one_hot(ya, C).double(), 0.1)


@pytest.mark.parametrize("tdtype", [torch.float32, BF], ids=["t_fp32", "t_bf16"])
@pytest.mark.parametrize("dtype", [torch.float32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("N,C", SHAPES)
def test_dense_target(N, C, eps, dtype, tdtype):
    g = torch.Generator(device="cuda").manual_seed(C)
    t = torch.softmax(torch.randn(N, C, device="cuda", generator=g) * 2, 1)
    t[0] *= 0.5   # rows need not sum to one
    t[N - 1] *= 1.75
    t = t.to(tdtype)
    _check_loss(_logits(N, C, dtype), t, t.double(), eps)


def test_default_path_unchanged():
    """No smoothing on hard labels is today's kernel pair: same bits with and without the argument."""
    lg, (y, _, _) = _logits(5, 1000, torch.float32), _pair(5, 1000)
    a, b = lg.clone().requires_grad_(), lg.clone().requires_grad_()
    la, lb = cross_entropy(a, y), cross_entropy(b, y, label_smoothing=0.0)
    la.backward()
    lb.backward()
    assert torch.equal(la, lb) and torch.equal(a.grad, b.grad)
    assert la.grad_fn.name().startswith("_CrossEntropyBackward")


def _run_pair(lg, tgt, eps):
    a = lg.clone().requires_grad_()
    loss = cross_entropy(a, tgt, label_smoothing=eps)
    (g,) = torch.autograd.grad(loss, a)
    return loss.detach(), g


def test_repeatable():
    ya, yb, lam = _pair(5, 1000)
    lg = _logits(5, 1000, torch.float32)
    for tgt in (MixedTarget(ya, yb, lam), ya, _dense64(ya, yb, lam, 1000).float()):
        l1, g1 = _run_pair(lg, tgt, 0.1)
        l2, g2 = _run_pair(lg, tgt, 0.1)
        assert torch.equal(l1, l2) and torch.equal(g1, g2)


def test_graph_replay_sees_new_targets():
    """Forward + backward captured over a static MixedTarget: overwriting y_a / y_b / lam between
    replays changes the result, and each replay equals the eager run on those values bit for bit."""
    N, C = 5, 1000
    lg = _logits(N, C, torch.float32)
    ya, yb, lam = _pair(N, C)
    ya2, yb2, lam2 = yb.clone(), (ya + 7) % C, torch.tensor([0.9, 0.2, 1.0, 0.0, 0.5], device="cuda")
    eager = [_run_pair(lg, MixedTarget(*t), 0.1) for t in ((ya, yb, lam), (ya2, yb2, lam2))]
    assert not torch.equal(eager[0][0], eager[1][0])
    static = MixedTarget(ya.clone(), yb.clone(), lam.clone())
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up on the side stream, as torch's capture recipe
        _run_pair(lg, static, 0.1)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        l_c, g_c = _run_pair(lg, static, 0.1)
    for (t, (l_e, g_e)) in zip(((ya, yb, lam), (ya2, yb2, lam2)), eager):
        for dst, src in zip(static, t):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(l_c, l_e) and torch.equal(g_c, g_e)


# ------------------------------------------------------------------------------------- mixing
N_, H_, W_, PAD, SEED = 5, 9, 11, 2, 17


@pytest.fixture(scope="module")
def batch():
    """One uint8 batch and what ``augment`` makes of it at 3 and 8 output channels (computed once)."""
    g = torch.Generator(device="cuda").manual_seed(1)
    u8 = torch.randint(0, 256, (N_, H_, W_, 3), dtype=torch.uint8, device="cuda", generator=g)
    labels = torch.tensor([3, 1, 4, 1, 5], device="cuda")
    ref = {c: augment(u8, c, MEAN, STD, pad=PAD, flip=True, seed=SEED) for c in (3, 8)}
    return u8, labels, ref


def _params(partner, lam, box):
    return MixParams(torch.tensor(partner, dtype=torch.int32, device="cuda"),
                     torch.tensor(lam, dtype=torch.float32, device="cuda"),
                     torch.tensor(box, dtype=torch.int32, device="cuda").view(-1, 4))


def _mix(batch, cout, params, **kw):
    u8, labels, _ = batch
    return augment_mix(u8, labels, cout, MEAN, STD, params, pad=PAD, flip=True, seed=SEED, **kw)


PARTNER = [4, 0, 1, 2, 3]
BOXES = [[2, 5, 3, 7],      # interior
         [0, 4, 0, 11],     # touching three borders
         [0, 9, 0, 11],     # the full image
         [5, 9, 8, 11],     # the bottom-right corner
         [-3, 4, 6, 20]]    # reaching past the image: clipped to rows 0..4, columns 6..11
CLIPPED = [[2, 5, 3, 7], [0, 4, 0, 11], [0, 9, 0, 11], [5, 9, 8, 11], [0, 4, 6, 11]]
MIX_LAM = [0.3, 0.0, 1.0, 0.5, 0.9]
EMPTY = [[0, 0, 0, 0], [3, 3, 2, 8], [0, 0, 0, 0], [4, 9, 5, 5], [0, 0, 0, 0]]  # zero-area boxes are Mixup


@pytest.mark.parametrize("cout", [3, 8])
def test_mix_identity_equals_augment(batch, cout):
    x, t = _mix(batch, cout, _params(PARTNER, [1.0] * N_, [[0, 0, 0, 0]] * N_))
    assert x.dtype == BF and x.shape == (N_, cout, H_, W_) and x.is_contiguous(memory_format=CL)
    assert torch.equal(x, batch[2][cout])
    assert torch.equal(t.lam, torch.ones(N_, device="cuda"))


@pytest.mark.parametrize("cout", [3, 8])
def test_cutmix_pastes_the_partner_exactly(batch, cout):
    ref = batch[2][cout]
    x, _ = _mix(batch, cout, _params(PARTNER, [0.5] * N_, BOXES))
    for n, (y0, y1, x0, x1) in enumerate(CLIPPED):
        inside = torch.zeros(H_, W_, dtype=torch.bool, device="cuda")
        inside[y0:y1, x0:x1] = True
        want = torch.where(inside, ref[PARTNER[n]], ref[n])
        assert torch.equal(x[n], want), n
        assert not torch.equal(ref[PARTNER[n]], ref[n])  # the comparison can tell them apart


@pytest.mark.parametrize("cout", [3, 8])
def test_mixup_blends_in_fp32(batch, cout):
    """|out - ref| <= 2^-7 max(|a'|, |b'|) + 1e-6: the reference's inputs a', b' are augment's bf16
    outputs and the kernel's output is rounded to bf16 once, each at most 2^-8 relative."""
    ref = batch[2][cout].float()
    x, _ = _mix(batch, cout, _params(PARTNER, MIX_LAM, EMPTY))
    a, b = ref, ref[torch.tensor(PARTNER, device="cuda")]
    lam = torch.tensor(MIX_LAM, device="cuda").view(N_, 1, 1, 1)
    want = lam * a + (1 - lam) * b
    bound = 2.0 ** -7 * torch.maximum(a.abs(), b.abs()) + 1e-6
    excess = ((x.float() - want).abs() - bound).max()
    print(f"mixup cout={cout}: max |out - ref| {float((x.float() - want).abs().max()):.3e}, max excess {float(excess):.3e}")
    assert excess <= 0
    assert torch.equal(x[1].float(), b[1]) and torch.equal(x[2].float(), a[2])  # lam 0 / 1: one source, exact


def test_emitted_targets(batch):
    _, labels, _ = batch
    want_b = labels[torch.tensor(PARTNER, device="cuda")]
    _, t = _mix(batch, 8, _params(PARTNER, [0.5] * N_, BOXES))
    area = torch.tensor([(y1 - y0) * (x1 - x0) for y0, y1, x0, x1 in CLIPPED], dtype=torch.float32)
    want_lam = (1.0 - area / float(H_ * W_)).cuda()  # the host formula, in fp32
    assert t.y_a.dtype == torch.int64 and t.y_b.dtype == torch.int64 and t.lam.dtype == torch.float32
    assert torch.equal(t.y_a, labels) and torch.equal(t.y_b, want_b) and torch.equal(t.lam, want_lam)
    _, t = _mix(batch, 8, _params(PARTNER, MIX_LAM, EMPTY))
    assert torch.equal(t.y_a, labels) and torch.equal(t.y_b, want_b)
    assert torch.equal(t.lam, torch.tensor(MIX_LAM, device="cuda"))


def test_batch_mixer_feeds_the_kernel(batch):
    """BatchMixer's device tensors are what augment_mix takes, and the emitted lam is the mixer's."""
    m = BatchMixer(per_sample=True, seed=2, device="cuda")
    host = m.host_params(3, N_, H_, W_)
    p = m.params(3, N_, H_, W_)
    _, t = _mix(batch, 8, p)
    assert p.partner.tolist() == host[0].tolist() and p.box.tolist() == host[2].tolist()
    assert torch.equal(t.lam.cpu(), torch.from_numpy(host[1]))
    assert torch.equal(t.y_b, batch[1][p.partner.long()])


def test_static_buffers_are_written_in_place(batch):
    p = _params(PARTNER, MIX_LAM, BOXES[:2] + EMPTY[2:])
    x, t = _mix(batch, 8, p)
    out = torch.zeros((N_, 8, H_, W_), dtype=BF, device="cuda").contiguous(memory_format=CL)
    tgt = MixedTarget(torch.zeros(N_, dtype=torch.int64, device="cuda"), torch.zeros(N_, dtype=torch.int64, device="cuda"),
                      torch.zeros(N_, device="cuda"))
    ptrs = [out.data_ptr()] + [v.data_ptr() for v in tgt]
    x2, t2 = _mix(batch, 8, p, out=out, target=tgt)
    assert [x2.data_ptr()] + [v.data_ptr() for v in t2] == ptrs
    assert torch.equal(out, x) and all(torch.equal(u, v) for u, v in zip(tgt, t))


# ------------------------------------------------------------------------------ one step end to end
def test_resnet18_mixed_step_matches_fp32():
    """ResNet-18, batch 8 at 64x64: augment_mix + smoothed pair loss on the native path vs the fp32
    stock model on the same mixed input with the dense target; the rule of
    test_resnet18_train_step_matches_fp32 (every gradient within 1.5x (+0.02) of stock bf16's error)."""
    from mi355x_dp.models import resnet18
    from mi355x_dp.models.stock import stock_resnet
    torch.manual_seed(0)
    m = resnet18(num_classes=10).cuda()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    u8 = torch.randint(0, 256, (8, 64, 64, 3), dtype=torch.uint8, device="cuda")
    y = torch.randint(0, 10, (8,), device="cuda")
    p = BatchMixer(per_sample=True, seed=0, device="cuda").params(0, 8, 64, 64)
    xb, tgt = augment_mix(u8, y, 3, MEAN, STD, p, pad=4, flip=True, seed=5)
    x = xb.float().contiguous()  # the same (bf16-exact) mixed input for all three models
    dense = tgt.dense(10)
    assert 0 < int((tgt.lam < 1).sum())  # the batch really is mixed
    loss = cross_entropy(m(x), tgt, label_smoothing=0.1)
    loss.backward()
    ref = stock_resnet("resnet18", 10).cuda()
    ref.load_state_dict(sd)
    loss_r = F.cross_entropy(ref(x), dense, label_smoothing=0.1)
    loss_r.backward()
    st = stock_resnet("resnet18", 10).cuda().to(BF).to(memory_format=CL)
    st.load_state_dict(sd)
    F.cross_entropy(st(x.to(BF).contiguous(memory_format=CL)).float(), dense, label_smoothing=0.1).backward()
    assert abs(float(loss.detach()) - float(loss_r.detach())) < 0.05 * max(1.0, abs(float(loss_r.detach())))
    pn, pr, ps = dict(m.named_parameters()), dict(ref.named_parameters()), dict(st.named_parameters())
    for n in pr:
        e_native = rel_l2(pn[n].grad, pr[n].grad)
        e_stock = rel_l2(ps[n].grad, pr[n].grad)
        assert e_native <= 1.5 * e_stock + 0.02, (n, e_native, e_stock)
