"""Segmentation head kernels (ops/csrc/segloss.hip) against float64 CPU
references computed from the same, already dtype-rounded, inputs.

Tolerances are the project's own for fused losses (test_lsnll_*):
loss rtol=1e-5/atol=1e-6, fp32 gradients rtol=1e-4/atol=1e-6, bf16/fp16
gradients rtol=1e-2/atol=1e-3 against the float64 gradient cast to that
dtype, counts and matrices exact. Gradients are taken of loss * numel so
their entries are O(1) and atol decides nothing."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.metrics import ConfusionMatrix, Prf1a

LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = {torch.float32: dict(rtol=1e-4, atol=1e-6),
            torch.bfloat16: dict(rtol=1e-2, atol=1e-3),
            torch.float16: dict(rtol=1e-2, atol=1e-3)}

# The launcher caps the grid at 2048 blocks of 256 threads, one 16-byte
# vector per thread per sweep: 2048 * 256 * 8 = 4 194 304 bf16/fp16 voxels
# (2 097 152 in fp32). 136*136*240 = 4 439 040 exceeds both, so the
# grid-stride loop wraps.
BIG = (1, 1, 136, 136, 240)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _labels(shape, kind, gen):
    if kind == 'soft':
        return torch.rand(shape, generator=gen)
    t = torch.rand(shape, generator=gen) > 0.6
    return t.to({'uint8': torch.uint8, 'bool': torch.bool,
                 'int64': torch.int64}[kind])


def _dice_ref(x, t, w, beta, eps=1e-5):
    """float64 loss and d(loss * numel)/dx on the CPU."""
    x64 = x.detach().double().cpu().reshape(-1).requires_grad_(True)
    t64 = t.detach().double().cpu().reshape(-1)
    p = torch.sigmoid(x64)
    if w is not None:
        w64 = w.detach().double().cpu().reshape(-1)
        p, t64 = p * w64, t64 * w64
    b2 = beta * beta
    num = (1 + b2) * (p * t64).sum() + eps
    den = b2 * t64.sum() + p.sum() + eps
    loss = 1.0 - num / den
    (loss * x64.numel()).backward()
    return loss.detach(), x64.grad.reshape(x.shape)


def _check_dice(x, t, w, beta, dev):
    """x: leaf logits on the device; t, w on the device."""
    ref_loss, ref_grad = _dice_ref(x, t, w, beta)
    x.grad = None
    loss = ops.dice_loss_with_logits(x, t, beta=beta, weights=w)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * x.numel()).backward()
    print(f'dice n={x.numel()} {x.dtype} {t.dtype} w={w is not None} '
          f'beta={beta}: loss={loss.item():.9g} ref={ref_loss.item():.9g}')
    torch.testing.assert_close(loss.double().cpu(), ref_loss, **LOSS_TOL)
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    torch.testing.assert_close(x.grad.cpu(), ref_grad.to(x.dtype),
                               **GRAD_TOL[x.dtype])


def _make_logits(shape, dtype, dev, gen, misaligned=False):
    n = 1
    for s in shape:
        n *= s
    if misaligned:
        # buf[1:] starts one element (2 or 4 bytes) past a 16-byte boundary
        buf = (2.0 * torch.randn(n + 1, generator=gen)).to(dtype).to(dev)
        x = buf[1:].view(shape).detach()
        assert x.data_ptr() % 16 != 0
    else:
        x = (2.0 * torch.randn(shape, generator=gen)).to(dtype).to(dev)
    return x.requires_grad_(True)


DICE_SHAPES = [((1,), False), ((7,), False), ((2, 1, 9, 11, 13), False),
               ((2, 1, 16, 16, 16), False), ((2, 1, 8, 8, 8), True)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16,
                                   torch.float32])
@pytest.mark.parametrize('shape,misaligned', DICE_SHAPES)
def test_dice_forward_backward(dev, shape, misaligned, dtype):
    gen = torch.Generator().manual_seed(11)
    x = _make_logits(shape, dtype, dev, gen, misaligned)
    w = (0.5 + torch.rand(shape, generator=gen)).to(dev)
    for kind in ('uint8', 'bool', 'int64', 'soft'):
        t = _labels(shape, kind, gen).to(dev)
        for weights in (None, w):
            for beta in (1.0, 2.0):
                _check_dice(x, t, weights, beta, dev)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16,
                                   torch.float32])
def test_dice_grid_stride_wraps(dev, dtype):
    gen = torch.Generator().manual_seed(12)
    x = _make_logits(BIG, dtype, dev, gen)
    w = (0.5 + torch.rand(BIG, generator=gen)).to(dev)
    for kind, weights, beta in (('uint8', None, 1.0), ('bool', w, 2.0),
                                ('int64', w, 1.0), ('soft', None, 2.0)):
        t = _labels(BIG, kind, gen).to(dev)
        _check_dice(x, t, weights, beta, dev)


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16,
                                   torch.float32])
@pytest.mark.parametrize('value,mask', [(-100.0, 0), (100.0, 1)])
def test_dice_saturated_logits(dev, dtype, value, mask):
    shape = (2, 1, 9, 11, 13)
    x = torch.full(shape, value, dtype=dtype, device=dev, requires_grad=True)
    t = torch.full(shape, mask, dtype=torch.uint8, device=dev)
    loss = ops.dice_loss_with_logits(x, t)
    (loss * x.numel()).backward()
    assert torch.isfinite(loss).item()
    assert torch.isfinite(x.grad.float()).all().item()
    assert x.grad.float().abs().max().item() < 1e-6
    ref_loss, ref_grad = _dice_ref(x, t, None, 1.0)
    torch.testing.assert_close(loss.double().cpu(), ref_loss, **LOSS_TOL)
    torch.testing.assert_close(x.grad.cpu(), ref_grad.to(dtype),
                               **GRAD_TOL[dtype])


def test_dice_reproducible(dev):
    gen = torch.Generator().manual_seed(13)
    x = _make_logits(BIG, torch.bfloat16, dev, gen)
    t = _labels(BIG, 'uint8', gen).to(dev)
    w = (0.5 + torch.rand(BIG, generator=gen)).to(dev)
    runs = []
    for _ in range(2):
        x.grad = None
        loss = ops.dice_loss_with_logits(x, t, beta=2.0, weights=w)
        (loss * x.numel()).backward()
        runs.append((loss.detach().clone(), x.grad.clone()))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])


# ---- voxelwise cross-entropy -------------------------------------------------
CE_CASES = [(2, 2, (4, 4, 4)),
            (2, 3, (5, 6, 7)),      # S = 210, no multiple of 8: scalar path
            (1, 4, (9, 11, 13)),    # odd S
            (2, 5, (8, 8, 8)),      # vector path
            (1, 1, (4, 4, 4)),      # C = 1: loss and gradient are 0
            (2, 4, (64, 64, 64))]   # multi-block


def _class_labels(N, C, spatial, gen, dtype=torch.int64):
    y = torch.randint(0, C, (N, *spatial), generator=gen)
    y.view(-1)[0] = C - 1
    y.view(-1)[-1] = C - 1
    return y.to(dtype)


@pytest.mark.parametrize('label_dtype', [torch.int64, torch.uint8])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('N,C,spatial', CE_CASES)
def test_voxel_cross_entropy(dev, N, C, spatial, dtype, label_dtype):
    gen = torch.Generator().manual_seed(21)
    x = _make_logits((N, C, *spatial), dtype, dev, gen)
    y = _class_labels(N, C, spatial, gen, label_dtype)
    assert int(y.max()) == C - 1
    x64 = x.detach().double().cpu().requires_grad_(True)
    ref = F.cross_entropy(x64, y.long())
    nvox = y.numel()
    (ref * nvox).backward()

    loss = ops.cross_entropy(x, y.to(dev))
    (loss * nvox).backward()
    print(f'ce {N}x{C}x{spatial} {dtype}: loss={loss.item():.9g} '
          f'ref={ref.item():.9g}')
    assert loss.dtype == torch.float32 and loss.dim() == 0
    torch.testing.assert_close(loss.double().cpu(), ref.detach(), **LOSS_TOL)
    assert x.grad.dtype == dtype and x.grad.shape == x.shape
    torch.testing.assert_close(x.grad.cpu(), x64.grad.to(dtype),
                               **GRAD_TOL[dtype])
    if C == 1:
        assert loss.item() == 0.0
        assert x.grad.float().abs().max().item() == 0.0


def test_cross_entropy_2d_unchanged(dev):
    """The classifier-head path: same assertions as
    test_gpu_kernels.py::test_lsnll_forward_backward."""
    torch.manual_seed(3)
    for B, Cc in [(32, 2), (128, 10), (7, 33)]:
        logits = torch.randn(B, Cc, device=dev, requires_grad=True)
        target = torch.randint(0, Cc, (B,), device=dev)
        loss = ops.cross_entropy(logits, target)
        ref_logits = logits.detach().clone().requires_grad_(True)
        ref = torch.nn.functional.cross_entropy(ref_logits, target)
        torch.testing.assert_close(loss, ref, rtol=1e-5, atol=1e-6)
        loss.backward()
        ref.backward()
        torch.testing.assert_close(logits.grad, ref_logits.grad,
                                   rtol=1e-4, atol=1e-6)


# ---- counts and confusion from logits ---------------------------------------
def _case_counts(pred, true):
    cases = true.long().reshape(-1) * 2 + pred.long().reshape(-1)
    return tuple(int((cases == c).sum()) for c in (3, 1, 0, 2))


@pytest.mark.parametrize('label_dtype', [torch.uint8, torch.int64])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('shape', [(10001,), (2, 1, 9, 11, 13)])
def test_counts_from_logits(dev, shape, dtype, label_dtype):
    gen = torch.Generator().manual_seed(31)
    x = torch.randn(shape, generator=gen).to(dtype)
    flat = x.view(-1)
    flat[0::17] = 0.0      # exact zeros of both signs: both negative
    flat[5::17] = -0.0
    y = (torch.rand(shape, generator=gen) > 0.5).to(label_dtype)
    ref = _case_counts(x > 0, y)
    assert ops.seg_prf1a_counts(x.to(dev), y.to(dev)) == ref
    assert sum(ref) == x.numel()


def _argmax_lowest(x):
    K = x.shape[1]
    idx = torch.arange(K).view(1, K, *([1] * (x.dim() - 2)))
    return torch.where(x == x.amax(1, keepdim=True), idx, K).amin(1)


def _confusion_ref(x, y, K):
    pred = _argmax_lowest(x.float()).reshape(-1)
    binc = torch.bincount(y.long().reshape(-1) * K + pred, minlength=K * K)
    return binc.reshape(K, K)


@pytest.mark.parametrize('K', [2, 4, 7])
@pytest.mark.parametrize('N,spatial', [(2, (5, 6, 7)), (1, (64, 64, 64))])
def test_confusion_from_logits(dev, N, spatial, K):
    gen = torch.Generator().manual_seed(41)
    x = torch.randn(N, K, *spatial, generator=gen).to(torch.bfloat16)
    label_dtype = torch.uint8 if K == 4 else torch.int64
    y = _class_labels(N, K, spatial, gen, label_dtype)
    ref = _confusion_ref(x, y, K)
    got = ops.seg_confusion_matrix(x.to(dev), y.to(dev), K)
    assert got.dtype == torch.int64 and got.shape == (K, K)
    assert torch.equal(got.cpu(), ref)
    assert int(ref.sum()) == y.numel()


@pytest.mark.parametrize('spatial', [(5, 6, 7), (8, 8, 8)])
def test_confusion_all_equal_logits_go_to_class_0(dev, spatial):
    K = 4
    gen = torch.Generator().manual_seed(42)
    x = torch.full((2, K, *spatial), 0.75, dtype=torch.bfloat16)
    y = _class_labels(2, K, spatial, gen)
    got = ops.seg_confusion_matrix(x.to(dev), y.to(dev), K).cpu()
    assert int(got[:, 1:].sum()) == 0
    assert torch.equal(got[:, 0], torch.bincount(y.reshape(-1), minlength=K))


def test_metrics_add_logits_match_add(dev):
    gen = torch.Generator().manual_seed(51)
    # binary, same shape
    x = torch.randn(2, 1, 9, 11, 13, generator=gen).to(torch.bfloat16)
    y = (torch.rand(2, 1, 9, 11, 13, generator=gen) > 0.5).to(torch.uint8)
    a, b = Prf1a(), Prf1a()
    a.add_logits(x.to(dev), y.to(dev))
    b.add((x > 0).long(), y.long())
    assert (a.tp, a.fp, a.tn, a.fn) == (b.tp, b.fp, b.tn, b.fn)
    # two-plane logits: argmax rule through the 2x2 matrix
    x2 = torch.randn(2, 2, 5, 6, 7, generator=gen).to(torch.bfloat16)
    y2 = _class_labels(2, 2, (5, 6, 7), gen)
    a, b = Prf1a(), Prf1a()
    a.add_logits(x2.to(dev), y2.to(dev))
    b.add(_argmax_lowest(x2.float()), y2)
    assert (a.tp, a.fp, a.tn, a.fn) == (b.tp, b.fp, b.tn, b.fn)
    # K classes
    x4 = torch.randn(2, 4, 8, 8, 8, generator=gen).to(torch.bfloat16)
    y4 = _class_labels(2, 4, (8, 8, 8), gen)
    a, b = ConfusionMatrix(num_classes=4), ConfusionMatrix(num_classes=4)
    a.add_logits(x4.to(dev), y4.to(dev))
    b.add(_argmax_lowest(x4.float()), y4)
    assert torch.equal(a.matrix, b.matrix)


# ---- graph capture ----------------------------------------------------------
def test_dice_graph_replay_matches_eager(dev):
    """Forward and backward on static buffers, one stream, no parallel
    branches; replay after changing the input in place."""
    gen = torch.Generator().manual_seed(61)
    shape = (2, 1, 16, 16, 16)
    x = _make_logits(shape, torch.bfloat16, dev, gen)
    t = _labels(shape, 'uint8', gen).to(dev)
    w = (0.5 + torch.rand(shape, generator=gen)).to(dev)
    x.grad = torch.zeros_like(x)
    static_loss = torch.zeros((), device=dev)

    def fwd_bwd():
        x.grad.zero_()
        loss = ops.dice_loss_with_logits(x, t, beta=2.0, weights=w)
        (loss * x.numel()).backward()
        static_loss.copy_(loss.detach())

    for _ in range(3):
        fwd_bwd()
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        fwd_bwd()

    new = (2.0 * torch.randn(shape, generator=gen)).to(torch.bfloat16)
    with torch.no_grad():
        x.copy_(new.to(dev))
    g.replay()
    torch.cuda.synchronize()
    got_loss, got_grad = static_loss.clone(), x.grad.clone()

    fwd_bwd()   # eager, same new input
    torch.cuda.synchronize()
    assert torch.equal(got_loss, static_loss)
    assert torch.equal(got_grad, x.grad)
    ref_loss, ref_grad = _dice_ref(x, t, w, 2.0)
    torch.testing.assert_close(got_loss.double().cpu(), ref_loss, **LOSS_TOL)
    torch.testing.assert_close(got_grad.cpu(), ref_grad.to(torch.bfloat16),
                               **GRAD_TOL[torch.bfloat16])


# ---- end to end ---------------------------------------------------------------
def test_unet_multiclass_cross_entropy_end_to_end(dev):
    from coinstac_dinunet_amd.models import UNet3D
    torch.manual_seed(71)
    net = UNet3D(1, 3, widths=(16, 32)).to(dev)
    x = torch.randn(1, 1, 16, 16, 16, device=dev)
    y = torch.randint(0, 3, (1, 16, 16, 16), device=dev)
    logits = net(x)
    assert logits.shape == (1, 3, 16, 16, 16)
    loss = ops.cross_entropy(logits, y)
    loss.backward()
    ref = F.cross_entropy(logits.detach().double().cpu(), y.cpu())
    torch.testing.assert_close(loss.double().cpu(), ref, rtol=1e-2, atol=1e-3)
    for name, p in net.named_parameters():
        assert p.grad is not None, name
        assert torch.isfinite(p.grad.float()).all().item(), name
