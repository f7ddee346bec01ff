"""ops.softmax_dice_loss (ops/csrc/segdice.hip) against a float64 CPU
reference written out here from the definition, computed from the same,
already dtype-rounded, logits.

Tolerances are those of test_gpu_segloss.py: loss rtol=1e-5/atol=1e-6, fp32
gradients rtol=1e-4/atol=1e-6, bf16/fp16 gradients rtol=1e-2/atol=1e-3
against the float64 gradient cast to that dtype. Gradients are taken of
loss * N * S so their entries are O(1).

Dispatch boundaries covered by C: 4|5 (register class cap 4 -> 8), 8|9
(register -> LDS tile), and the tile widths 512|256 at 25|26, 256|128 at
55|56, 128|64 at 111|112 (tile_voxels in segdice.hip)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops

LOSS_TOL = dict(rtol=1e-5, atol=1e-6)
GRAD_TOL = {torch.float32: dict(rtol=1e-4, atol=1e-6),
            torch.bfloat16: dict(rtol=1e-2, atol=1e-3),
            torch.float16: dict(rtol=1e-2, atol=1e-3)}

# 315: odd, scalar instance, less than one 512-voxel tile. 640 = 4*8*20:
# 16-byte instance, partial last tile at widths 512 and 256 but whole tiles
# at 128 and 64. 672 = 4*8*21 is a multiple of 8 and no multiple of 64, so
# the 16-byte instance ends in a partial tile at every width
# (512 + 160 = 2*256 + 160 = 5*128 + 32 = 10*64 + 32).
SPATIAL = [(5, 7, 9), (4, 8, 20), (4, 8, 21)]

# The register path caps its grid at 2048 blocks of 256 threads, one 16-byte
# vector of 8 bf16 voxels per thread per sweep: 2048 * 256 * 8 = 4 194 304
# voxels. 136*136*240 = 4 439 040 exceeds it, so blocks take a second vector.
BIG = (136, 136, 240)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _reference(x, y, ce_weight, include_background, batch_dice, eps=1e-5):
    """float64 loss and d(loss * N * S)/dx on the CPU, from the definition."""
    x64 = x.detach().double().cpu().requires_grad_(True)
    N, C = x64.shape[:2]
    t = y.cpu().long().reshape(N, -1)
    keep = (t >= 0) & (t < C)
    xs = x64.reshape(N, C, -1)
    p = torch.softmax(xs, 1) * keep.unsqueeze(1)
    onehot = (t.unsqueeze(1) == torch.arange(C).view(1, C, 1)).double()
    dims = (0, 2) if batch_dice else (2,)
    dice = ((2 * (p * onehot).sum(dims) + eps)
            / (p.sum(dims) + onehot.sum(dims) + eps))
    if not include_background:
        dice = dice[..., 1:]
    nll = torch.logsumexp(xs, 1) - xs.gather(
        1, t.clamp(0, C - 1).unsqueeze(1)).squeeze(1)
    loss = 1 - dice.mean() + ce_weight * (nll * keep).sum() / t.numel()
    (loss * t.numel()).backward()
    return loss.detach(), x64.grad, keep


def _logits(shape, dtype, dev, gen, misaligned=False):
    n = 1
    for s in shape:
        n *= s
    vals = (2.0 * torch.randn(n + 1, generator=gen)).to(dtype).to(dev)
    # buf[1:] starts one element (2 or 4 bytes) past a 16-byte boundary
    x = vals[1:] if misaligned else vals[:n].clone()
    assert (x.data_ptr() % 16 != 0) == misaligned
    return x.view(shape).detach().requires_grad_(True)


def _labels(N, C, spatial, label_dtype, gen, drop_sample=False):
    """Class indices with class C-1 absent from sample 0 (a Y = 0 row), a
    sprinkling of out-of-range voxels and, on request, sample 1 all dropped."""
    y = torch.randint(0, C, (N, *spatial), generator=gen)
    y[0][y[0] == C - 1] = 0
    if label_dtype == torch.bool:
        return y.bool()
    bad = 255 if label_dtype == torch.uint8 else -1
    y[torch.rand(y.shape, generator=gen) < 0.1] = bad
    if drop_sample:
        y[1] = bad
    return y.to(label_dtype)


def _check(x, y, ce_weight, include_background, batch_dice):
    ref_loss, ref_grad, keep = _reference(x, y, ce_weight, include_background,
                                          batch_dice)
    x.grad = None
    loss = ops.softmax_dice_loss(x, y, ce_weight=ce_weight,
                                 include_background=include_background,
                                 batch_dice=batch_dice)
    assert loss.dtype == torch.float32 and loss.dim() == 0
    (loss * y.numel()).backward()
    print(f'sdice {tuple(x.shape)} {x.dtype} {y.dtype}: '
          f'loss={loss.item():.9g} ref={ref_loss.item():.9g}')
    torch.testing.assert_close(loss.double().cpu(), ref_loss, **LOSS_TOL)
    assert x.grad.dtype == x.dtype and x.grad.shape == x.shape
    got = x.grad.cpu()
    torch.testing.assert_close(got, ref_grad.to(x.dtype), **GRAD_TOL[x.dtype])
    N, C = x.shape[:2]
    dropped = ~keep.unsqueeze(1).expand(N, C, -1)
    assert (got.reshape(N, C, -1)[dropped] == 0).all()
    return loss.detach().clone(), x.grad.clone()


# (C, label dtype, ce_weight, include_background, batch_dice, drop sample 1)
GRID = [(2, torch.bool, 1.0, False, True, False),
        (2, torch.int64, 0.0, True, False, True),
        (3, torch.uint8, 1.0, True, True, False),
        (4, torch.int64, 1.0, False, False, False),
        (5, torch.uint8, 0.0, False, False, True),
        (8, torch.int64, 1.0, True, True, False),
        (9, torch.uint8, 1.0, True, False, True),
        (25, torch.int64, 0.0, False, True, False),
        (26, torch.uint8, 1.0, True, False, False),
        (33, torch.int64, 1.0, False, False, True),
        (55, torch.uint8, 0.0, True, True, False),
        (56, torch.int64, 1.0, False, True, False),
        (111, torch.uint8, 1.0, True, False, False),
        (112, torch.int64, 0.0, False, False, False),
        (128, torch.uint8, 1.0, True, True, True)]


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('spatial', SPATIAL)
@pytest.mark.parametrize('C,label_dtype,ce_weight,bg,batch,drop', GRID)
def test_softmax_dice(dev, C, label_dtype, ce_weight, bg, batch, drop,
                      spatial, dtype):
    gen = torch.Generator().manual_seed(100 * C + spatial[0])
    x = _logits((2, C, *spatial), dtype, dev, gen)
    y = _labels(2, C, spatial, label_dtype, gen, drop)
    assert not (y[0] == C - 1).any()
    if label_dtype != torch.bool:
        assert (y.long() >= C).any() or (y < 0).any()
    _check(x, y.to(dev), ce_weight, bg, batch)


@pytest.mark.parametrize('C', [4, 33])
@pytest.mark.parametrize('spatial', SPATIAL)
def test_softmax_dice_fp16(dev, C, spatial):
    gen = torch.Generator().manual_seed(7 + C)
    x = _logits((2, C, *spatial), torch.float16, dev, gen)
    y = _labels(2, C, spatial, torch.uint8, gen)
    _check(x, y.to(dev), 1.0, True, False)


@pytest.mark.parametrize('C', [3, 33])
def test_softmax_dice_misaligned_base(dev, C):
    gen = torch.Generator().manual_seed(8 + C)
    x = _logits((2, C, *SPATIAL[2]), torch.bfloat16, dev, gen,
                misaligned=True)
    y = _labels(2, C, SPATIAL[2], torch.int64, gen)
    _check(x, y.to(dev), 1.0, True, False)


def test_softmax_dice_grid_cap(dev):
    gen = torch.Generator().manual_seed(9)
    x = _logits((1, 2, *BIG), torch.bfloat16, dev, gen)
    y = _labels(1, 2, BIG, torch.uint8, gen)
    _check(x, y.to(dev), 1.0, True, False)


def test_softmax_dice_tile_grid_cap(dev):
    """Tile path: 1024 blocks cap, 256-voxel tiles at C = 33, so more than
    1024 * 256 = 262 144 voxels make a block loop: 72*72*56 = 290 304."""
    gen = torch.Generator().manual_seed(10)
    spatial = (72, 72, 56)
    x = _logits((1, 33, *spatial), torch.bfloat16, dev, gen)
    y = _labels(1, 33, spatial, torch.uint8, gen)
    _check(x, y.to(dev), 1.0, False, False)


@pytest.mark.parametrize('C', [5, 33])
def test_softmax_dice_reproducible(dev, C):
    gen = torch.Generator().manual_seed(11 + C)
    x = _logits((2, C, 16, 24, 40), torch.bfloat16, dev, gen)
    y = _labels(2, C, (16, 24, 40), torch.int64, gen).to(dev)
    first = _check(x, y, 1.0, True, True)
    second = _check(x, y, 1.0, True, True)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])


@pytest.mark.parametrize('C', [1, 129])
def test_softmax_dice_refuses_class_count(dev, C):
    x = torch.zeros(1, C, 4, 4, 4, device=dev)
    y = torch.zeros(1, 4, 4, 4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match='dice_loss_with_logits' if C == 1
                       else '128'):
        ops.softmax_dice_loss(x, y)
