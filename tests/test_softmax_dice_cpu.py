"""The plain-torch multi-class soft-dice: dice_loss_multiclass against the
written-out float64 formula, and the CPU path of ops.softmax_dice_loss
against its composition."""
import pytest
import torch
import torch.nn.functional as F

from coinstac_dinunet_amd import ops
from coinstac_dinunet_amd.metrics import dice_loss_binary, dice_loss_multiclass
from coinstac_dinunet_amd.metrics.loss import softmax_dice_loss

N, C, SPATIAL = 2, 4, (3, 5, 7)


def _case(out_of_range):
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(N, C, *SPATIAL, generator=gen)
    y = torch.randint(0, C, (N, *SPATIAL), generator=gen)
    y[0][y[0] == C - 1] = 0            # a Y = 0 row
    if out_of_range:
        y[torch.rand(y.shape, generator=gen) < 0.1] = -1
    return x, y


@pytest.mark.parametrize('batch_dice', [False, True])
@pytest.mark.parametrize('include_background', [True, False])
def test_dice_loss_multiclass_matches_formula(include_background, batch_dice):
    x, y = _case(out_of_range=True)
    eps = 1e-5
    p = torch.softmax(x, 1)
    p64 = p.double().reshape(N, C, -1)
    t = y.reshape(N, -1)
    rows = []
    for c in range(0 if include_background else 1, C):
        sums = []
        for n in range(N):
            keep = t[n] >= 0
            hit = keep & (t[n] == c)
            sums.append((p64[n, c][hit].sum(), p64[n, c][keep].sum(),
                         hit.sum().double()))
        if batch_dice:
            sums = [tuple(sum(s[k] for s in sums) for k in range(3))]
        rows += [(2 * i + eps) / (pp + yy + eps) for i, pp, yy in sums]
    ref = 1 - sum(rows) / len(rows)
    got = dice_loss_multiclass(p, y, include_background, batch_dice, eps)
    torch.testing.assert_close(got.double(), ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('ce_weight', [0.0, 1.0])
def test_cpu_path_is_dice_plus_cross_entropy(ce_weight):
    x, y = _case(out_of_range=False)
    x.requires_grad_(True)
    got = ops.softmax_dice_loss(x, y, ce_weight=ce_weight, batch_dice=True)
    assert got.dim() == 0 and got.dtype == torch.float32
    ref = (dice_loss_multiclass(torch.softmax(x, 1), y, batch_dice=True)
           + ce_weight * F.cross_entropy(x, y))
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)
    got.backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert softmax_dice_loss is ops.softmax_dice_loss


def test_two_classes_foreground_batch_dice_is_binary_dice():
    gen = torch.Generator().manual_seed(6)
    x = torch.randn(N, 2, *SPATIAL, generator=gen)
    y = torch.randint(0, 2, (N, *SPATIAL), generator=gen)
    got = ops.softmax_dice_loss(x, y.bool(), include_background=False,
                                batch_dice=True)
    ref = dice_loss_binary(torch.softmax(x, 1)[:, 1], y)
    torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('classes', [1, 129])
def test_class_count_is_checked(classes):
    x = torch.zeros(1, classes, 2, 2, 2)
    y = torch.zeros(1, 2, 2, 2, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.softmax_dice_loss(x, y)
