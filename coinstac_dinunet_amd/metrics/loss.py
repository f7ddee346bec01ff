"""Segmentation losses (parity: reference metrics/loss.py:1-23).

dice_loss_with_logits is the fused form for training: it takes the logits,
runs as HIP kernels on GPU (ops/csrc/segloss.hip) and equals
dice_loss_binary(sigmoid(logits), ...). softmax_dice_loss is its multi-class
counterpart (ops/csrc/segdice.hip): dice_loss_multiclass(softmax(logits), ...)
plus an optional cross-entropy term."""
import torch

from ..ops import (dice_loss_with_logits,  # noqa: F401  (re-export)
                   softmax_dice_loss)


def dice_loss_binary(outputs, target, beta=1.0, weights=None, eps=1e-5):
    """Weighted soft-dice loss in beta-F-score form for binary segmentation.

    outputs: probabilities in [0,1], same shape as target.
    """
    outputs = outputs.reshape(-1).float()
    target = target.reshape(-1).float()
    if weights is not None:
        w = weights.reshape(-1).float()
        outputs = outputs * w
        target = target * w
    b2 = beta * beta
    intersection = (outputs * target).sum()
    num = (1 + b2) * intersection
    den = b2 * target.sum() + outputs.sum()
    return 1.0 - (num + eps) / (den + eps)


def dice_loss_multiclass(probs, target, include_background=True,
                         batch_dice=False, eps=1e-5):
    """Soft-dice loss for C classes: 1 - mean_r (2 I_r + eps) / (P_r + Y_r + eps).

    probs: [N, C, S...] class probabilities; target: [N, S...] class indices.
    A voxel whose label is outside [0, C) is dropped from every sum. Rows are
    (n, c), or c over the whole batch with batch_dice;
    include_background=False leaves the class-0 rows out of the mean.
    """
    N, C = probs.shape[:2]
    p = probs.reshape(N, C, -1).float()
    t = target.reshape(N, -1).long()
    keep = ((t >= 0) & (t < C)).unsqueeze(1)
    y = torch.nn.functional.one_hot(t.clamp(0, C - 1), C).permute(0, 2, 1)
    y = y.float() * keep
    p = p * keep
    dims = (0, 2) if batch_dice else (2,)
    dice = (2 * (p * y).sum(dims) + eps) / (p.sum(dims) + y.sum(dims) + eps)
    if not include_background:
        dice = dice[..., 1:]
    return 1.0 - dice.mean()
