"""CPU fallbacks of the segmentation-head functions against the plain-torch
formulas, and the threshold / tie rules they share with the HIP kernels."""
import pytest
import torch
import torch.nn.functional as F

from coinstac_dinunet_amd import ops
from coinstac_dinunet_amd.metrics import ConfusionMatrix, Prf1a
from coinstac_dinunet_amd.metrics import loss as loss_mod
from coinstac_dinunet_amd.metrics.loss import dice_loss_binary
from coinstac_dinunet_amd.metrics.metrics import COINNMetrics


def _counts(p):
    return p.tp, p.fp, p.tn, p.fn


@pytest.mark.parametrize('beta', [1.0, 2.0])
@pytest.mark.parametrize('weighted', [False, True])
def test_dice_with_logits_is_dice_of_sigmoid(beta, weighted):
    torch.manual_seed(0)
    x = torch.randn(2, 1, 5, 6, 7, requires_grad=True)
    t = (torch.rand(2, 1, 5, 6, 7) > 0.6).to(torch.uint8)
    w = 0.5 + torch.rand(2, 1, 5, 6, 7) if weighted else None
    loss = ops.dice_loss_with_logits(x, t, beta=beta, weights=w)
    ref_x = x.detach().clone().requires_grad_(True)
    ref = dice_loss_binary(torch.sigmoid(ref_x), t, beta, w, 1e-5)
    torch.testing.assert_close(loss, ref, rtol=0, atol=0)
    loss.backward()
    ref.backward()
    torch.testing.assert_close(x.grad, ref_x.grad, rtol=0, atol=0)
    assert loss_mod.dice_loss_with_logits is ops.dice_loss_with_logits


def test_cross_entropy_5d_cpu_unchanged():
    torch.manual_seed(1)
    x = torch.randn(2, 3, 4, 5, 6, requires_grad=True)
    y = torch.randint(0, 3, (2, 4, 5, 6))
    loss = ops.cross_entropy(x, y)
    ref_x = x.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(ref_x, y)
    torch.testing.assert_close(loss, ref, rtol=0, atol=0)
    loss.backward()
    ref.backward()
    torch.testing.assert_close(x.grad, ref_x.grad, rtol=0, atol=0)


@pytest.mark.parametrize('label_dtype', [torch.uint8, torch.bool,
                                         torch.int64])
def test_seg_prf1a_counts_cpu(label_dtype):
    torch.manual_seed(2)
    x = torch.randn(2, 1, 9, 11, 13)
    x.view(-1)[0::17] = 0.0
    x.view(-1)[5::17] = -0.0
    y = (torch.rand(2, 1, 9, 11, 13) > 0.5).to(label_dtype)
    cases = y.long().reshape(-1) * 2 + (x > 0).long().reshape(-1)
    ref = tuple(int((cases == c).sum()) for c in (3, 1, 0, 2))
    got = ops.seg_prf1a_counts(x, y)
    assert got == ref and all(isinstance(v, int) for v in got)
    with pytest.raises(TypeError):
        ops.seg_prf1a_counts(x, y.float())


def test_seg_confusion_matrix_cpu_lowest_index_on_ties():
    torch.manual_seed(3)
    K = 4
    x = torch.randn(2, K, 5, 6, 7).to(torch.bfloat16)
    x[0, :, 0, 0, 0] = 1.0                      # all four tie -> class 0
    x[0, :, 0, 0, 1] = torch.tensor([0., 2., 2., 1.]).to(x.dtype)  # -> 1
    x[0, :, 0, 0, 2] = torch.tensor([0., 1., 3., 3.]).to(x.dtype)  # -> 2
    y = torch.randint(0, K, (2, 5, 6, 7))
    pred = ops.argmax_lowest(x)
    assert pred[0, 0, 0, 0] == 0 and pred[0, 0, 0, 1] == 1 \
        and pred[0, 0, 0, 2] == 2
    idx = torch.arange(K).view(1, K, 1, 1, 1)
    expect = torch.where(x == x.amax(1, keepdim=True), idx, K).amin(1)
    assert torch.equal(pred, expect)
    ref = torch.bincount(y.reshape(-1) * K + expect.reshape(-1),
                         minlength=K * K).reshape(K, K)
    got = ops.seg_confusion_matrix(x, y, K)
    assert got.dtype == torch.int64 and torch.equal(got, ref)
    with pytest.raises(ValueError):
        ops.seg_confusion_matrix(x, y, K + 1)


def test_prf1a_add_logits_binary_rule_and_sigmoid_deviation():
    # x = 1e-8 is positive under the logit rule; fp32 sigmoid rounds it to
    # exactly 0.5, so the probability rule calls it negative — the one
    # documented deviation. Zeros of both signs are negative under both.
    x = torch.tensor([1e-8, 0.0, -0.0, 3.0, -3.0, 1e-8, 2.0, -1.0])
    y = torch.tensor([1, 1, 0, 1, 0, 0, 0, 1])
    assert not bool(torch.sigmoid(x[0]) > 0.5) and bool(x[0] > 0)
    a, b, c = Prf1a(), Prf1a(), Prf1a()
    a.add_logits(x, y)
    b.add((x > 0).long(), y)
    assert _counts(a) == _counts(b) == (2, 2, 2, 2)
    c.add((torch.sigmoid(x) > 0.5).long(), y)
    assert _counts(c) == (1, 1, 3, 3)


def test_prf1a_add_logits_two_plane_rule_with_tie():
    torch.manual_seed(4)
    x = torch.randn(2, 2, 5, 6, 7)
    x[:, 1, 0, 0, 0] = x[:, 0, 0, 0, 0]        # tie -> class 0 (negative)
    y = torch.randint(0, 2, (2, 5, 6, 7))
    y[:, 0, 0, 0] = 1
    a, b = Prf1a(), Prf1a()
    a.add_logits(x, y)
    pred = (x[:, 1] > x[:, 0]).long()
    assert int(pred[:, 0, 0, 0].sum()) == 0
    b.add(pred, y)
    assert _counts(a) == _counts(b)
    with pytest.raises(ValueError):
        a.add_logits(torch.randn(2, 3, 5, 6, 7), y)


def test_confusion_matrix_add_logits_matches_add():
    torch.manual_seed(5)
    K = 3
    x = torch.randn(2, K, 4, 4, 4)
    x[0, :, 1, 1, 1] = 0.5
    y = torch.randint(0, K, (2, 4, 4, 4))
    a, b = ConfusionMatrix(num_classes=K), ConfusionMatrix(num_classes=K)
    a.add_logits(x, y)
    b.add(ops.argmax_lowest(x), y)
    assert torch.equal(a.matrix, b.matrix)
    assert int(a.matrix.sum()) == y.numel()


def test_base_metrics_add_logits_not_implemented():
    with pytest.raises(NotImplementedError):
        COINNMetrics().add_logits(torch.zeros(2), torch.zeros(2))
