"""upsample2_conv3d's CPU fallback and the pure routing predicates."""
import torch
import torch.nn.functional as F

from coinstac_dinunet_amd import ops
from coinstac_dinunet_amd.ops.conv import (OpsConv3d, can_fuse_upsample,
                                           route_upconv3d)


def test_upsample2_conv3d_cpu_is_interpolate_then_conv():
    g = torch.Generator().manual_seed(7)
    x = torch.randn(2, 3, 2, 3, 5, generator=g, requires_grad=True)
    w = torch.randn(4, 3, 3, 3, 3, generator=g, requires_grad=True)
    b = torch.randn(4, generator=g, requires_grad=True)
    go = torch.randn(2, 4, 4, 6, 10, generator=g)
    out = ops.upsample2_conv3d(x, w, b)
    grads = torch.autograd.grad(out, (x, w, b), go)
    ref = F.conv3d(F.interpolate(x, scale_factor=2, mode='nearest'), w, b,
                   padding=1)
    ref_grads = torch.autograd.grad(ref, (x, w, b), go)
    assert torch.equal(out, ref)
    for a, r in zip(grads, ref_grads):
        assert torch.equal(a, r)


def test_can_fuse_upsample_false_on_cpu_and_for_non_doubling_size():
    conv = OpsConv3d(4, 4, 3, padding=1, bias=False)
    x = torch.zeros(1, 4, 2, 3, 4)
    assert not can_fuse_upsample(conv, x, (4, 6, 8))
    assert not can_fuse_upsample(conv, x, (4, 6, 9))


def test_route_upconv3d():
    assert route_upconv3d(32, 16, 16) == 'collapsed'
    assert route_upconv3d(8, 5, 6) == 'composed'
