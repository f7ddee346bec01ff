"""conv_transpose2x3d / OpsConvTranspose3d off the GPU, and UNet3D's
up_mode option."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from coinstac_dinunet_amd import ops
from coinstac_dinunet_amd.models import UNet3D


def test_cpu_fallback_is_conv_transpose3d():
    g = torch.Generator().manual_seed(11)
    x = torch.randn(2, 3, 2, 3, 5, generator=g)
    m = ops.OpsConvTranspose3d(3, 4, 2, stride=2)
    ref = F.conv_transpose3d(x, m.weight, m.bias, stride=2)
    assert torch.equal(ops.conv_transpose2x3d(x, m.weight, m.bias), ref)
    assert torch.equal(m(x), ref)
    assert list(m.state_dict()) == list(
        nn.ConvTranspose3d(3, 4, 2, stride=2).state_dict())


@pytest.mark.parametrize('kw', [dict(kernel_size=3, stride=2),
                                dict(kernel_size=2, stride=2,
                                     output_padding=1)])
def test_other_geometries_take_the_library(kw):
    g = torch.Generator().manual_seed(12)
    x = torch.randn(1, 3, 2, 3, 4, generator=g)
    m = ops.OpsConvTranspose3d(3, 2, **kw)
    ref = F.conv_transpose3d(x, m.weight, m.bias, stride=2,
                             output_padding=kw.get('output_padding', 0))
    assert torch.equal(m(x), ref)


@pytest.mark.parametrize('size', [(16, 16, 16), (13, 15, 17)])
def test_unet_transpose_keeps_the_input_size(size):
    net = UNet3D(in_channels=1, num_class=2, widths=(4, 8, 16),
                 up_mode='transpose')
    assert net(torch.randn(1, 1, *size)).shape == (1, 2) + size


def test_unet_default_mode_is_nearest_unchanged():
    torch.manual_seed(5)
    a = UNet3D(widths=(4, 8)).state_dict()
    torch.manual_seed(5)
    b = UNet3D(widths=(4, 8), up_mode='nearest').state_dict()
    assert list(a) == list(b)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert 'up_conv.0.bias' not in a
    assert 'up_conv.0.bias' in UNet3D(widths=(4, 8),
                                      up_mode='transpose').state_dict()
