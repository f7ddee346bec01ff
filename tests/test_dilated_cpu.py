"""ops.conv3d's dilation keyword and MeshNet off the GPU."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from coinstac_dinunet_amd import ops
from coinstac_dinunet_amd.models import MeshNet


def test_conv3d_dilation_cpu_is_torch():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 3, 5, 6, 7, generator=g)
    w = torch.randn(4, 3, 3, 3, 3, generator=g)
    b = torch.randn(4, generator=g)
    go = torch.randn(2, 4, 5, 6, 7, generator=g)
    ref_in = [t.clone().requires_grad_(True) for t in (x, w, b)]
    ref = F.conv3d(*ref_in, padding=2, dilation=2)
    ref.backward(go)
    got_in = [t.clone().requires_grad_(True) for t in (x, w, b)]
    out = ops.conv3d(*got_in, dilation=2)
    out.backward(go)
    assert torch.equal(out, ref)
    for a, r in zip(got_in, ref_in):
        assert torch.equal(a.grad, r.grad)


def test_meshnet_cpu_shape_and_backward():
    torch.manual_seed(0)
    net = MeshNet(in_channels=2, num_class=3, channels=4,
                  dilations=(1, 2, 3, 1), dropout=0.1)
    out = net(torch.randn(2, 2, 6, 7, 8))
    assert out.shape == (2, 3, 6, 7, 8)
    out.square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in net.parameters())


def test_meshnet_state_dict_round_trip():
    """The same stack from plain nn modules has the same keys and, with the
    weights loaded, the same output."""
    torch.manual_seed(0)
    dil = (1, 2, 4, 1)
    layers, c_in = [], 1
    for d in dil:
        layers += [nn.Conv3d(c_in, 4, 3, padding=d, dilation=d, bias=False),
                   nn.BatchNorm3d(4)]
        c_in = 4
    layers.append(nn.Conv3d(4, 2, 1))
    plain = nn.Sequential(*layers)
    net = MeshNet(in_channels=1, num_class=2, channels=4, dilations=dil)
    sd = {'layers.' + k: v for k, v in plain.state_dict().items()}
    assert set(sd) == set(net.state_dict())
    net.load_state_dict(sd)
    plain.load_state_dict({k[len('layers.'):]: v
                           for k, v in net.state_dict().items()})
    x = torch.randn(1, 1, 6, 6, 6)
    ref = x
    for m in plain.eval():
        ref = F.relu(m(ref)) if isinstance(m, nn.BatchNorm3d) else m(ref)
    torch.testing.assert_close(net.eval()(x), ref)
