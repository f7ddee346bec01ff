"""GroupNorm / InstanceNorm (+ReLU / LeakyReLU) HIP kernels (groupnorm.hip)
against float64 F.group_norm on the same bf16-quantized x and dy.

Tolerances: y and dx are rounded once to bf16 (relative 2^-9), so
rtol = atol = 1e-2; dgamma and dbeta are fp32 sums of N*S exact products:
rtol = 1e-3, atol = 1e-3 * sqrt(N*S). Nothing is excluded from a
comparison: each seed is chosen so that no reference z lies within 1e-4 of
the activation's kink, which the test asserts.

The entry points allocate their outputs, so the out-of-bounds check is the
S = 75 and S = 210 cases: planes start misaligned there, and a store past a
plane's end would land in the neighbouring channel, which is compared too.
"""
import copy
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.ops.groupnorm import (OpsGroupNorm,
                                                    OpsInstanceNorm3d)

DEV = torch.device('cuda:0')
ACTS = {'none': (False, 0.0), 'relu': (True, 0.0), 'leaky': (True, 0.01)}
# (N, C, G, spatial): seed with min |z| > 1e-4 on the reference
SHAPES = {
    (2, 8, 2, (5, 6, 7)): 0,       # S = 210, not a multiple of 8
    (2, 8, 8, (3, 5, 5)): 0,       # instance norm, S = 75 odd
    (3, 6, 1, (4, 4, 4)): 0,       # one group
    (1, 4, 2, (1, 1, 5)): 0,       # plane shorter than one vector
    (2, 16, 4, (8, 16, 16)): 59,   # aligned fast path
}


def reference(N, C, G, spatial, act, seed, scale=1.0, offset=0.0):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, *spatial, generator=g) * scale + offset).bfloat16()
    dy = torch.randn(N, C, *spatial, generator=g).bfloat16()
    gamma = torch.randn(C, generator=g).abs() + 0.5
    beta = torch.randn(C, generator=g)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    z = F.group_norm(xr, G, gr, br, 1e-5)
    relu, slope = ACTS[act]
    ref = F.leaky_relu(z, slope) if relu else z
    ref.backward(dy.double())
    return x, dy, gamma, beta, z.detach(), ref.detach(), (xr.grad, gr.grad,
                                                          br.grad)


def check(N, C, G, spatial, act, seed, **kw):
    x, dy, gamma, beta, z, ref, grads = reference(N, C, G, spatial, act,
                                                  seed, **kw)
    relu, slope = ACTS[act]
    if relu:
        assert z.abs().min() > 1e-4
    xg, gg, bg = (t.to(DEV).requires_grad_(True) for t in (x, gamma, beta))
    y = ops.group_norm(xg, G, gg, bg, 1e-5, relu, slope)
    y.backward(dy.to(DEV))
    assert y.dtype == torch.bfloat16 and xg.grad.dtype == torch.bfloat16
    tol = dict(rtol=1e-2, atol=1e-2)
    torch.testing.assert_close(y.double().cpu(), ref, **tol)
    torch.testing.assert_close(xg.grad.double().cpu(), grads[0], **tol)
    tol = dict(rtol=1e-3, atol=1e-3 * math.sqrt(N * math.prod(spatial)))
    torch.testing.assert_close(gg.grad.double().cpu(), grads[1], **tol)
    torch.testing.assert_close(bg.grad.double().cpu(), grads[2], **tol)


@pytest.mark.parametrize('act', list(ACTS))
@pytest.mark.parametrize('shape', list(SHAPES), ids=str)
def test_forward_backward(shape, act):
    check(*shape, act, SHAPES[shape])


def test_split_rows():
    """L = 131072 per row on 4 rows: statistics and backward both split."""
    C = ops.require_native()
    assert C.gn_splits(4 * 32 ** 3, 2 * 2) > 1
    assert C.gn_splits(32 ** 3, 2 * 8) > 1
    check(2, 8, 2, (32, 32, 32), 'none', 0)


def test_large_mean_does_not_cancel():
    """|mean| = 60 std: sum / sum-of-squares statistics in fp32 miss the
    variance by percent here."""
    check(2, 8, 2, (16, 16, 16), 'none', 0, scale=0.5, offset=30.0)


@pytest.mark.parametrize('make, stock', [
    (lambda: OpsGroupNorm(4, 8, relu=True), lambda: nn.GroupNorm(4, 8)),
    (lambda: OpsInstanceNorm3d(8, affine=True, relu=True,
                               negative_slope=0.01),
     lambda: nn.InstanceNorm3d(8, affine=True))], ids=['group', 'instance'])
def test_modules_load_stock_state_and_ignore_mode(make, stock):
    torch.manual_seed(0)
    src = stock()
    nn.init.normal_(src.weight)
    nn.init.normal_(src.bias)
    m = make()
    m.load_state_dict(src.state_dict())
    m = m.to(DEV)
    x = torch.randn(2, 8, 3, 5, 5, device=DEV)
    y_train, y_eval = m.train()(x), m.eval()(x)
    assert torch.equal(y_train, y_eval)
    ref = F.leaky_relu(src.double()(x.bfloat16().double().cpu()),
                       m.negative_slope)
    torch.testing.assert_close(y_train.double().cpu(), ref, rtol=1e-2,
                               atol=1e-2)


class StockNormReLU(nn.Module):
    """nn.GroupNorm / nn.InstanceNorm3d + ReLU with an Ops module's weights."""

    def __init__(self, m):
        super().__init__()
        if isinstance(m, nn.GroupNorm):
            self.norm = nn.GroupNorm(m.num_groups, m.num_channels, m.eps)
        else:
            self.norm = nn.InstanceNorm3d(m.num_features, m.eps, affine=True)
        self.norm.load_state_dict(m.state_dict())
        self.norm.to(m.weight.device)

    def forward(self, x):
        return F.relu(self.norm(x.float()))


def with_stock_norms(net):
    net = copy.deepcopy(net)
    for mod in list(net.modules()):
        for name, child in mod.named_children():
            if isinstance(child, (OpsGroupNorm, OpsInstanceNorm3d)):
                setattr(mod, name, StockNormReLU(child))
    return net


@pytest.mark.parametrize('model', ['unet-group', 'meshnet-instance'])
def test_model_matches_stock_norm_modules(model):
    from coinstac_dinunet_amd.models import MeshNet, UNet3D
    torch.manual_seed(0)
    if model == 'unet-group':
        net = UNet3D(widths=(8, 16), norm='group', norm_groups=4)
    else:
        net = MeshNet(channels=8, dilations=(1, 2, 1), norm='instance')
    for p in net.parameters():      # non-trivial gamma / beta
        if p.dim() == 1:
            nn.init.normal_(p, 1.0, 0.2)
    net = net.to(DEV)
    ref_net = with_stock_norms(net)
    assert not any(isinstance(m, (OpsGroupNorm, OpsInstanceNorm3d))
                   for m in ref_net.modules())
    x = torch.randn(2, 1, 16, 16, 16, device=DEV)
    out = net(x)
    out.float().square().mean().backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all()
               for p in net.parameters())
    torch.testing.assert_close(out.float(), ref_net(x).float(), rtol=0,
                               atol=5e-2)
