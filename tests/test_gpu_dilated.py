"""Dilated 3x3x3 conv3d (dilation == padding == d) on the HIP path
(conv3d_dilated.hip): forward, dgrad, wgrad, routing and MeshNet, against
fp64 torch on the same bf16-rounded inputs.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.ops.conv import OpsConv3d

DEV = 'cuda:0'

# (N, Cin, Cout, D, H, W, d, bias)
CASES = [
    (1, 16, 16, 4, 8, 16, 2, False),    # aligned baseline
    (2, 48, 40, 5, 7, 13, 2, True),     # ragged k/Cout tiles, odd W, classes
    (1, 32, 32, 3, 9, 24, 4, False),    # D < d: kd != 1 is all padding
    (1, 20, 24, 6, 10, 11, 3, True),    # odd d, unaligned shifts
    (1, 32, 16, 2, 18, 40, 16, False),  # d = 16 > D, H just over d, W tiles
    (1, 64, 72, 9, 6, 32, 8, False),    # several k and Cout tiles, d > H
    (1, 3, 5, 3, 3, 3, 2, True),        # everything tiny
]


def _problem(N, Cin, Cout, D, H, W, d, bias):
    """bf16 (x, w, bias or None, go) on the GPU, seeded on the CPU."""
    g = torch.Generator(device='cpu').manual_seed(
        hash((N, Cin, Cout, D, H, W, d)) % 2 ** 31)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    b = torch.randn(Cout, generator=g).to(DEV, torch.bfloat16)
    go = torch.randn(N, Cout, D, H, W, generator=g).to(DEV, torch.bfloat16)
    return x, w, (b if bias else None), go


@pytest.mark.parametrize('case', CASES)
def test_conv3d_dilated_fwd(case):
    d = case[6]
    x, w, b, _ = _problem(*case)
    ref = F.conv3d(x.double(), w.double(), None if b is None else b.double(),
                   padding=d, dilation=d)
    out = ops.conv3d(x, w, b, dilation=d)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    atol = 5e-2 * (27 * case[1]) ** 0.5 * 0.2
    err = (out.double() - ref).abs().max().item()
    print(f'conv3d_dil fwd {case}: max abs err {err:.4g}, atol {atol:.4g}')
    torch.testing.assert_close(out.double(), ref, rtol=5e-2, atol=atol)


@pytest.mark.parametrize('case', CASES)
def test_conv3d_dilated_backward(case):
    N, Cin, Cout, D, H, W, d, _ = case
    x, w, b, go = _problem(*case)
    leaves = [t.double().requires_grad_(True) for t in (x, w)]
    if b is not None:
        leaves.append(b.double().requires_grad_(True))
    F.conv3d(*leaves, padding=d, dilation=d).backward(go.double())

    got = [t.clone().requires_grad_(True)
           for t in (x, w) + (() if b is None else (b,))]
    ops.conv3d(*got, dilation=d).backward(go)

    S = N * D * H * W
    atols = [5e-2 * (27 * Cout) ** 0.5 * 0.2, 3e-2 * S ** 0.5 * 0.03,
             5e-2 * S ** 0.5 * 0.1]
    for name, g, r, atol in zip(('dx', 'dw', 'dbias'), got, leaves, atols):
        assert g.grad.dtype == g.dtype and g.grad.shape == g.shape
        err = (g.grad.double() - r.grad).abs().max().item()
        print(f'conv3d_dil bwd {case}: {name} max abs err {err:.4g}, '
              f'atol {atol:.4g}')
        torch.testing.assert_close(g.grad.double(), r.grad, rtol=5e-2,
                                   atol=atol)


def _shifted(t, off):
    """out[..., p] = t[..., p + off] per spatial axis, zero outside."""
    out = torch.zeros_like(t)
    src, dst = [Ellipsis], [Ellipsis]
    for o, n in zip(off, t.shape[2:]):
        if abs(o) >= n:
            return out
        src.append(slice(max(o, 0), n + min(o, 0)))
        dst.append(slice(max(-o, 0), n - max(o, 0)))
    out[tuple(dst)] = t[tuple(src)]
    return out


@pytest.mark.parametrize('d', [2, 4])
@pytest.mark.parametrize('tap', [(0, 1, 1), (1, 2, 0), (2, 0, 2), (0, 0, 0)])
def test_conv3d_dilated_tap_isolation(tap, d):
    """Identity weight on one off-centre tap: the output is x shifted by
    d*(k - 1) per axis and dx is go shifted the other way, exactly."""
    x, w, _, go = _problem(1, 16, 16, 6, 9, 40, d, False)
    w1 = torch.zeros_like(w)
    w1[torch.arange(16), torch.arange(16), tap[0], tap[1], tap[2]] = 1
    off = [d * (k - 1) for k in tap]
    xg = x.clone().requires_grad_(True)
    out = ops.conv3d(xg, w1, dilation=d)
    out.backward(go)
    assert torch.equal(out.detach(), _shifted(x, off))
    assert torch.equal(xg.grad, _shifted(go, [-o for o in off]))


def test_opsconv3d_dilated_routing():
    """dilation == padding takes the native path (bf16 out for fp32 in);
    padding != dilation stays on the library conv."""
    torch.manual_seed(0)
    x = torch.randn(1, 16, 4, 8, 16, device=DEV)
    native = OpsConv3d(16, 16, 3, padding=2, dilation=2).to(DEV)
    out = native(x)
    assert out.dtype == torch.bfloat16 and out.shape == x.shape
    ref = F.conv3d(x, native.weight, native.bias, padding=2, dilation=2)
    torch.testing.assert_close(out.float(), ref, rtol=5e-2,
                               atol=5e-2 * (27 * 16) ** 0.5 * 0.2)
    lib = OpsConv3d(16, 16, 3, padding=1, dilation=2).to(DEV)
    out = lib(x)
    ref = F.conv3d(x, lib.weight, lib.bias, padding=1, dilation=2)
    assert out.dtype == torch.float32
    torch.testing.assert_close(out, ref)


def test_meshnet_matches_cpu_reference():
    """One mean-cross-entropy step of MeshNet against a float64 copy on the
    CPU; logits within test_unet_gpu_matches_cpu_reference's bound."""
    from coinstac_dinunet_amd.models import MeshNet
    torch.manual_seed(0)
    net = MeshNet(in_channels=1, num_class=2, channels=16,
                  dilations=(1, 2, 4, 2, 1))
    ref_net = copy.deepcopy(net).double()
    net = net.to(DEV)
    g = torch.Generator(device='cpu').manual_seed(1616)
    x = torch.randn(1, 1, 16, 16, 16, generator=g)
    y = torch.randint(0, 2, (1, 16, 16, 16), generator=g)
    ref = ref_net(x.double())
    F.cross_entropy(ref, y).backward()
    out = net(x.to(DEV))
    ops.cross_entropy(out.float(), y.to(DEV)).backward()
    for i in (2, 4, 6):  # the d = 2, 4, 2 convs
        g_ref = ref_net.layers[i].weight.grad
        g_gpu = net.layers[i].weight.grad
        assert torch.isfinite(g_gpu).all()
        rel = ((g_gpu.double().cpu() - g_ref).norm() / g_ref.norm()).item()
        print(f'meshnet layers[{i}] (d = {net.layers[i].dilation[0]}) grad '
              f'rel L2 err vs fp64: {rel:.4g}')
    torch.testing.assert_close(out.detach().double().cpu(), ref.detach(),
                               rtol=1e-1, atol=1e-1)
