"""ConvTranspose3d kernel 2 / stride 2 on the HIP path (deconv3d.hip):
forward with bias, dgrad, wgrad and UNet3D(up_mode='transpose'), against
fp64 torch on the same bf16-rounded inputs.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops

DEV = 'cuda:0'

# (N, Cin, Cout, D, H, W, bias) of the low-res input
CASES = [
    (2, 48, 40, 3, 5, 6, True),     # ragged k-step and Cout tile, odd D/H
    (1, 16, 8, 1, 1, 8, False),     # below one k-step / fragment, one row
    (1, 72, 136, 2, 4, 7, True),    # k tail, several Cout tiles, odd W
    (2, 32, 32, 2, 8, 24, False),   # full tiles, W over several tiles
    (1, 3, 5, 2, 3, 3, True),       # everything tiny and odd
]


def _problem(N, Cin, Cout, D, H, W, bias):
    """bf16 (x, w, bias or None, go) on the GPU, seeded on the CPU."""
    g = torch.Generator(device='cpu').manual_seed(
        hash((N, Cin, Cout, D, H, W)) % 2 ** 31)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cin, Cout, 2, 2, 2, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    b = torch.randn(Cout, generator=g).to(DEV, torch.bfloat16)
    go = torch.randn(N, Cout, 2 * D, 2 * H, 2 * W, generator=g).to(
        DEV, torch.bfloat16)
    return x, w, (b if bias else None), go


def _ref(x, w, b):
    return F.conv_transpose3d(x.double(), w.double(),
                              None if b is None else b.double(), stride=2)


@pytest.mark.parametrize('case', CASES)
def test_conv_transpose2x3d_fwd(case):
    x, w, b, _ = _problem(*case)
    ref = _ref(x, w, b)
    out = ops.conv_transpose2x3d(x, w, b)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    atol = 5e-2 * case[1] ** 0.5 * 0.2
    err = (out.double() - ref).abs().max().item()
    print(f'deconv3d fwd {case}: max abs err {err:.4g}, atol {atol:.4g}')
    torch.testing.assert_close(out.double(), ref, rtol=5e-2, atol=atol)


@pytest.mark.parametrize('case', CASES)
def test_conv_transpose2x3d_backward(case):
    """dbias is held to test_gpu_fusebn's bias-gradient bound,
    5e-2 * sqrt(positions summed) * 0.1."""
    N, Cin, Cout, D, H, W, _ = case
    x, w, b, go = _problem(*case)
    leaves = [t.double().requires_grad_(True) for t in (x, w)]
    if b is not None:
        leaves.append(b.double().requires_grad_(True))
    F.conv_transpose3d(*leaves, stride=2).backward(go.double())

    got = [t.clone().requires_grad_(True)
           for t in (x, w) + (() if b is None else (b,))]
    ops.conv_transpose2x3d(*got).backward(go)

    S = N * D * H * W
    atols = [5e-2 * (8 * Cout) ** 0.5 * 0.2, 3e-2 * S ** 0.5 * 0.03,
             5e-2 * (8 * S) ** 0.5 * 0.1]
    for name, g, r, atol in zip(('dx', 'dw', 'dbias'), got, leaves, atols):
        assert g.grad.dtype == g.dtype and g.grad.shape == g.shape
        err = (g.grad.double() - r.grad).abs().max().item()
        print(f'deconv3d bwd {case}: {name} max abs err {err:.4g}, '
              f'atol {atol:.4g}')
        torch.testing.assert_close(g.grad.double(), r.grad, rtol=5e-2,
                                   atol=atol)


def test_conv_transpose2x3d_single_class():
    """Weight zero except class (pd, ph, pw) = (1, 0, 1): the output is
    exactly zero off that class and right on it."""
    x, w, _, _ = _problem(1, 32, 16, 2, 4, 8, False)
    w1 = torch.zeros_like(w)
    w1[:, :, 1, 0, 1] = w[:, :, 1, 0, 1]
    out = ops.conv_transpose2x3d(x, w1)
    on = torch.zeros_like(out, dtype=torch.bool)
    on[:, :, 1::2, 0::2, 1::2] = True
    assert out[~on].abs().max().item() == 0.0
    assert out[on].abs().max().item() > 0.0
    torch.testing.assert_close(out.double(), _ref(x, w1, None), rtol=5e-2,
                               atol=5e-2 * 32 ** 0.5 * 0.2)


def test_unet_transpose_matches_cpu_reference():
    """One mean-cross-entropy step of UNet3D(up_mode='transpose') against a
    float64 copy on the CPU; logits within
    test_unet_gpu_matches_cpu_reference's bound."""
    from coinstac_dinunet_amd.models import UNet3D
    torch.manual_seed(0)
    net = UNet3D(in_channels=1, num_class=2, widths=(16, 32),
                 up_mode='transpose')
    ref_net = copy.deepcopy(net).double()
    net = net.to(DEV)
    g = torch.Generator(device='cpu').manual_seed(1616)
    x = torch.randn(1, 1, 16, 16, 16, generator=g)
    y = torch.randint(0, 2, (1, 16, 16, 16), generator=g)
    ref = ref_net(x.double())
    F.cross_entropy(ref, y).backward()
    out = net(x.to(DEV))
    ops.cross_entropy(out.float(), y.to(DEV)).backward()
    g_ref = ref_net.up_conv[0].weight.grad
    g_gpu = net.up_conv[0].weight.grad
    assert torch.isfinite(g_gpu).all()
    rel = ((g_gpu.double().cpu() - g_ref).norm() / g_ref.norm()).item()
    print(f'unet transpose up_conv[0] grad rel L2 err vs fp64: {rel:.4g}')
    torch.testing.assert_close(out.detach().double().cpu(), ref.detach(),
                               rtol=1e-1, atol=1e-1)
