"""Collapsed backward of nearest-2x upsample + 3x3x3 conv (upconv3d_dgrad,
upconv3d_wgrad in upconv3d.hip) against fp64 autograd through
F.conv3d(F.interpolate(x, 2, 'nearest'), w, padding=1) on the same
bf16-rounded inputs, at test_upsample2_conv3d_backward's tolerances: the
only new rounding is the once-rounded slot sums the forward is held to.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.ops import conv as opsconv
    C = ops.require_native()

DEV = 'cuda:0'

# (N, Cin, Cout, D, H, W) of the low-res input
CASES = [
    (2, 48, 40, 3, 16, 16),   # ragged ci and co tiles, odd D, N > 1
    (1, 32, 32, 1, 8, 8),     # D = 1: both depth halos; whole-plane instance
    (2, 80, 16, 5, 8, 8),     # three ci tiles, half co k-tile, ragged depth
    (1, 32, 64, 2, 12, 16),   # H no multiple of the row tile; two co k-tiles
    (1, 16, 32, 2, 16, 24),   # W a multiple of 8 not of 16; Cin < one k-step
]


@functools.lru_cache(maxsize=None)
def _problem(case):
    """bf16 (x, w, bias, go) on the GPU, seeded on the CPU, and the fp64
    reference (dx, dw, dbias) on the same rounded values."""
    N, Cin, Cout, D, H, W = case
    g = torch.Generator(device='cpu').manual_seed(hash(case) % 2 ** 31)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    bias = torch.randn(Cout, generator=g).to(DEV, torch.bfloat16)
    go = torch.randn(N, Cout, 2 * D, 2 * H, 2 * W, generator=g).to(
        DEV, torch.bfloat16)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    br = bias.double().requires_grad_(True)
    F.conv3d(F.interpolate(xr, scale_factor=2, mode='nearest'), wr, br,
             padding=1).backward(go.double())
    return x, w, bias, go, (xr.grad, wr.grad, br.grad)


def _dx_atol(case):
    return 5e-2 * (case[2] * 27 * 8) ** 0.5 * 0.2


def _dw_atol(case):
    N, _, _, D, H, W = case
    return 3e-2 * (8 * N * D * H * W) ** 0.5 * 0.03


@pytest.mark.parametrize('case', CASES)
def test_upconv3d_dgrad(case):
    x, w, _, go, (dx_ref, _, _) = _problem(case)
    dx = C.upconv3d_dgrad(go, w, list(x.shape))
    assert dx.shape == x.shape and dx.dtype == torch.bfloat16
    err = (dx.double() - dx_ref).abs().max().item()
    print(f'upconv3d_dgrad {case}: max abs err {err:.4g}, '
          f'atol {_dx_atol(case):.4g}')
    torch.testing.assert_close(dx.double(), dx_ref, rtol=5e-2,
                               atol=_dx_atol(case))


@pytest.mark.parametrize('case', CASES)
def test_upconv3d_wgrad(case):
    x, w, _, go, (_, dw_ref, _) = _problem(case)
    dw = C.upconv3d_wgrad(x, go)
    assert dw.shape == w.shape and dw.dtype == torch.float32
    err = (dw.double() - dw_ref).abs().max().item()
    print(f'upconv3d_wgrad {case}: max abs err {err:.4g}, '
          f'atol {_dw_atol(case):.4g}')
    torch.testing.assert_close(dw.double(), dw_ref, rtol=5e-2,
                               atol=_dw_atol(case))


def test_upsample2_conv3d_collapsed_backward():
    case = CASES[0]
    x, w, bias, go, (dx_ref, dw_ref, db_ref) = _problem(case)
    assert opsconv.route_upconv3d_bwd(case[1], case[2], case[4],
                                      case[5]) == 'collapsed'
    xg, wg, bg = (t.clone().requires_grad_(True) for t in (x, w, bias))
    opsconv.upsample2_conv3d(xg, wg, bg).backward(go)
    for name, got, ref, atol in (
            ('dx', xg.grad, dx_ref, _dx_atol(case)),
            ('dw', wg.grad, dw_ref, _dw_atol(case)),
            # a sum of M bf16-rounded unit normals, rounded once to bf16
            ('dbias', bg.grad, db_ref, _dw_atol(case))):
        err = (got.double() - ref).abs().max().item()
        print(f'upsample2_conv3d collapsed bwd {name}: max abs err {err:.4g},'
              f' atol {atol:.4g}')
        torch.testing.assert_close(got.double(), ref, rtol=5e-2, atol=atol)
