"""Nearest-2x upsample + 3x3x3 conv on the HIP path (upconv3d.hip): the
collapsed 8-class forward kernel, the composed route, the backward through
fold2_sum3d / upsample2_nearest3d, and UNet3D's decoder using it, against
fp64 torch on the same bf16-rounded inputs.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.ops import conv as opsconv
    C = ops.require_native()

DEV = 'cuda:0'


def _problem(N, Cin, Cout, D, H, W):
    """bf16 (x, w, bias, go) on the GPU, seeded on the CPU, and the fp64
    reference function on them."""
    g = torch.Generator(device='cpu').manual_seed(
        hash((N, Cin, Cout, D, H, W)) % 2 ** 31)
    x = torch.randn(N, Cin, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    bias = torch.randn(Cout, generator=g).to(DEV, torch.bfloat16)
    go = torch.randn(N, Cout, 2 * D, 2 * H, 2 * W, generator=g).to(
        DEV, torch.bfloat16)

    def ref(x, w, bias=None):
        return F.conv3d(F.interpolate(x, scale_factor=2, mode='nearest'), w,
                        bias, padding=1)
    return x, w, bias, go, ref


# (N, Cin, Cout, D, H, W) of the low-res input
FWD_CASES = [
    (2, 48, 40, 3, 16, 16),   # ragged ci tile, ragged co tile, odd D, N > 1
    (1, 32, 32, 1, 8, 8),     # D = 1: both depth halos; the 8x8 instance
    (2, 16, 160, 5, 8, 8),    # 8x8: ragged depth group, several co tiles
    (1, 64, 32, 2, 12, 16),   # H no multiple of the row tile; two ci tiles
    (1, 32, 16, 2, 16, 24),   # W a multiple of 8, not of the widest tile
]


@pytest.mark.parametrize('case', FWD_CASES)
def test_upconv3d_fwd(case):
    x, w, _, _, ref_fn = _problem(*case)
    ref = ref_fn(x.double(), w.double())
    out = C.upconv3d_fwd(x, w)
    assert out.shape == ref.shape and out.dtype == torch.bfloat16
    atol = 5e-2 * (case[1] * 27) ** 0.5 * 0.2
    err = (out.double() - ref).abs().max().item()
    print(f'upconv3d_fwd {case}: max abs err {err:.4g}, atol {atol:.4g}')
    torch.testing.assert_close(out.double(), ref, rtol=5e-2, atol=atol)


def test_upsample2_conv3d_composed_with_bias():
    case = (1, 8, 16, 2, 5, 6)
    assert opsconv.route_upconv3d(case[1], case[4], case[5]) == 'composed'
    x, w, bias, _, ref_fn = _problem(*case)
    ref = ref_fn(x.double(), w.double(), bias.double())
    out = opsconv.upsample2_conv3d(x, w, bias)
    err = (out.double() - ref).abs().max().item()
    print(f'upsample2_conv3d composed {case}: max abs err {err:.4g}')
    torch.testing.assert_close(out.double(), ref, rtol=5e-2,
                               atol=5e-2 * (case[1] * 27) ** 0.5 * 0.2)


@pytest.mark.parametrize('case', [(2, 32, 48, 3, 8, 8),
                                  (1, 48, 32, 2, 16, 16)])
def test_upsample2_conv3d_backward(case):
    N, Cin, Cout, D, H, W = case
    x, w, _, go, ref_fn = _problem(*case)
    xr = x.double().requires_grad_(True)
    wr = w.double().requires_grad_(True)
    ref_fn(xr, wr).backward(go.double())

    xg = x.clone().requires_grad_(True)
    wg = w.clone().requires_grad_(True)
    out = opsconv.upsample2_conv3d(xg, wg)
    up_numel = x.numel() * 8
    saved = out.grad_fn.saved_tensors
    assert saved and all(t.numel() < up_numel for t in saved)
    out.backward(go)

    M = N * 8 * D * H * W
    dx_err = (xg.grad.double() - xr.grad).abs().max().item()
    dw_err = (wg.grad.double() - wr.grad).abs().max().item()
    print(f'upsample2_conv3d bwd {case}: dx err {dx_err:.4g}, '
          f'dw err {dw_err:.4g}')
    torch.testing.assert_close(
        xg.grad.double(), xr.grad, rtol=5e-2,
        atol=5e-2 * (Cout * 27 * 8) ** 0.5 * 0.2)
    torch.testing.assert_close(wg.grad.double(), wr.grad, rtol=5e-2,
                               atol=3e-2 * M ** 0.5 * 0.03)


def test_unet_fused_upsample_matches_unfused(monkeypatch):
    """One training step (mean cross-entropy, the loss the model documents)
    with the decoder fused and unfused: logits and up_conv[0].weight.grad
    agree within test_unet_gpu_matches_cpu_reference's bound. That absolute
    bound says little about a mean-loss gradient, so the gradient is also
    held to a scale-free one taken from the unfused path's own error: both
    paths are bf16 roundings of the same fp64 model (train-mode BN on one
    sample amplifies either rounding alike), and the fused path may be at
    most twice as far from it in relative L2 as the unfused one is. The two
    gradients are also compared directly: two independent roundings, each e
    from the model, lie about sqrt(2) e apart, so their relative L2
    distance may be at most twice the unfused path's e. A wrong slot, fold
    or upsample puts either figure at order 1."""
    import copy
    from coinstac_dinunet_amd.models import unet
    torch.manual_seed(0)
    net = unet.UNet3D(in_channels=1, num_class=2, widths=(16, 32))
    ref_net = copy.deepcopy(net).double()
    net = net.to(DEV)
    g = torch.Generator(device='cpu').manual_seed(1616)
    x = torch.randn(1, 1, 16, 16, 16, generator=g)
    y = torch.randint(0, 2, (1, 16, 16, 16), generator=g)
    F.cross_entropy(ref_net(x.double()), y).backward()
    g_ref = ref_net.up_conv[0].weight.grad
    res = {}
    for flag in (True, False):
        monkeypatch.setattr(unet, '_FUSE_UPSAMPLE', flag)
        net.zero_grad(set_to_none=True)
        out = net(x.to(DEV))
        ops.cross_entropy(out.float(), y.to(DEV)).backward()
        res[flag] = (out.detach().float(),
                     net.up_conv[0].weight.grad.detach().float().clone())
    rel = {f: ((res[f][1].double().cpu() - g_ref).norm()
               / g_ref.norm()).item() for f in res}
    apart = ((res[True][1] - res[False][1]).norm()
             / res[False][1].norm()).item()
    print(f'unet up_conv[0] grad rel L2 err vs fp64: fused {rel[True]:.4g}, '
          f'unfused {rel[False]:.4g}; fused vs unfused {apart:.4g}; '
          f'|grad| max {g_ref.abs().max().item():.4g}')
    torch.testing.assert_close(res[True][0], res[False][0],
                               rtol=1e-1, atol=1e-1)
    torch.testing.assert_close(res[True][1], res[False][1],
                               rtol=1e-1, atol=1e-1)
    assert rel[True] <= 2 * rel[False]
    assert apart <= 2 * rel[False]
