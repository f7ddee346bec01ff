"""Wide-column (64 / 128) stride-2 chunk-128 instances of
conv3d_spatial_kernel in the plain, fused and fused-stats forms vs torch
fp32 conv3d on the same bf16-rounded inputs. Tolerances are those of
tests/test_gpu_conv3d.py (outputs) and tests/test_gpu_fusebn.py (epilogue
statistics).
"""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    C = ops.require_native()

DEV = 'cuda:0'


def _tol(k_channels):
    return dict(rtol=5e-2, atol=5e-2 * (k_channels * 27) ** 0.5 * 0.2)


def _seed(*key):
    return int.from_bytes(repr(key).encode(), 'little') % (2 ** 31)


@functools.lru_cache(maxsize=None)
def _problem(N, Cin, Cout, D, H, W, stride, fused):
    """(x, w, ab, ref): ref is torch fp32 on what the kernel's MFMAs see —
    bf16 x (through the bf16-rounded BN+ReLU when fused) and bf16 w."""
    g = torch.Generator(device='cpu').manual_seed(
        _seed('s2wide', N, Cin, Cout, D, H, W, stride))
    x = torch.randn(N, Cin, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    ab = None
    z = x.float()
    if fused:
        a = torch.rand(Cin, generator=g) + 0.5
        b = torch.randn(Cin, generator=g) * 0.1
        ab = torch.stack([a, b], 1).to(DEV).contiguous()
        z = torch.relu(x.float() * ab[:, 0].view(1, -1, 1, 1, 1)
                       + ab[:, 1].view(1, -1, 1, 1, 1))
        z = z.to(torch.bfloat16).float()
    ref = F.conv3d(z, w.float(), stride=stride, padding=1)
    return x, w, ab, ref


def _check_stats(out, stats):
    sums = stats.sum(0)
    o = out.float()
    torch.testing.assert_close(sums[:, 0], o.sum(dim=(0, 2, 3, 4)),
                               rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(sums[:, 1], (o * o).sum(dim=(0, 2, 3, 4)),
                               rtol=1e-3, atol=1e-1)


# (N, Cin, Cout, D, H, W, stride)
CASES = [
    # 64-column tile + ragged second tile, ragged channel tile, OWT 16
    (1, 24, 80, 5, 32, 32, 2),
    # 128-column tile + a ragged one
    (1, 24, 160, 3, 32, 32, 2),
    # OWT 32
    (1, 16, 64, 3, 16, 64, 2),
]


@pytest.mark.parametrize('mode', ['plain', 'fused', 'stats'])
@pytest.mark.parametrize('case', CASES)
def test_stride2_wide_fwd(case, mode):
    N, Cin, Cout, D, H, W, s = case
    x, w, ab, ref = _problem(N, Cin, Cout, D, H, W, s, mode != 'plain')
    if mode == 'plain':
        out = C.conv3d_fwd_spatial(x, w, s, 0)
    elif mode == 'fused':
        out = C.conv3d_fwd_spatial(x, w, s, 0, ab)
    else:
        out, stats = C.conv3d_fwd_spatial_stats(x, w, s, ab)
        _check_stats(out, stats)
    assert out.shape == ref.shape
    err = (out.float() - ref).abs().max().item()
    print(f's2 wide {case} {mode}: max abs err {err:.4g}')
    torch.testing.assert_close(out.float(), ref, **_tol(Cin))
