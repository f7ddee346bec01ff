"""Depth-blocked whole-plane instances of conv3d_spatial_kernel (output
planes of 8 columns and at most 8 rows: one tile is the plane, a block
covers several output depth planes) in the plain, fused and fused-stats
forms vs torch fp32 conv3d on the same bf16-rounded inputs. Tolerances are
those of tests/test_gpu_spatial_s2_wide.py.
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
def _problem(N, Cin, Cout, D, H, W, stride, fused, b_positive=False):
    """(x, w, ab, ref): ref is torch fp32 on what the kernel's MFMAs see —
    bf16 x (through the bf16-rounded BN+ReLU when fused) and bf16 w. With
    b_positive every channel has relu(b) > 0, so padding that went through
    the BN transform instead of staying zero shows in every border output."""
    g = torch.Generator(device='cpu').manual_seed(
        _seed('smallplane', N, Cin, Cout, D, H, W, stride))
    x = torch.randn(N, Cin, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    ab = None
    z = x.float()
    if fused:
        a = torch.rand(Cin, generator=g) + 0.5
        b = torch.randn(Cin, generator=g) * 0.1
        if b_positive:
            b = torch.rand(Cin, generator=g) + 0.5
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


def _run(case, mode, b_positive=False):
    N, Cin, Cout, D, H, W, s = case
    x, w, ab, ref = _problem(N, Cin, Cout, D, H, W, s, mode != 'plain',
                             b_positive)
    if mode == 'plain':
        out = C.conv3d_fwd_spatial(x, w, s, 0)
    elif mode == 'fused':
        out = C.conv3d_fwd_spatial(x, w, s, 0, ab)
    else:
        out, stats = C.conv3d_fwd_spatial_stats(x, w, s, ab)
        # rows and planes past the tensor must not be counted
        _check_stats(out, stats)
    assert out.shape == ref.shape
    err = (out.float() - ref).abs().max().item()
    print(f'smallplane fwd {case} {mode} b>0={b_positive}: '
          f'max abs err {err:.4g}')
    torch.testing.assert_close(out.float(), ref, **_tol(Cin))


# (N, Cin, Cout, D, H, W, stride)
CASES = [
    # ragged channel tile and column tile; D no multiple of 2 or 4 (ragged
    # last depth group); N > 1
    (2, 48, 160, 5, 8, 8, 1),
    # D = 1: both depth halos and an almost empty group
    (1, 32, 32, 1, 8, 8, 1),
    # TH < 8: rows past the plane are zero and unstored
    (2, 32, 64, 6, 6, 8, 1),
    # stride 2, OD = 5: ragged group, ragged 16-channel tile
    (2, 24, 160, 9, 16, 16, 2),
    # stride 2, OH = 6
    (1, 16, 64, 8, 12, 16, 2),
]


@pytest.mark.parametrize('mode', ['plain', 'fused', 'stats'])
@pytest.mark.parametrize('case', CASES)
def test_smallplane_fwd(case, mode):
    _run(case, mode)


@pytest.mark.parametrize('case', [CASES[2], CASES[3]])
def test_smallplane_fwd_zero_halo_under_bn(case):
    """b > 0 on every channel: the padding is zero after BN, not relu(b)."""
    _run(case, 'stats', b_positive=True)
