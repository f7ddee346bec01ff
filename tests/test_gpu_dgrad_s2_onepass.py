"""One-pass parity stride-2 conv3d dgrad (all 8 parity classes from one
staged go slab, 16-byte LDS operand reads, 16-byte dx stores, one-launch
weight prep) vs torch fp32 on the same bf16-rounded inputs.

Shapes are dx shapes (N, Cin, Cout, D, H, W); go is the stride-2, pad-1
output grid ((D+1)//2, (H+1)//2, (W+1)//2). Tolerances are those of
tests/test_gpu_conv3d.py.
"""
import functools

import pytest
import torch

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
def _problem(N, Cin, Cout, D, H, W):
    """(go, w, in_shape, ref): ref is torch's fp32 input gradient of the
    stride-2 conv on the bf16-rounded go and w."""
    g = torch.Generator(device='cpu').manual_seed(
        _seed('dgrad_s2', N, Cin, Cout, D, H, W))
    od, oh, ow = (D + 1) // 2, (H + 1) // 2, (W + 1) // 2
    go = torch.randn(N, Cout, od, oh, ow, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    shape = [N, Cin, D, H, W]
    ref = torch.nn.grad.conv3d_input(shape, w.float(), go.float(), stride=2,
                                     padding=1)
    return go, w, shape, ref


CASES = [
    # OWT 32, two h-tiles, packed stores
    (1, 32, 32, 4, 16, 64),
    # ragged ci column tile, ragged second co tile, odd D (the a classes
    # have different depths), ragged h-tile at OWT 16
    (2, 24, 48, 5, 18, 32),
    # odd H and W: scalar stores, the c = 1 class one column narrower
    (1, 40, 32, 3, 15, 15),
    # L5 class: 4 co tiles, 2 column tiles
    (1, 64, 128, 4, 32, 32),
    # D = 2: the second depth plane of the last id' is past the go extent;
    # go rows of 9 elements are ragged and not 16-byte aligned
    (2, 32, 32, 2, 12, 18),
]


@pytest.mark.parametrize('case', CASES)
def test_dgrad_s2_onepass(case):
    N, Cin, Cout, D, H, W = case
    go, w, shape, ref = _problem(*case)
    dx = C.conv3d_dgrad_s2_spatial(go, w, shape)
    assert list(dx.shape) == shape and dx.dtype == torch.bfloat16
    err = (dx.float() - ref).abs().max().item()
    print(f'dgrad_s2 {case}: max abs err {err:.4g}, '
          f'ref max {ref.abs().max().item():.4g}')
    torch.testing.assert_close(dx.float(), ref, **_tol(Cout))
