"""Depth-blocked one-pass stride-2 conv3d dgrad for 8-wide sub-grid planes
(the <OWT 8, DT 2> instance: a block owns the whole 8 x 8 sub-plane at two
sub-grid depths) and the native dispatch that sends such shapes from
conv3d_dgrad onto it, vs torch fp32 on the same bf16-rounded inputs.

Shapes are dx shapes (N, Cin, Cout, D, H, W). Reference and tolerance are
those of tests/test_gpu_dgrad_s2_onepass.py.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    C = ops.require_native()

DEV = 'cuda:0'
SENTINEL = -24576.0  # exact in bf16, far outside any dx of these problems


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


def _poison(shape):
    """Fill a dx-sized block with the sentinel and hand it back to the
    caching allocator, so the kernel's torch::empty output starts from it."""
    junk = torch.full(shape, SENTINEL, device=DEV, dtype=torch.bfloat16)
    torch.cuda.synchronize()
    del junk


def _run_poisoned(fn, shape):
    _poison(shape)
    dx = fn()
    assert list(dx.shape) == shape and dx.dtype == torch.bfloat16
    assert torch.isfinite(dx).all().item(), 'non-finite dx element'
    assert not (dx == SENTINEL).any().item(), 'unwritten dx element'
    return dx


CASES = [
    # one depth pair, both planes live, packed stores, batch stride
    (2, 32, 32, 4, 16, 16),
    # ragged ci column tile, ragged second co tile, Dq = 3: the last block's
    # second plane is past the end
    (1, 40, 48, 6, 16, 16),
    # odd D/H/W: the odd classes one shorter, scalar stores, go rows of 8
    (1, 32, 32, 5, 15, 15),
    # Hq = 6 < 8, Dq = 1 (only plane 0 of the pair exists), two co tiles
    (1, 32, 64, 2, 12, 16),
]


@pytest.mark.parametrize('case', CASES)
def test_dgrad_s2_smallplane(case):
    N, Cin, Cout, D, H, W = case
    go, w, shape, ref = _problem(*case)
    direct = _run_poisoned(lambda: C.conv3d_dgrad_s2_spatial(go, w, shape),
                           shape)
    routed = _run_poisoned(lambda: C.conv3d_dgrad(go, w, shape, 2), shape)
    for name, dx in (('direct', direct), ('routed', routed)):
        err = (dx.float() - ref).abs().max().item()
        print(f'dgrad_s2 smallplane {name} {case}: max abs err {err:.4g}, '
              f'ref max {ref.abs().max().item():.4g}')
    torch.testing.assert_close(direct.float(), ref, **_tol(Cout))
    torch.testing.assert_close(routed.float(), ref, **_tol(Cout))
    # same kernel, no atomics: the native dispatch took the one-pass kernel
    assert torch.equal(direct, routed)


def test_dgrad_s2_below_channel_floor_stays_igemm():
    case = (1, 32, 16, 4, 16, 16)   # Cout 16 < 32
    go, w, shape, ref = _problem(*case)
    dx = _run_poisoned(lambda: C.conv3d_dgrad(go, w, shape, 2), shape)
    err = (dx.float() - ref).abs().max().item()
    print(f'dgrad_s2 igemm {case}: max abs err {err:.4g}, '
          f'ref max {ref.abs().max().item():.4g}')
    torch.testing.assert_close(dx.float(), ref, **_tol(case[2]))
