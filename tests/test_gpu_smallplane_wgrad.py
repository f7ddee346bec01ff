"""Tap-reuse wgrad on whole-plane shapes (output planes of 8 columns and at
most 8 rows, where one chunk-64 tile is the plane and the slab halo is conv
padding), through the tap-major atomic fold and the sliced fold, vs torch
fp32 conv weight gradients on the same bf16-rounded inputs. Tolerance is
that of tests/test_gpu_wgrad_chunkloop.py.
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

# (N, Cin, Cout, D, H, W, stride)
# partial ci and co tiles, ragged depth group, atomic fold
PARTIAL_C = (2, 48, 80, 5, 8, 8, 1)
# one (co, ci) tile: z-stride >= 32 and the sliced fold
SLICED = (8, 32, 32, 16, 8, 8, 1)
# 4 tiles -> z 128; several chunk-loop rounds per block, ragged last round
MULTI_ROUND = (3, 64, 64, 40, 8, 8, 1)
# stride 2, OD = 5 (ragged group), ragged 16-channel ci tile
STRIDE2 = (2, 24, 80, 9, 16, 16, 2)
# OH = 6 < 8: go rows past the plane are zero
PARTIAL_ROWS = (2, 32, 64, 6, 6, 8, 1)
CASES = [PARTIAL_C, SLICED, MULTI_ROUND, STRIDE2, PARTIAL_ROWS]


@functools.lru_cache(maxsize=None)
def _case(case, fused, b_positive=False):
    """(x bf16, go bf16, ab or None, fp32 reference dw), computed once. With
    b_positive every channel has relu(b) > 0, so padding that went through
    the BN transform instead of staying zero shows in every border tap."""
    N, Cin, Cout, D, H, W, s = case
    torch.manual_seed(5)
    x = (torch.randn(N, Cin, D, H, W, device=DEV) * 0.3).to(torch.bfloat16)
    OD, OH, OW = [(d + 2 - 3) // s + 1 for d in (D, H, W)]
    go = (torch.randn(N, Cout, OD, OH, OW, device=DEV) * 0.1).to(
        torch.bfloat16)
    ab = None
    xr = x.float()
    if fused:
        b = torch.randn(Cin, device=DEV) * 0.1
        if b_positive:
            b = torch.rand(Cin, device=DEV) + 0.5
        ab = torch.stack([torch.rand(Cin, device=DEV) + 0.5, b],
                         1).contiguous()
        xr = torch.relu(ab[:, 0].view(1, Cin, 1, 1, 1) * xr
                        + ab[:, 1].view(1, Cin, 1, 1, 1))
        xr = xr.to(torch.bfloat16).float()
    w0 = torch.zeros(Cout, Cin, 3, 3, 3, device=DEV, requires_grad=True)
    F.conv3d(xr, w0, stride=s, padding=1).backward(go.float())
    return x, go, ab, w0.grad.detach()


def _check(case, fused=False, b_positive=False):
    N, Cin, Cout, D, H, W, s = case
    x, go, ab, ref = _case(case, fused, b_positive)
    dw = C.conv3d_wgrad(x, go, s, 0, ab) if fused else \
        C.conv3d_wgrad(x, go, s)
    M = go.numel() // Cout
    atol = 3e-2 * M ** 0.5 * 0.03
    print(f'smallplane wgrad case={case} fused={fused} b>0={b_positive} '
          f'max|err|={(dw.float() - ref).abs().max().item():.4g} '
          f'atol={atol:.4g} max|ref|={ref.abs().max().item():.4g}')
    torch.testing.assert_close(dw.float(), ref, rtol=5e-2, atol=atol)


@pytest.mark.parametrize('fused', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_smallplane_wgrad(case, fused):
    _check(case, fused)


@pytest.mark.parametrize('case', [PARTIAL_C, STRIDE2])
def test_smallplane_wgrad_zero_halo_under_bn(case):
    """b > 0 on every channel: the padding is zero after BN, not relu(b)."""
    _check(case, fused=True, b_positive=True)


def test_smallplane_wgrad_sliced_is_deterministic():
    """The sliced fold has no atomics: two calls agree bitwise."""
    x, go, _, _ = _case(SLICED, False)
    a = C.conv3d_wgrad(x, go, 1)
    b = C.conv3d_wgrad(x, go, 1)
    assert torch.equal(a, b)
