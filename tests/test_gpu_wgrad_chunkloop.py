"""Tap-reuse wgrad kernels over SEVERAL chunk-loop rounds per block.

The shapes make every z-block run the chunk loop three full rounds plus a
ragged last one (blocks-in-flight target 512 for 3D, 768 for 2D), so a
loop that carries state from chunk to chunk (register accumulators, a
staged prefetch) executes its prologue, steady state and drain. Reference:
torch fp32 conv weight gradients on the same bf16-rounded inputs.
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
SLICED_S1 = (2, 64, 64, 100, 16, 16, 1)     # 4 tiles, z 128, 400 chunks
SLICED_PARTIAL_C = (2, 48, 80, 100, 16, 16, 1)   # partial ci and co tiles
ATOMIC_CHUNK64 = (2, 128, 160, 40, 8, 8, 1)  # 20 tiles, z 25, 80 chunks
STRIDE2 = (2, 32, 64, 64, 32, 32, 2)
PARTIAL_ROWS = (2, 64, 64, 100, 12, 16, 1)  # OH=12 vs row tile 8: zero fill
# several column tiles per row, so the left/right halo columns of a slab
# come from neighbouring tiles (1 tile, z 512; 800 and 600 chunks)
WTILES_32 = (1, 32, 32, 200, 8, 64, 1)
WTILES_16 = (1, 32, 32, 200, 8, 48, 1)


@functools.lru_cache(maxsize=None)
def _case3d(case, fused):
    """(x bf16, go bf16, ab or None, fp32 reference dw), computed once."""
    N, Cin, Cout, D, H, W, s = case
    torch.manual_seed(3)
    x = (torch.randn(N, Cin, D, H, W, device=DEV) * 0.3).to(torch.bfloat16)
    OD, OH, OW = [(d + 2 - 3) // s + 1 for d in (D, H, W)]
    go = (torch.randn(N, Cout, OD, OH, OW, device=DEV) * 0.1).to(
        torch.bfloat16)
    ab = None
    xr = x.float()
    if fused:
        ab = torch.stack([torch.rand(Cin, device=DEV) + 0.5,
                          torch.randn(Cin, device=DEV) * 0.1], 1).contiguous()
        a = ab[:, 0].view(1, Cin, 1, 1, 1)
        b = ab[:, 1].view(1, Cin, 1, 1, 1)
        xr = torch.relu(a * xr + b).to(torch.bfloat16).float()
    w0 = torch.zeros(Cout, Cin, 3, 3, 3, device=DEV, requires_grad=True)
    F.conv3d(xr, w0, stride=s, padding=1).backward(go.float())
    return x, go, ab, w0.grad.detach()


def _check3d(case, fused=False):
    N, Cin, Cout, D, H, W, s = case
    x, go, ab, ref = _case3d(case, fused)
    dw = C.conv3d_wgrad(x, go, s, 0, ab) if fused else \
        C.conv3d_wgrad(x, go, s)
    M = go.numel() // Cout
    atol = 3e-2 * M ** 0.5 * 0.03
    print(f'case={case} fused={fused} max|err|='
          f'{(dw.float() - ref).abs().max().item():.4g} atol={atol:.4g} '
          f'max|ref|={ref.abs().max().item():.4g}')
    torch.testing.assert_close(dw.float(), ref, rtol=5e-2, atol=atol)
    return dw


@pytest.mark.parametrize('case', [SLICED_S1, SLICED_PARTIAL_C,
                                  ATOMIC_CHUNK64, STRIDE2, PARTIAL_ROWS,
                                  WTILES_32, WTILES_16])
def test_wgrad3d_multi_round(case):
    _check3d(case)


@pytest.mark.parametrize('case', [SLICED_S1, STRIDE2, WTILES_32])
def test_wgrad3d_multi_round_fused_bn(case):
    """relu(a*x+b) applied on load; reference applies it in fp32 and rounds
    to bf16 before the conv."""
    _check3d(case, fused=True)


def test_wgrad3d_sliced_is_deterministic():
    """The sliced fold has no atomics: two calls agree bitwise."""
    x, go, _, _ = _case3d(SLICED_S1, False)
    a = C.conv3d_wgrad(x, go, 1)
    b = C.conv3d_wgrad(x, go, 1)
    assert torch.equal(a, b)


# 2D: blocks-in-flight target 768, sliced from z-stride 16.
# stride 1: 4 tiles -> z 192; 300 images x 2 chunks = 600 = 3 * 192 + 24
# stride 2: 8 tiles -> z 96;  160 images x 2 chunks = 320 = 3 * 96 + 32
@pytest.mark.parametrize('case', [(300, 64, 64, 16, 16, 1),
                                  (160, 64, 128, 32, 32, 2)])
def test_wgrad2d_multi_round(case):
    N, Ci, Co, H, W, s = case
    torch.manual_seed(62)
    x = torch.randn(N, Ci, H, W, device=DEV, dtype=torch.bfloat16)
    OH, OW = (H + 2 - 3) // s + 1, (W + 2 - 3) // s + 1
    go = torch.randn(N, Co, OH, OW, device=DEV, dtype=torch.bfloat16) * 0.1
    go[0, 0, 0, min(3, OW - 1)] += 1.5
    gw = C.conv2d_wgrad(x, go, s)
    wr = torch.zeros(Co, Ci, 3, 3, device=DEV, requires_grad=True)
    F.conv2d(x.float(), wr, stride=s, padding=1).backward(go.float())
    m = (N * OH * OW) ** 0.5
    atol = 5e-2 * m * 0.1 + 0.2
    print(f'case={case} max|err|='
          f'{(gw.view_as(wr) - wr.grad).abs().max().item():.4g} '
          f'atol={atol:.4g}')
    torch.testing.assert_close(gw.view_as(wr), wr.grad, rtol=5e-2, atol=atol)
