"""Channel-innermost spatial conv3d kernels (16-byte A reads, packed stores,
one-launch weight prep) vs torch fp32 conv3d on the same bf16-rounded inputs.

The shapes are the smallest that reach each instance of
conv3d_spatial_kernel with ragged edges: a ragged channel tile, a ragged
h- or w-tile, a ragged column tile, more than one block. Every fused
chunk-256 forward and every dgrad here has at most 32 output-side channels,
which keeps them clear of the under-covered column grid (docs/NEXT.md).
Tolerances are those of tests/test_gpu_conv3d.py (outputs) and
tests/test_gpu_fusebn.py (epilogue statistics).
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
def _fwd_problem(N, Cin, Cout, D, H, W, stride, fused):
    """(x, w, ab, ref): ref is torch fp32 on what the kernel's MFMAs see —
    bf16 x (through the bf16-rounded BN+ReLU when fused) and bf16 w."""
    g = torch.Generator(device='cpu').manual_seed(
        _seed('fwd', N, Cin, Cout, D, H, W, stride))
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


@functools.lru_cache(maxsize=None)
def _dgrad_problem(N, Cin, Cout, D, H, W):
    """(go, w, in_shape, ref) for the stride-1 input gradient."""
    g = torch.Generator(device='cpu').manual_seed(
        _seed('dgrad', N, Cin, Cout, D, H, W))
    go = torch.randn(N, Cout, D, H, W, generator=g).to(DEV, torch.bfloat16)
    w = (torch.randn(Cout, Cin, 3, 3, 3, generator=g) * 0.2).to(
        DEV, torch.bfloat16)
    ref = F.conv_transpose3d(go.float(), w.float(), stride=1, padding=1)
    return go, w, [N, Cin, D, H, W], ref


def _check_stats(out, stats):
    sums = stats.sum(0)
    o = out.float()
    torch.testing.assert_close(sums[:, 0], o.sum(dim=(0, 2, 3, 4)),
                               rtol=1e-3, atol=1e-1)
    torch.testing.assert_close(sums[:, 1], (o * o).sum(dim=(0, 2, 3, 4)),
                               rtol=1e-3, atol=1e-1)


def _run_fwd(case, mode):
    N, Cin, Cout, D, H, W, s = case
    x, w, ab, ref = _fwd_problem(N, Cin, Cout, D, H, W, s, mode != 'plain')
    if mode == 'plain':
        out = C.conv3d_fwd_spatial(x, w, s, 0)
    elif mode == 'fused':
        out = C.conv3d_fwd_spatial(x, w, s, 0, ab)
    else:
        out, stats = C.conv3d_fwd_spatial_stats(x, w, s, ab)
        _check_stats(out, stats)
    assert out.shape == ref.shape
    torch.testing.assert_close(out.float(), ref, **_tol(Cin))


# (N, Cin, Cout, D, H, W, stride)
CHUNK512 = (1, 24, 24, 3, 24, 32, 1)   # CTILE 16 x 2 (ragged), ragged h-tile
CHUNK256 = (2, 48, 32, 3, 16, 16, 1)   # CTILE 32 + ragged 16
CHUNK256_WIDE = (2, 48, 80, 3, 16, 16, 1)  # 64-column instance, ragged tile
CHUNK64 = [(2, 48, co, 3, 8, 8, 1) for co in (32, 64, 128)]
STRIDE2 = [(1, 24, 48, 5, 32, 32, 2),  # chunk 128, OWT 16
           (1, 24, 48, 5, 16, 16, 2)]  # chunk 64, OWT 8


def test_chunk512_fused_stats_fwd():
    _run_fwd(CHUNK512, 'stats')


def test_chunk512_dgrad():
    N, Cin, Cout, D, H, W, _ = CHUNK512
    go, w, shape, ref = _dgrad_problem(N, Cin, Cout, D, H, W)
    dx = C.conv3d_dgrad_spatial(go, w, shape)
    torch.testing.assert_close(dx.float(), ref, **_tol(Cout))


@pytest.mark.parametrize('mode', ['plain', 'fused', 'stats'])
def test_chunk256_fwd(mode):
    _run_fwd(CHUNK256, mode)


def test_chunk256_wide_plain_fwd():
    _run_fwd(CHUNK256_WIDE, 'plain')


def test_chunk256_dgrad():
    # go channels 48 (K side), dx channels 32
    go, w, shape, ref = _dgrad_problem(2, 32, 48, 3, 16, 16)
    dx = C.conv3d_dgrad_spatial(go, w, shape)
    torch.testing.assert_close(dx.float(), ref, **_tol(48))


@pytest.mark.parametrize('mode', ['plain', 'fused', 'stats'])
@pytest.mark.parametrize('case', CHUNK64)
def test_chunk64_fwd(case, mode):
    _run_fwd(case, mode)


def test_chunk64_dgrad():
    go, w, shape, ref = _dgrad_problem(2, 32, 48, 3, 8, 8)
    dx = C.conv3d_dgrad_spatial(go, w, shape)
    torch.testing.assert_close(dx.float(), ref, **_tol(48))


@pytest.mark.parametrize('mode', ['plain', 'fused', 'stats'])
@pytest.mark.parametrize('case', STRIDE2)
def test_stride2_fwd(case, mode):
    _run_fwd(case, mode)


def test_packed_store_fallback_ragged_w_tile():
    """TW = 10 is no multiple of 4: the epilogue takes the scalar stores,
    the OWT=8 instance runs a ragged second w-tile, and the rows are not
    16-byte aligned, so staging takes its element-wise path."""
    _run_fwd((1, 16, 32, 3, 8, 10, 1), 'plain')
