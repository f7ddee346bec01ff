"""CPU tests for the shape-only pieces of ops.conv / ops.bnorm: the 3D
kernel routing functions and the running-statistics helper."""
import itertools

import pytest
import torch

from coinstac_dinunet_amd.ops.bnorm import (bn_momentum_step,
                                            update_running_stats)
from coinstac_dinunet_amd.ops.conv import (route_dgrad3d, route_fused_fwd3d,
                                           route_fwd3d)


# ---- oracles: the inline conditions the autograd functions carried before
# ---- the routing moved into functions, transcribed literally --------------

def _inline_fwd(cin, H, W, stride):
    ow = (W + 2 - 3) // stride + 1
    oh = (H + 2 - 3) // stride + 1
    min_chunk = 64
    ci_ok = cin >= 16 or stride == 1
    if ow % 8 == 0 and ci_ok and oh * ow >= min_chunk:
        return 'spatial-ctile1' if cin < 16 else 'spatial'
    return 'igemm'


def _inline_fused_fwd(cin, H, W, stride):
    ow = (W + 2 - 3) // stride + 1
    oh = (H + 2 - 3) // stride + 1
    if ow % 8 == 0 and cin >= 16 and oh * ow >= 64:
        return 'spatial'
    return 'igemm'


def _inline_dgrad(cout, H, W, stride):
    wsub = (W + 1) // 2
    hsub = (H + 1) // 2
    if stride == 1 and W % 8 == 0 and cout >= 16 and H * W >= 64:
        return 'spatial'
    if stride == 2 and wsub % 8 == 0 and cout >= 32 and hsub * wsub >= 128:
        return 's2-spatial'
    return 'igemm'


FWD_ROWS = [
    ((16, 8, 8, 1), 'spatial'),
    ((16, 7, 8, 1), 'igemm'),
    ((15, 8, 8, 1), 'spatial-ctile1'),
    ((15, 16, 16, 2), 'igemm'),
    ((16, 16, 16, 2), 'spatial'),
    ((32, 16, 12, 1), 'igemm'),
]
FUSED_ROWS = [
    ((15, 8, 8, 1), 'igemm'),
    ((16, 8, 8, 1), 'spatial'),
]
DGRAD_ROWS = [
    ((16, 8, 8, 1), 'spatial'),
    ((15, 8, 8, 1), 'igemm'),
    ((16, 4, 8, 1), 'igemm'),
    ((32, 16, 16, 2), 'igemm'),
    ((32, 32, 16, 2), 's2-spatial'),
    ((31, 32, 16, 2), 'igemm'),
    ((32, 32, 15, 2), 's2-spatial'),
]


@pytest.mark.parametrize('args,want', FWD_ROWS)
def test_route_fwd3d_pinned(args, want):
    assert _inline_fwd(*args) == want
    assert route_fwd3d(*args) == want


@pytest.mark.parametrize('args,want', FUSED_ROWS)
def test_route_fused_fwd3d_pinned(args, want):
    assert _inline_fused_fwd(*args) == want
    assert route_fused_fwd3d(*args) == want


@pytest.mark.parametrize('args,want', DGRAD_ROWS)
def test_route_dgrad3d_pinned(args, want):
    assert _inline_dgrad(*args) == want
    assert route_dgrad3d(*args) == want


# The flagship: VBMNet at 64^3, widths (32, 64, 128, 256). Per layer
# (cin, cout, input side, stride) -> (forward, dgrad). The first conv runs
# the plain forward, the other seven the fused (normalize-on-load) one.
VBM_LAYERS = [
    ((1, 32, 64, 1), ('spatial-ctile1', 'spatial')),
    ((32, 32, 64, 1), ('spatial', 'spatial')),
    ((32, 64, 64, 2), ('spatial', 's2-spatial')),
    ((64, 64, 32, 1), ('spatial', 'spatial')),
    ((64, 128, 32, 2), ('spatial', 's2-spatial')),
    ((128, 128, 16, 1), ('spatial', 'spatial')),
    ((128, 256, 16, 2), ('spatial', 'igemm')),
    ((256, 256, 8, 1), ('spatial', 'spatial')),
]


@pytest.mark.parametrize('i', range(len(VBM_LAYERS)))
def test_routes_of_the_vbm_flagship_layers(i):
    (cin, cout, side, stride), (want_fwd, want_dgrad) = VBM_LAYERS[i]
    inline_fwd, fwd = ((_inline_fwd, route_fwd3d) if i == 0
                       else (_inline_fused_fwd, route_fused_fwd3d))
    assert inline_fwd(cin, side, side, stride) == want_fwd
    assert fwd(cin, side, side, stride) == want_fwd
    assert _inline_dgrad(cout, side, side, stride) == want_dgrad
    assert route_dgrad3d(cout, side, side, stride) == want_dgrad


def test_routes_agree_with_inline_conditions_on_a_shape_sweep():
    chans = (1, 4, 15, 16, 17, 31, 32, 33, 64)
    sides = (3, 4, 7, 8, 9, 12, 15, 16, 17, 24, 31, 32, 33, 64)
    for c, h, w, s in itertools.product(chans, sides, sides, (1, 2)):
        assert route_fwd3d(c, h, w, s) == _inline_fwd(c, h, w, s), (c, h, w, s)
        assert route_fused_fwd3d(c, h, w, s) == _inline_fused_fwd(c, h, w, s)
        assert route_dgrad3d(c, h, w, s) == _inline_dgrad(c, h, w, s), \
            (c, h, w, s)


# ---- running statistics ---------------------------------------------------

@pytest.mark.parametrize('momentum', [0.1, None])
def test_running_stat_helper_matches_batchnorm3d(momentum):
    torch.manual_seed(0)
    ref = torch.nn.BatchNorm3d(3, momentum=momentum).train()
    mine = torch.nn.BatchNorm3d(3, momentum=momentum).train()  # buffers only
    for _ in range(3):
        x = torch.randn(4, 3, 5, 5, 5) * 1.5 + 0.3
        ref(x)
        mean = x.mean(dim=(0, 2, 3, 4))
        var = x.var(dim=(0, 2, 3, 4), unbiased=False)
        update_running_stats(mine.running_mean, mine.running_var, mean, var,
                             x.numel() // x.size(1), bn_momentum_step(mine))
    torch.testing.assert_close(mine.running_mean, ref.running_mean)
    torch.testing.assert_close(mine.running_var, ref.running_var)
    assert int(mine.num_batches_tracked) == int(ref.num_batches_tracked) == 3


def test_running_stat_helper_without_tracking_touches_nothing():
    bn = torch.nn.BatchNorm3d(3, track_running_stats=False).train()
    assert bn.running_mean is None and bn.num_batches_tracked is None
    x = torch.randn(4, 3, 5, 5, 5)
    factor = bn_momentum_step(bn)
    assert factor is None
    update_running_stats(bn.running_mean, bn.running_var,
                         x.mean(dim=(0, 2, 3, 4)),
                         x.var(dim=(0, 2, 3, 4), unbiased=False),
                         x.numel() // x.size(1), factor)
    assert bn.running_mean is None and bn.running_var is None \
        and bn.num_batches_tracked is None
