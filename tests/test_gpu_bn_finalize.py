"""One-launch BN finalize (C.bn_finalize): epilogue partials [64][C][2] ->
mean, biased var, (mean, rstd), the normalize-on-load affine (a, b) and the
in-place running-stat update.

Reference: a float64 evaluation of the same formulas from the same fp32
partials. Tolerance: the composed torch chain the op replaces (stats.sum(0),
bn_stats_of's arithmetic, update_running_stats, the ab lines) runs on the
same inputs; per output the op's max error against float64 may be at most
twice the composed chain's, plus one fp32 ulp of the reference magnitude.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from coinstac_dinunet_amd import ops
    from coinstac_dinunet_amd.ops.bnorm import (OpsBatchNorm3d,
                                                update_running_stats)
    from coinstac_dinunet_amd.ops.conv import (OpsConv3d, bn_stats_of,
                                               conv_bn3d)
    C = ops.require_native()

DEV = 'cuda:0'
EPS = 1e-5
SHAPE = (2, 4, 8, 8)          # N, D, H, W of the 2 x C x 4 x 8 x 8 tensor
PER_CH = 2 * 4 * 8 * 8
ULP32 = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _inputs(ch):
    """Seeded (stats[64][C][2], gamma, beta, running_mean, running_var) on
    the GPU; the partials are fp32 sums and sums of squares of bf16
    activations dealt round-robin to the 64 slices."""
    g = torch.Generator(device='cpu').manual_seed(1000 + ch)
    # pre-BN conv outputs: channel means within two standard deviations of
    # zero, so E[x^2] / var <= 5. A channel with var << mean^2 (first tried:
    # sd 0.05 at |mean| ~ 1) turns ONE fp32 rounding of the folded sum of
    # squares (1 ulp of 513 is 6e-5, 1.2e-7 in var, 5e-4 in rstd = 20) into
    # the whole error of either path, and the 2x comparison then compares
    # two single roundings, whichever code made them.
    sd = torch.rand(ch, generator=g) * 2.75 + 0.25
    mu = (torch.rand(ch, generator=g) * 4.0 - 2.0) * sd
    x = torch.randn(PER_CH, ch, generator=g) * sd + mu
    x = x.to(torch.bfloat16).float()
    xs = x.view(PER_CH // 64, 64, ch)
    stats = torch.stack([xs.sum(0), (xs * xs).sum(0)], 2)   # [64][C][2]
    gamma = torch.rand(ch, generator=g) + 0.5
    beta = torch.randn(ch, generator=g) * 0.3
    rmean = torch.randn(ch, generator=g) * 0.5
    rvar = torch.rand(ch, generator=g) + 0.5
    return tuple(t.to(DEV).contiguous()
                 for t in (stats, gamma, beta, rmean, rvar))


def _reference(stats, gamma, beta, rmean, rvar, factor):
    s = stats.double().sum(0)
    mean = s[:, 0] / PER_CH
    var = (s[:, 1] / PER_CH - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + EPS)
    a = gamma.double() * rstd
    b = beta.double() - mean * a
    unbiased = var * (PER_CH / (PER_CH - 1))
    return dict(mean=mean, var=var, rstd=rstd, a=a, b=b,
                running_mean=rmean.double() * (1 - factor) + factor * mean,
                running_var=rvar.double() * (1 - factor) + factor * unbiased)


def _composed(stats, gamma, beta, rmean, rvar, factor):
    """The torch chain of the parent, kernel for kernel."""
    xb = torch.empty(SHAPE[0], stats.size(1), *SHAPE[1:], device=DEV,
                     dtype=torch.bfloat16)
    xb._coinn_bn_stats = stats
    mean, var, mean_rstd = bn_stats_of(xb, EPS)
    rmean, rvar = rmean.clone(), rvar.clone()
    update_running_stats(rmean, rvar, mean, var, PER_CH, factor)
    a = gamma.float() * mean_rstd[:, 1]
    b = beta.float() - mean_rstd[:, 0] * a
    return dict(mean=mean, var=var, rstd=mean_rstd[:, 1], a=a, b=b,
                running_mean=rmean, running_var=rvar)


def _native(stats, gamma, beta, rmean, rvar, factor):
    rmean, rvar = rmean.clone(), rvar.clone()
    mean, var, mean_rstd, ab = C.bn_finalize(stats, PER_CH, EPS, gamma, beta,
                                             rmean, rvar, factor)
    assert torch.equal(mean_rstd[:, 0], mean)
    return dict(mean=mean, var=var, rstd=mean_rstd[:, 1], a=ab[:, 0],
                b=ab[:, 1], running_mean=rmean, running_var=rvar)


@pytest.mark.parametrize('factor', [0.1, 0.5])
@pytest.mark.parametrize('ch', [32, 40, 256])
def test_bn_finalize_vs_float64(ch, factor):
    inp = _inputs(ch)
    ref = _reference(*inp, factor)
    old = _composed(*inp, factor)
    new = _native(*inp, factor)
    bad = []
    for key, r in ref.items():
        e_old = (old[key].double() - r).abs().max().item()
        e_new = (new[key].double() - r).abs().max().item()
        bound = 2 * e_old + ULP32 * r.abs().max().item()
        print(f'bn_finalize C={ch} f={factor} {key}: new {e_new:.3g} '
              f'composed {e_old:.3g} bound {bound:.3g}')
        if not e_new <= bound:
            bad.append((key, e_new, e_old, bound))
    assert not bad, bad


def test_bn_finalize_without_buffers_writes_nothing():
    stats, gamma, beta, rmean, rvar = _inputs(40)
    keep = [t.clone() for t in (stats, gamma, beta, rmean, rvar)]
    with_buf = _native(stats, gamma, beta, rmean, rvar, 0.1)
    mean, var, mean_rstd, ab = C.bn_finalize(stats, PER_CH, EPS, gamma, beta)
    torch.cuda.synchronize()
    for t, k in zip((stats, gamma, beta, rmean, rvar), keep):
        assert torch.equal(t, k)
    # the batch outputs do not depend on the buffers
    assert torch.equal(mean, with_buf['mean'])
    assert torch.equal(var, with_buf['var'])
    assert torch.equal(mean_rstd[:, 1], with_buf['rstd'])
    assert torch.equal(ab[:, 0], with_buf['a'])
    assert torch.equal(ab[:, 1], with_buf['b'])


def test_conv_bn3d_with_finalize_is_capturable():
    torch.manual_seed(7)
    conv0 = OpsConv3d(4, 16, 3, padding=1, bias=False).to(DEV)
    bn0 = OpsBatchNorm3d(16, relu=True).to(DEV)
    conv1 = OpsConv3d(16, 32, 3, padding=1, bias=False).to(DEV)
    bn1 = OpsBatchNorm3d(32, relu=True).to(DEV)
    conv2 = OpsConv3d(32, 32, 3, padding=1, bias=False).to(DEV)
    x = torch.randn(2, 4, 8, 8, 8, device=DEV)
    used = []

    def run():
        with torch.autocast('cuda', dtype=torch.bfloat16):
            x1 = conv_bn3d(conv0(x), bn0, conv1)
            # x1 carries epilogue partials: this call runs the finalize op
            used.append(getattr(x1, '_coinn_bn_stats', None) is not None)
            return conv_bn3d(x1, bn1, conv2)

    for _ in range(2):
        eager = run().detach().clone()
    assert all(used)
    g = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        out = run()
    g.replay()
    torch.cuda.synchronize()
    assert torch.isfinite(out).all().item()
    # same inputs and batch statistics; the conv epilogue accumulates its
    # partials with fp32 atomics, so the last bit of (a, b) and with it a
    # bf16 rounding of the output may differ between two runs: the bound of
    # tests/test_gpu_graph.py
    torch.testing.assert_close(out.detach().float(), eager.float(),
                               rtol=2e-2, atol=2e-2)
