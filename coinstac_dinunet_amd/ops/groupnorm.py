"""GroupNorm / InstanceNorm with a fused (leaky) ReLU on the HIP kernels of
csrc/groupnorm.hip.

Per-sample normalization for federated training on non-IID sites: no batch
statistics and no running buffers. A group of one sample is one contiguous
run of the NC(S...) tensor, so one kernel family serves GroupNorm (G
groups), InstanceNorm (G == C) and the one-group case. The activation
z > 0 ? z : negative_slope * z folds into the normalize pass (0 is ReLU,
0.01 nnU-Net's LeakyReLU); the backward recomputes z from the saved input,
so no activation output or mask is kept.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native_available, require_native
from .bnorm import OpsBatchNorm3d


class _GroupNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, groups, eps, act, slope):
        C = require_native()
        xb = x.to(torch.bfloat16).contiguous()
        y, mean_rstd = C.gn_fwd(xb, gamma, beta, groups, eps, act, slope)
        ctx.save_for_backward(xb, mean_rstd, gamma, beta)
        ctx.groups, ctx.act, ctx.slope = groups, act, slope
        ctx.in_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        C = require_native()
        xb, mean_rstd, gamma, beta = ctx.saved_tensors
        dx, dgamma, dbeta = C.gn_bwd(
            dy.to(torch.bfloat16).contiguous(), xb, mean_rstd, gamma, beta,
            ctx.groups, ctx.act, ctx.slope)
        return (dx.to(ctx.in_dtype), dgamma.to(gamma.dtype),
                dbeta.to(beta.dtype), None, None, None, None)


def _check_act(relu, negative_slope):
    if negative_slope and not relu:
        raise ValueError('negative_slope is the slope of the fused '
                         'activation: it needs relu=True')


def _activate(y, relu, negative_slope):
    if not relu:
        return y
    return F.leaky_relu(y, negative_slope) if negative_slope else F.relu(y)


def group_norm(x, num_groups, weight=None, bias=None, eps=1e-5, relu=False,
               negative_slope=0.0):
    """F.group_norm over [N, C, S...] followed, with relu=True, by
    z > 0 ? z : negative_slope * z. On GPU the HIP kernels (bf16 out); on
    CPU the composed torch ops."""
    _check_act(relu, negative_slope)
    if not (x.is_cuda and native_available()):
        y = F.group_norm(x, num_groups, weight, bias, eps)
        return _activate(y, relu, negative_slope)
    if x.dim() < 3:
        raise ValueError(f'group_norm wants [N, C, S...], got {x.dim()}D')
    channels = x.size(1)
    if channels % num_groups != 0:
        raise ValueError(f'{channels} channels do not divide into '
                         f'{num_groups} groups')
    if weight is None:
        weight = torch.ones(channels, device=x.device)
    if bias is None:
        bias = torch.zeros(channels, device=x.device)
    return _GroupNormFn.apply(x, weight, bias, num_groups, float(eps),
                              bool(relu), float(negative_slope))


class OpsGroupNorm(nn.GroupNorm):
    """nn.GroupNorm (same parameters and state dict) with an optional fused
    (leaky) ReLU. No running statistics: train and eval are one path."""

    def __init__(self, num_groups, num_channels, eps=1e-5, affine=True,
                 relu=False, negative_slope=0.0, **kw):
        super().__init__(num_groups, num_channels, eps=eps, affine=affine,
                         **kw)
        _check_act(relu, negative_slope)
        self.relu = relu
        self.negative_slope = negative_slope

    def forward(self, x):
        return group_norm(x, self.num_groups, self.weight, self.bias,
                          self.eps, self.relu, self.negative_slope)


class OpsInstanceNorm3d(nn.InstanceNorm3d):
    """nn.InstanceNorm3d with an optional fused (leaky) ReLU: group_norm
    with one group per channel. With track_running_stats the parent class
    normalizes (running-statistics InstanceNorm has no kernel here)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=False,
                 track_running_stats=False, relu=False, negative_slope=0.0,
                 **kw):
        super().__init__(num_features, eps=eps, momentum=momentum,
                         affine=affine,
                         track_running_stats=track_running_stats, **kw)
        _check_act(relu, negative_slope)
        self.relu = relu
        self.negative_slope = negative_slope

    def forward(self, x):
        if (x.is_cuda and native_available() and x.dim() == 5
                and not self.track_running_stats):
            return group_norm(x, x.size(1), self.weight, self.bias,
                              self.eps, self.relu, self.negative_slope)
        return _activate(super().forward(x), self.relu, self.negative_slope)


def norm_relu3d(norm, channels, norm_groups=8):
    """The models' norm + ReLU layer after a conv of `channels` outputs:
    'batch' (OpsBatchNorm3d), 'group' (min(norm_groups, channels) groups)
    or 'instance' (affine)."""
    if norm == 'batch':
        return OpsBatchNorm3d(channels, relu=True)
    if norm == 'group':
        groups = min(norm_groups, channels)
        if groups < 1 or channels % groups != 0:
            raise ValueError(f'{channels} channels do not divide into '
                             f'{groups} groups')
        return OpsGroupNorm(groups, channels, relu=True)
    if norm == 'instance':
        return OpsInstanceNorm3d(channels, affine=True, relu=True)
    raise ValueError(f"norm must be 'batch', 'group' or 'instance', "
                     f'got {norm!r}')
