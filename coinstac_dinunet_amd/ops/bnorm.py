"""BatchNorm3d(+fused ReLU) on the HIP streaming kernels.

Training fwd: one reduce + one normalize pass (HBM-roofline); the ReLU
folds into the normalize so conv->bn->relu is 2 passes instead of
MIOpen's BN + a separate clamp kernel. Running-stat semantics match
nn.BatchNorm3d (biased var normalizes, unbiased updates running_var).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native_available, require_native


def bn_momentum_step(bn):
    """Count one training batch on `bn` and return the running-stat update
    factor the way nn.BatchNorm resolves it: `momentum`, or the cumulative
    average 1/num_batches_tracked when momentum is None. Returns None when
    the module tracks no running stats (nothing is touched)."""
    if bn.num_batches_tracked is not None:
        bn.num_batches_tracked.add_(1)
    if bn.running_mean is None:
        return None
    if bn.momentum is None:
        # reads the counter back to the host, as nn.BatchNorm does: a device
        # sync per step, and not capturable in a hipGraph
        return 1.0 / float(bn.num_batches_tracked)
    return bn.momentum


def update_running_stats(running_mean, running_var, mean, var, n, factor):
    """running <- (1 - factor) * running + factor * batch, from the batch
    mean and BIASED variance over n elements per channel (running_var takes
    the unbiased estimate, as nn.BatchNorm). No-op without buffers."""
    if running_mean is None:
        return
    with torch.no_grad():
        unbiased = var * (n / max(n - 1, 1))
        running_mean.mul_(1 - factor).add_(mean, alpha=factor)
        running_var.mul_(1 - factor).add_(unbiased, alpha=factor)


def _native_running(t):
    return t.is_cuda and t.dtype == torch.float32 and t.is_contiguous()


def bn_finalize_attached(x, bn, factor):
    """(mean, var, mean_rstd, ab) of `x` from the epilogue partials its
    producing conv attached (x._coinn_bn_stats), in ONE launch: folds the
    slices, forms ab = (gamma*rstd, beta - mean*gamma*rstd) for the
    normalize-on-load consumers and applies `factor` (from
    bn_momentum_step; None = no update) to bn's running buffers."""
    C = require_native()
    per_ch = x.numel() // x.size(1)
    rm, rv = bn.running_mean, bn.running_var
    update = factor is not None and rm is not None
    fused = update and _native_running(rm) and _native_running(rv)
    with torch.no_grad():
        mean, var, mean_rstd, ab = C.bn_finalize(
            x._coinn_bn_stats, per_ch, bn.eps, bn.weight, bn.bias,
            rm if fused else None, rv if fused else None,
            factor if fused else 0.0)
        if update and not fused:
            update_running_stats(rm, rv, mean, var, per_ch, factor)
    return mean, var, mean_rstd, ab


def has_attached_stats(x):
    stats = getattr(x, '_coinn_bn_stats', None)
    return stats is not None and stats.numel() > 0


def _bn3d_backward(ctx, dy):
    """Shared backward of _BN3dFn / _BN3dPreFn: grads for (x, gamma, beta);
    every further forward argument is non-differentiable."""
    C = require_native()
    xb, mean_rstd, gamma, beta = ctx.saved_tensors
    dx, dgamma, dbeta = C.bn3d_bwd(dy.to(torch.bfloat16), xb, mean_rstd,
                                   gamma, beta, ctx.relu)
    return (dx.to(ctx.in_dtype), dgamma.to(gamma.dtype),
            dbeta.to(beta.dtype)) + (None,) * (len(ctx.needs_input_grad) - 3)


class _BN3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, factor,
                eps, relu):
        C = require_native()
        xb = x.to(torch.bfloat16)
        y, mean, var, mean_rstd = C.bn3d_fwd(xb, gamma, beta, eps, relu)
        update_running_stats(running_mean, running_var, mean, var,
                             xb.numel() // xb.size(1), factor)
        ctx.save_for_backward(xb, mean_rstd, gamma, beta)
        ctx.relu = relu
        ctx.in_dtype = x.dtype
        return y

    backward = staticmethod(_bn3d_backward)


class _OpsBNMixin:
    """Shared HIP-kernel forward for the 2D/3D BatchNorm modules — the
    streaming kernels only see [N, C, spatial] and are rank-agnostic."""

    def _ops_forward(self, x, super_forward):
        if not (x.is_cuda and native_available()):
            y = super_forward(x)
            return F.relu(y, inplace=True) if self.relu else y
        if self.training:
            factor = bn_momentum_step(self)
            if has_attached_stats(x):
                # stats came free from the producing conv's epilogue; pass
                # x itself: .to() would drop the attached stats
                _, _, mean_rstd, _ = bn_finalize_attached(x, self, factor)
                return _BN3dPreFn.apply(x, self.weight, self.bias,
                                        mean_rstd, self.relu)
            return _BN3dFn.apply(x, self.weight, self.bias,
                                 self.running_mean, self.running_var,
                                 factor, self.eps, self.relu)
        C = require_native()
        return C.bn3d_infer(x.to(torch.bfloat16), self.weight, self.bias,
                            self.running_mean, self.running_var, self.eps,
                            self.relu)


class _BN3dPreFn(torch.autograd.Function):
    """BN normalize with externally computed batch statistics (the
    producing conv's epilogue-stats path): one normalize pass instead of
    reduce + normalize. Backward is the standard bn3d_bwd."""

    @staticmethod
    def forward(ctx, x, gamma, beta, mean_rstd, relu):
        C = require_native()
        xb = x.to(torch.bfloat16)
        y = C.bn3d_normalize(xb, mean_rstd, gamma, beta, relu)
        ctx.save_for_backward(xb, mean_rstd, gamma, beta)
        ctx.relu = relu
        ctx.in_dtype = x.dtype
        return y

    backward = staticmethod(_bn3d_backward)


class _BNAddReluFn(torch.autograd.Function):
    """BN(x) + residual -> ReLU as ONE pass each way (ResNet BasicBlock
    tail: bn2 -> +identity -> ReLU was three elementwise round-trips).
    Backward recomputes the mask from (affine(x) + res) and emits the
    residual-branch gradient (masked dy) from the same kernel."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, running_mean, running_var,
                factor, eps):
        C = require_native()
        xb = x.to(torch.bfloat16)
        rb = res.to(torch.bfloat16)
        y, mean, var, mean_rstd = C.bn3d_fwd_res(xb, rb, gamma, beta, eps)
        update_running_stats(running_mean, running_var, mean, var,
                             xb.numel() // xb.size(1), factor)
        ctx.save_for_backward(xb, rb, mean_rstd, gamma, beta)
        ctx.in_dtype = x.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        C = require_native()
        xb, rb, mean_rstd, gamma, beta = ctx.saved_tensors
        dx, dgamma, dbeta, dres = C.bn3d_bwd_res(
            dy.to(torch.bfloat16), xb, rb, mean_rstd, gamma, beta)
        return (dx.to(ctx.in_dtype), dres.to(ctx.in_dtype),
                dgamma.to(gamma.dtype), dbeta.to(beta.dtype),
                None, None, None, None)


def bn_add_relu(x, residual, bn):
    """relu(bn(x) + residual) fused on the HIP path (train mode);
    falls back to the composed ops elsewhere."""
    if x.is_cuda and native_available() and bn.training:
        factor = bn_momentum_step(bn)
        if residual.dtype != torch.bfloat16:
            residual = residual.to(torch.bfloat16)
        return _BNAddReluFn.apply(x, residual, bn.weight, bn.bias,
                                  bn.running_mean, bn.running_var,
                                  factor, bn.eps)
    y = bn(x)
    if y.dtype != residual.dtype:
        residual = residual.to(y.dtype)
    return F.relu(y + residual)


class OpsBatchNorm3d(_OpsBNMixin, nn.BatchNorm3d):
    """BatchNorm3d with optional fused ReLU; HIP kernels on GPU."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=False,
                 **kw):
        super().__init__(num_features, eps=eps, momentum=momentum, **kw)
        self.relu = relu

    def forward(self, x):
        return self._ops_forward(x, super().forward)


class OpsBatchNorm2d(_OpsBNMixin, nn.BatchNorm2d):
    """BatchNorm2d with optional fused ReLU on the same streaming kernels
    (ResNet-18 config)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=False,
                 **kw):
        super().__init__(num_features, eps=eps, momentum=momentum, **kw)
        self.relu = relu

    def forward(self, x):
        return self._ops_forward(x, super().forward)
