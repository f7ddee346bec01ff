"""Conv modules on the hand-written implicit-GEMM MFMA kernels (K1).

GPU paths (bf16):
  - OpsConv3d: 3x3x3/pad-1/stride-{1,2} NCDHW on the spatial-slab/igemm
    kernels; 1x1x1 on the batched-MFMA pointwise kernels.
  - OpsConv2d: 3x3/pad-1/stride-{1,2} (+ the 7x7 stem, fwd+wgrad) on the
    2D family; 1x1 (incl. stride-2 downsamples) on the pointwise kernels.
  - conv_bn3d / conv_bn2d: the PREVIOUS block's BN(+ReLU) folded into the
    conv's input staging (normalize-on-load), with the conv epilogue
    emitting the next BN's statistics.
  - stem_conv_bn3d: the Cin = 1 first conv, its BN and the second conv as
    one node — statistics from the first conv's epilogue, BN-backward and
    the first conv's wgrad as one pass over its output.
CPU falls back to torch.nn.functional convs.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import native_available, require_native
from .bnorm import (OpsBatchNorm2d, OpsBatchNorm3d, bn_finalize_attached,
                    bn_momentum_step, has_attached_stats,
                    update_running_stats)

# Double-buffered stride-1 wgrad: numerically validated, measured WORSE
# (45.89 ms/step — LDS doubling costs co-residency more than intra-block
# overlap buys). Kept compiled behind the env flag.
_WGRAD_DB = os.environ.get('COINN_WGRAD_DB', '0') == '1'


# ---- 3x3x3 routing: pure functions of (channels, H, W, stride) ------------
# H, W are the INPUT plane of the conv being routed; the depth never
# matters (one slab covers 3 depth planes at any D).

def _out_plane(H, W, stride):
    return (H + 2 - 3) // stride + 1, (W + 2 - 3) // stride + 1


def route_fwd3d(cin, H, W, stride):
    """'spatial' | 'spatial-ctile1' | 'igemm' for the plain forward.

    Spatial tap-reuse pays when the channel tile fills and chunks are
    dense; else the igemm kernel wins (profiled in tools/bench_conv).
    Cin<16 stride-1 layers take the CTILE=1 single-channel instances
    (43.79 vs 44.46 ms/step on the flagship, profiles/r2_scaffold_ab.md).
    """
    oh, ow = _out_plane(H, W, stride)
    if ow % 8 != 0 or oh * ow < 64:
        return 'igemm'
    if cin >= 16:
        return 'spatial'
    return 'spatial-ctile1' if stride == 1 else 'igemm'


def route_fused_fwd3d(cin, H, W, stride):
    """'spatial' | 'igemm' for the normalize-on-load forward (the fused
    instances exist at the default channel tile only)."""
    oh, ow = _out_plane(H, W, stride)
    if ow % 8 == 0 and cin >= 16 and oh * ow >= 64:
        return 'spatial'
    return 'igemm'


def route_dgrad3d(cout, H, W, stride):
    """'spatial' | 's2-spatial' | 'igemm' for the input gradient; H, W are
    the conv INPUT (= dx) plane, cout the channels of grad_out."""
    if stride == 1:
        if W % 8 == 0 and cout >= 16 and H * W >= 64:
            return 'spatial'
    elif stride == 2:
        # parity classes: each works on the half-resolution sub-grid
        hsub, wsub = (H + 1) // 2, (W + 1) // 2
        if wsub % 8 == 0 and cout >= 32 and hsub * wsub >= 128:
            return 's2-spatial'
    return 'igemm'


def _dgrad3d(C, go, wb, in_shape, stride):
    route = route_dgrad3d(go.size(1), in_shape[3], in_shape[4], stride)
    if route == 'spatial':
        return C.conv3d_dgrad_spatial(go, wb, in_shape)
    if route == 's2-spatial':
        return C.conv3d_dgrad_s2_spatial(go, wb, in_shape)
    return C.conv3d_dgrad(go, wb, in_shape, stride)


class _Conv3dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        C = require_native()
        xb = x.to(torch.bfloat16)
        wb = weight.to(torch.bfloat16)
        route = route_fwd3d(xb.size(1), xb.size(3), xb.size(4), stride)
        if route == 'igemm':
            out = C.conv3d_fwd(xb, wb, stride)
        else:
            out = C.conv3d_fwd_spatial(xb, wb, stride,
                                       1 if route == 'spatial-ctile1' else 0)
        if bias is not None:
            out = out + bias.to(out.dtype).view(1, -1, 1, 1, 1)
        ctx.save_for_backward(xb, wb)
        ctx.stride = stride
        ctx.has_bias = bias is not None
        ctx.in_dtype = x.dtype
        ctx.w_dtype = weight.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        C = require_native()
        xb, wb = ctx.saved_tensors
        go = grad_out.to(torch.bfloat16).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = _dgrad3d(C, go, wb, list(xb.shape),
                          ctx.stride).to(ctx.in_dtype)
        if ctx.needs_input_grad[1]:
            variant = 1 if (_WGRAD_DB and ctx.stride == 1) else 0
            gw = C.conv3d_wgrad(xb, go, ctx.stride,
                                variant).to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = C.channel_sum(go)
        return gx, gw, gb, None


def _fused_fwd3d(C, xb, wb, bias, stride, ab):
    """Normalize-on-load forward of a 3x3x3 conv: (out, stats or None)."""
    stats = None
    if route_fused_fwd3d(xb.size(1), xb.size(3), xb.size(4),
                         stride) == 'spatial':
        if bias is None:
            # epilogue also emits this output's BN statistics — the
            # next fused pair skips its bn_reduce pass entirely
            out, stats = C.conv3d_fwd_spatial_stats(xb, wb, stride, ab)
        else:
            out = C.conv3d_fwd_spatial(xb, wb, stride, 0, ab)
    else:
        out = C.conv3d_fwd(xb, wb, stride, ab)
    if bias is not None:
        out = out + bias.to(out.dtype).view(1, -1, 1, 1, 1)
    return out, stats


class _ConvBNFn(torch.autograd.Function):
    """Previous block's BN(+ReLU) folded into this conv's input load.

    The normalized activation z = relu(gamma*xhat + beta) NEVER exists in
    HBM: the fwd kernels apply the per-channel affine during slab staging
    (bn_ab = [a, b] with a = gamma*rstd, b = beta - mean*a) and the wgrad
    kernels re-apply it on load in backward. Per BN layer this deletes one
    full activation write + one full read vs the separate normalize pass
    (VERDICT r1 item 3). mean_rstd enters as a non-differentiable constant:
    bn3d_bwd's dx formula accounts for the statistic dependence. `ab` comes
    ready from the one-launch finalize when the input carries epilogue
    partials; only without it is the affine formed here.
    """

    @staticmethod
    def forward(ctx, x_raw, gamma, beta, mean_rstd, weight, bias, stride,
                ab=None):
        C = require_native()
        xb = x_raw.to(torch.bfloat16)
        wb = weight.to(torch.bfloat16)
        if ab is None:
            ab = _affine_ab(gamma, beta, mean_rstd)
        out, stats = _fused_fwd3d(C, xb, wb, bias, stride, ab)
        ctx.save_for_backward(xb, wb, gamma, beta, mean_rstd, ab)
        ctx.stride = stride
        ctx.has_bias = bias is not None
        ctx.in_dtype = x_raw.dtype
        ctx.w_dtype = weight.dtype
        if stats is None:
            stats = torch.empty(0, device=out.device)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, grad_out, _grad_stats):
        C = require_native()
        xb, wb, gamma, beta, mean_rstd, ab = ctx.saved_tensors
        go = grad_out.to(torch.bfloat16).contiguous()
        stride = ctx.stride
        # dz = conv dgrad wrt the (virtual) normalized input — same
        # routing as the unfused path; bn3d_bwd then runs its own reduce
        # (folding it into the dgrad epilogue lost, docs/KERNELS.md)
        dz = _dgrad3d(C, go, wb, list(xb.shape), stride)
        gw = C.conv3d_wgrad(xb, go, stride, 0, ab).to(ctx.w_dtype) \
            if ctx.needs_input_grad[4] else None
        gb = C.channel_sum(go) if (ctx.has_bias
                                   and ctx.needs_input_grad[5]) else None
        dx, dgamma, dbeta = C.bn3d_bwd(dz, xb, mean_rstd, gamma, beta, True)
        return (dx.to(ctx.in_dtype), dgamma.to(gamma.dtype),
                dbeta.to(beta.dtype), None, gw, gb, None, None)


def conv_bn3d(x_raw, bn, conv):
    """Fused BN(of x_raw, from `bn`)->ReLU->conv(`conv`) on the HIP path.

    `bn` must be an OpsBatchNorm3d with relu=True; `conv` an OpsConv3d in
    the 3x3x3/pad-1/stride-{1,2} family. Handles running-stat updates with
    the exact semantics of the unfused module.
    """
    mean_rstd, ab = _bn_mean_rstd(x_raw, bn)
    out, stats = _ConvBNFn.apply(x_raw, bn.weight, bn.bias, mean_rstd,
                                 conv.weight, conv.bias,
                                 int(conv.stride[0]), ab)
    if stats.numel() > 0:
        out._coinn_bn_stats = stats
    return out


class _StemConvBNFn(torch.autograd.Function):
    """conv0 (Cin = 1) -> bn0(+ReLU) folded into conv1, as one node.

    Forward: conv0 on the single-channel instances whose epilogue emits
    bn0's statistics, the one-launch finalize, then conv1's normalize-on-
    load forward. Backward: conv0's input is the image, so the gradient of
    its raw output has one consumer, conv0's wgrad; BN-backward and that
    wgrad are linear in per-channel sums over positions and run as ONE pass
    over (x, dz, x1) — the BN input gradient never exists.
    """

    @staticmethod
    def forward(ctx, x, w0, gamma, beta, w1, bias1, stride1, bn0):
        C = require_native()
        xb = x.to(torch.bfloat16)
        w0b = w0.to(torch.bfloat16)
        w1b = w1.to(torch.bfloat16)
        x1, stats0 = C.conv3d_fwd_ci1_stats(xb, w0b)
        x1._coinn_bn_stats = stats0
        _, _, mean_rstd, ab = bn_finalize_attached(x1, bn0,
                                                   bn_momentum_step(bn0))
        out, stats = _fused_fwd3d(C, x1, w1b, bias1, stride1, ab)
        ctx.save_for_backward(xb, x1, w1b, gamma, beta, mean_rstd, ab)
        ctx.stride1 = stride1
        ctx.has_bias1 = bias1 is not None
        ctx.w0_dtype = w0.dtype
        ctx.w1_dtype = w1.dtype
        if stats is None:
            stats = torch.empty(0, device=out.device)
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    def backward(ctx, grad_out, _grad_stats):
        C = require_native()
        xb, x1, w1b, gamma, beta, mean_rstd, ab = ctx.saved_tensors
        go = grad_out.to(torch.bfloat16).contiguous()
        stride1 = ctx.stride1
        dz = _dgrad3d(C, go, w1b, list(x1.shape), stride1)
        gw1 = C.conv3d_wgrad(x1, go, stride1, 0, ab).to(ctx.w1_dtype) \
            if ctx.needs_input_grad[4] else None
        gb1 = C.channel_sum(go) if (ctx.has_bias1
                                    and ctx.needs_input_grad[5]) else None
        gw0 = dgamma = dbeta = None
        if any(ctx.needs_input_grad[1:4]):
            gw0, dgamma, dbeta = C.conv3d_wgrad_ci1_bn(
                xb, dz, x1, mean_rstd, gamma, beta)
            gw0 = gw0.to(ctx.w0_dtype)
            dgamma, dbeta = dgamma.to(gamma.dtype), dbeta.to(beta.dtype)
        return None, gw0, dgamma, dbeta, gw1, gb1, None, None


def can_fuse_stem(conv0, bn0, conv1, x):
    """True when (conv0 -> bn0 -> conv1) runs as _StemConvBNFn: conv0 is a
    bias-free stride-1 Cin = 1 conv on the image (no input gradient), bn0
    uses batch statistics, and the shape fits the one-pass backward."""
    if not (conv0.in_channels == 1 and conv0.bias is None
            and conv0.stride == (1, 1, 1) and _is_3x3_family(conv0)
            and not x.requires_grad and bn0.training
            and can_fuse_bn_conv(bn0, conv1, x) and x.dim() == 5):
        return False
    H, W = x.size(3), x.size(4)
    return (route_fwd3d(1, H, W, 1) == 'spatial-ctile1'
            and require_native().conv3d_wgrad_ci1_bn_fits(H, W))


def stem_conv_bn3d(x, conv0, bn0, conv1):
    """conv1(relu(bn0(conv0(x)))) for a stem that can_fuse_stem accepts;
    running statistics update exactly as in the unfused modules."""
    out, stats = _StemConvBNFn.apply(x, conv0.weight, bn0.weight, bn0.bias,
                                     conv1.weight, conv1.bias,
                                     int(conv1.stride[0]), bn0)
    if stats.numel() > 0:
        out._coinn_bn_stats = stats
    return out


def _affine_ab(gamma, beta, mean_rstd):
    """[C][2] (a, b) of the normalize-on-load affine z = a*x + b."""
    with torch.no_grad():
        a = gamma.float() * mean_rstd[:, 1]
        b = beta.float() - mean_rstd[:, 0] * a
        return torch.stack([a, b], 1).contiguous()


def _bn_mean_rstd(x_raw, bn):
    """([C][2] (mean, rstd), [C][2] (a, b) or None) that `bn` normalizes
    x_raw with — batch stats in training (running stats updated exactly as
    the unfused module would), running stats in eval. With epilogue
    partials attached to x_raw the training form is one native launch and
    brings the affine along; otherwise ab is None."""
    xb = x_raw if x_raw.dtype == torch.bfloat16 \
        else x_raw.to(torch.bfloat16)
    if bn.training:
        if has_attached_stats(xb):
            _, _, mean_rstd, ab = bn_finalize_attached(
                xb, bn, bn_momentum_step(bn))
            return mean_rstd, ab
        mean, var, mean_rstd = bn_stats_of(xb, bn.eps)
        update_running_stats(bn.running_mean, bn.running_var, mean, var,
                             xb.numel() // xb.size(1), bn_momentum_step(bn))
        return mean_rstd, None
    mean = bn.running_mean.float()
    rstd = torch.rsqrt(bn.running_var.float() + bn.eps)
    return torch.stack([mean, rstd], 1).contiguous(), None


def bn_stats_of(xb, eps):
    """(mean, var, mean_rstd) of a bf16 activation — from the producing
    conv's epilogue partials when attached, else one reduce pass."""
    C = require_native()
    stats = getattr(xb, '_coinn_bn_stats', None)
    if stats is not None and stats.numel() > 0:
        with torch.no_grad():
            sums = stats.sum(0)                      # [C][2]
            per_ch = xb.numel() // xb.size(1)
            mean = sums[:, 0] / per_ch
            var = (sums[:, 1] / per_ch - mean * mean).clamp_min(0)
            rstd = torch.rsqrt(var + eps)
            return mean, var, torch.stack([mean, rstd], 1).contiguous()
    return C.bn3d_stats(xb.detach(), eps)


class _ConvBN2dFn(torch.autograd.Function):
    """2D twin of _ConvBNFn: the previous BN(+ReLU) folds into this 3x3
    conv's input load (ResNet BasicBlock's bn1 -> conv2 pair)."""

    @staticmethod
    def forward(ctx, x_raw, gamma, beta, mean_rstd, weight, stride,
                ab=None):
        C = require_native()
        xb = x_raw.to(torch.bfloat16)
        wb = weight.to(torch.bfloat16)
        if ab is None:
            ab = _affine_ab(gamma, beta, mean_rstd)
        out = C.conv2d_fwd(xb, wb, stride, ab)
        ctx.save_for_backward(xb, wb, gamma, beta, mean_rstd, ab)
        ctx.stride = stride
        ctx.in_dtype = x_raw.dtype
        ctx.w_dtype = weight.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        C = require_native()
        xb, wb, gamma, beta, mean_rstd, ab = ctx.saved_tensors
        go = grad_out.to(torch.bfloat16).contiguous()
        dz = C.conv2d_dgrad(go, wb, list(xb.shape), ctx.stride)
        gw = C.conv2d_wgrad(xb, go, ctx.stride, ab).to(ctx.w_dtype) \
            if ctx.needs_input_grad[4] else None
        dx, dgamma, dbeta = C.bn3d_bwd(dz, xb, mean_rstd, gamma, beta, True)
        return (dx.to(ctx.in_dtype), dgamma.to(gamma.dtype),
                dbeta.to(beta.dtype), None, gw, None, None)


def conv_bn2d(x_raw, bn, conv):
    """Fused BN(+ReLU) -> 3x3 Conv2d (the 2D twin of conv_bn3d)."""
    mean_rstd, ab = _bn_mean_rstd(x_raw, bn)
    return _ConvBN2dFn.apply(x_raw, bn.weight, bn.bias, mean_rstd,
                             conv.weight, int(conv.stride[0]), ab)


def _is_3x3_family(conv):
    """3x3(x3) / pad 1 / isotropic stride 1 or 2 / no dilation / groups 1:
    the family the in-tree implicit-GEMM kernels cover, at either rank."""
    rank = len(conv.kernel_size)
    return (conv.kernel_size == (3,) * rank
            and conv.padding == (1,) * rank
            and conv.stride[0] in (1, 2)
            and conv.stride == (conv.stride[0],) * rank
            and conv.dilation == (1,) * rank and conv.groups == 1)


def can_fuse_bn_conv2d(bn, conv, x):
    """True when the 2D (bn -> conv) pair routes onto the fused kernels."""
    return (x.is_cuda and native_available()
            and isinstance(bn, OpsBatchNorm2d) and bn.relu
            and isinstance(conv, OpsConv2d) and conv.bias is None
            and _is_3x3_family(conv))


def can_fuse_bn_conv(bn, conv, x):
    """True when the (bn -> conv) pair routes onto the fused kernels."""
    return (x.is_cuda and native_available()
            and isinstance(bn, OpsBatchNorm3d) and bn.relu
            and isinstance(conv, OpsConv3d) and _is_3x3_family(conv))


class _ConvPw3dFn(torch.autograd.Function):
    """1x1x1 (pointwise) conv — a per-position channel GEMM on the
    bandwidth-shaped pointwise kernels (UNet3D segmentation head)."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        C = require_native()
        xb = x.to(torch.bfloat16)
        wb = weight.to(torch.bfloat16)
        empty = torch.empty(0, device=x.device)
        out = C.conv3d_pw_fwd(xb, wb.view(wb.size(0), wb.size(1)),
                              bias if bias is not None else empty)
        ctx.save_for_backward(xb, wb)
        ctx.has_bias = bias is not None
        ctx.in_dtype = x.dtype
        ctx.w_dtype = weight.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        C = require_native()
        xb, wb = ctx.saved_tensors
        go = grad_out.to(torch.bfloat16).contiguous()
        gx = gw = gb = None
        w2d = wb.view(wb.size(0), wb.size(1))
        if ctx.needs_input_grad[0]:
            gx = C.conv3d_pw_dgrad(go, w2d).to(ctx.in_dtype)
        if ctx.needs_input_grad[1]:
            gw = C.conv3d_pw_wgrad(xb, go).view_as(wb).to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = C.channel_sum(go)
        return gx, gw, gb


def conv3d(x, weight, bias=None, stride=1):
    if x.is_cuda and native_available() and weight.shape[2:] == (3, 3, 3):
        return _Conv3dFn.apply(x, weight, bias, int(stride))
    return F.conv3d(x, weight, bias, stride=stride, padding=1)


class _Conv2dFn(torch.autograd.Function):
    """3x3/pad-1 (and 7x7/pad-3 stem, fwd+wgrad) Conv2d on the 2D
    implicit-GEMM MFMA kernels (conv2d.hip) — the ResNet-18 hot path
    (VERDICT r1 item 7). The 7x7 dgrad is unimplemented: the stem is the
    first layer, its input never needs a gradient (module routing
    enforces this)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride):
        C = require_native()
        xb = x.to(torch.bfloat16)
        wb = weight.to(torch.bfloat16)
        out = C.conv2d_fwd(xb, wb, stride)
        if bias is not None:
            out = out + bias.to(out.dtype).view(1, -1, 1, 1)
        ctx.save_for_backward(xb, wb)
        ctx.stride = stride
        ctx.ks = weight.shape[2]
        ctx.has_bias = bias is not None
        ctx.in_dtype = x.dtype
        ctx.w_dtype = weight.dtype
        return out

    @staticmethod
    def backward(ctx, grad_out):
        C = require_native()
        xb, wb = ctx.saved_tensors
        go = grad_out.to(torch.bfloat16).contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            assert ctx.ks == 3, '7x7 dgrad not implemented (stem only)'
            gx = C.conv2d_dgrad(go, wb, list(xb.shape),
                                ctx.stride).to(ctx.in_dtype)
        if ctx.needs_input_grad[1]:
            gw = C.conv2d_wgrad(xb, go, ctx.stride,
                                ks=ctx.ks).to(ctx.w_dtype)
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = C.channel_sum(go)
        return gx, gw, gb, None


class OpsConv2d(nn.Conv2d):
    """nn.Conv2d on the in-tree MFMA kernels where the family allows.

    3x3/pad-1/stride-{1,2} -> 2D implicit-GEMM kernels; 1x1 -> the
    (rank-agnostic) pointwise kernels, with stride-2 1x1 downsamples
    handled by a strided view ahead of the pointwise GEMM. Anything else
    (e.g. the 7x7 stem) falls through to the library conv.
    """

    def forward(self, x):
        if x.is_cuda and native_available() and self.dilation == (1, 1) \
                and self.groups == 1:
            if _is_3x3_family(self):
                return _Conv2dFn.apply(x, self.weight, self.bias,
                                       int(self.stride[0]))
            # 7x7 stem: fwd+wgrad in-tree; input must not need a gradient
            # (it is the image) since the 7x7 dgrad is not implemented
            if (self.kernel_size == (7, 7) and self.padding == (3, 3)
                    and self.stride[0] in (1, 2)
                    and self.stride[0] == self.stride[1]
                    and not x.requires_grad):
                return _Conv2dFn.apply(x, self.weight, self.bias,
                                       int(self.stride[0]))
            if self.kernel_size == (1, 1) and self.padding == (0, 0):
                if self.stride != (1, 1):
                    x = x[:, :, ::self.stride[0], ::self.stride[1]] \
                        .contiguous()
                return _ConvPw3dFn.apply(x, self.weight, self.bias)
        if x.is_cuda and x.dtype != self.weight.dtype:
            x = x.to(self.weight.dtype)
        return super().forward(x)


class OpsConv3d(nn.Conv3d):
    """nn.Conv3d that runs the MFMA implicit-GEMM kernels on GPU.

    Only 3x3x3/pad-1/stride-{1,2} routes to the HIP path; anything else
    falls through to the library conv.
    """

    def forward(self, x):
        if x.is_cuda and native_available() and _is_3x3_family(self):
            return _Conv3dFn.apply(x, self.weight, self.bias,
                                   int(self.stride[0]))
        if (x.is_cuda and native_available()
                and self.kernel_size == (1, 1, 1)
                and self.padding == (0, 0, 0)
                and self.stride == (1, 1, 1)
                and self.dilation == (1, 1, 1) and self.groups == 1):
            return _ConvPw3dFn.apply(x, self.weight, self.bias)
        # library fallback must still accept the bf16 activations the fused
        # kernels upstream emit (bf16 act into fp32 head crashed)
        if x.is_cuda and x.dtype != self.weight.dtype:
            x = x.to(self.weight.dtype)
        return super().forward(x)
