"""3D U-Net for volumetric segmentation — the reference ecosystem's
segmentation use case (dice_loss_binary in metrics/loss.py, the U-Net
patch utilities in vision/imageutils.py, safe_concat in
utils/tensorutils.py all exist to serve it; the model itself lives in
the external implementation repos).

MI355X mapping: every conv is a 3x3x3/pad-1 stride-1 or stride-2
OpsConv3d, so the whole encoder/decoder runs on the spatial-slab MFMA
kernels; BN+ReLU are the fused bnorm kernels. Downsampling is stride-2
convolution (not pooling). Upsampling has two modes:

up_mode='nearest' (default): nearest-neighbor interp + 3x3x3 conv. Where the
skip is exactly twice the decoder input (even sizes) the pair runs as
ops.upsample2_conv3d: 8 parity classes of 2x2x2 convs on the low-res input
(upconv3d.hip), so the 8x upsampled activation is never written, read or
kept for backward. COINN_FUSE_UPSAMPLE=0 restores interpolate + conv, which
odd skip sizes always take.

up_mode='transpose': the learned upsample of the original 3D U-Net, V-Net
and nnU-Net, ConvTranspose3d(kernel 2, stride 2) with bias, as
OpsConvTranspose3d on the deconv3d.hip kernels (same parameter names as
nn.ConvTranspose3d, so such checkpoints load). Its output is exactly twice
the decoder input; where the skip is smaller (odd encoder sizes) it is
cropped to the skip before the concat.

Skip connections go through safe_concat (center-crop) so odd input sizes
work.

Loss head: the model returns logits. Train on them directly with
ops.dice_loss_with_logits (num_class=1) or ops.cross_entropy on the
[N, C, D, H, W] logits (num_class > 1), or ops.softmax_dice_loss for
multi-class soft-dice + CE (ops/csrc/segdice.hip), and count with
Prf1a.add_logits / ConfusionMatrix.add_logits — on GPU these are the fused
kernels of ops/csrc/segloss.hip, with no probability or prediction tensor.
"""
import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.groupnorm import norm_relu3d
from ..ops.conv import (OpsConv3d, OpsConvTranspose3d, can_fuse_bn_conv,
                        can_fuse_upsample, conv_bn3d, upsample2_conv3d)
from ..utils.tensorutils import safe_concat

_FUSE_BN = os.environ.get('COINN_FUSE_BN', '1') == '1'
_FUSE_UPSAMPLE = os.environ.get('COINN_FUSE_UPSAMPLE', '1') == '1'


class _Block(nn.Module):
    """conv(3x3x3) -> fused BN+ReLU, twice; optional stride-2 entry.

    On GPU the inner (b1 -> c2) pair runs as one normalize-on-load fused
    conv (conv_bn3d), so b1's normalized activation never hits HBM."""

    def __init__(self, cin, cout, stride=1, norm='batch', norm_groups=8):
        super().__init__()
        self.c1 = OpsConv3d(cin, cout, 3, stride=stride, padding=1,
                            bias=False)
        self.b1 = norm_relu3d(norm, cout, norm_groups)
        self.c2 = OpsConv3d(cout, cout, 3, stride=1, padding=1, bias=False)
        self.b2 = norm_relu3d(norm, cout, norm_groups)

    def forward(self, x):
        if _FUSE_BN and can_fuse_bn_conv(self.b1, self.c2, x):
            return self.b2(conv_bn3d(self.c1(x), self.b1, self.c2))
        return self.b2(self.c2(self.b1(self.c1(x))))


class UNet3D(nn.Module):
    """Encoder-decoder with skip connections; `widths` sets depth.

    norm='batch' (default), 'group' (min(norm_groups, C) groups) or
    'instance' picks the fused norm + ReLU of every block; the per-sample
    norms (ops/groupnorm.py) keep no batch statistics, which suits sites
    with differently distributed data. They run as separate passes, not on
    the normalize-on-load path."""

    def __init__(self, in_channels=1, num_class=2, widths=(16, 32, 64),
                 up_mode='nearest', norm='batch', norm_groups=8):
        super().__init__()
        if up_mode not in ('nearest', 'transpose'):
            raise ValueError(f"up_mode must be 'nearest' or 'transpose', "
                             f'got {up_mode!r}')
        self.up_mode = up_mode
        nk = dict(norm=norm, norm_groups=norm_groups)
        self.stem = _Block(in_channels, widths[0], **nk)
        self.down = nn.ModuleList(
            _Block(widths[i], widths[i + 1], stride=2, **nk)
            for i in range(len(widths) - 1))
        if up_mode == 'transpose':
            self.up_conv = nn.ModuleList(
                OpsConvTranspose3d(widths[i + 1], widths[i], 2, stride=2)
                for i in reversed(range(len(widths) - 1)))
        else:
            self.up_conv = nn.ModuleList(
                OpsConv3d(widths[i + 1], widths[i], 3, padding=1, bias=False)
                for i in reversed(range(len(widths) - 1)))
        self.up_block = nn.ModuleList(
            _Block(2 * widths[i], widths[i], **nk)
            for i in reversed(range(len(widths) - 1)))
        # 1x1x1 head runs on the pointwise HIP kernel (accepts the fused-BN
        # path's bf16 activations; the stock fp32 nn.Conv3d head crashed on
        # the dtype boundary — ADVICE r1 / VERDICT r1 item 1)
        self.head = OpsConv3d(widths[0], num_class, 1)

    def forward(self, x):
        skips = []
        x = self.stem(x)
        for d in self.down:
            skips.append(x)
            x = d(x)
        for conv, block in zip(self.up_conv, self.up_block):
            skip = skips.pop()
            if self.up_mode == 'transpose':
                x = conv(x)
                sd, sh, sw = skip.shape[2:]
                if tuple(x.shape[2:]) != (sd, sh, sw):
                    x = x[..., :sd, :sh, :sw]
            elif _FUSE_UPSAMPLE and can_fuse_upsample(conv, x, skip.shape[2:]):
                x = upsample2_conv3d(x, conv.weight, conv.bias)
            else:
                x = F.interpolate(x, size=skip.shape[2:], mode='nearest')
                x = conv(x)
            x = block(safe_concat(skip, x))
        return self.head(x)
