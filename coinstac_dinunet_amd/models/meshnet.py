"""MeshNet: volumetric segmentation by a stack of dilated 3x3x3 convs at
full resolution (Fedorov et al., "End-to-end learning of brain tissue
segmentation from imperfect labeling", IJCNN 2017; the dilation schedule
follows Yu & Koltun's context module).

No pooling, no decoder: conv(3x3x3, dilation d, padding d) -> BN -> ReLU
with d running up and back down at a constant small channel count, then a
1x1x1 head. The receptive field grows with the dilations while every
activation keeps the input's resolution.

MI355X mapping: the d = 1 layers are the dense spatial-slab kernels, the
d >= 2 layers the sub-lattice slab kernels of conv3d_dilated.hip (forward,
dgrad, wgrad), BN+ReLU the fused bnorm kernels and the head the pointwise
kernel. Like UNet3D the model returns logits: train with ops.cross_entropy
or ops.dice_loss_with_logits, or with ops.softmax_dice_loss (multi-class
soft-dice + CE, segdice.hip) for parcellation labels; count with
Prf1a.add_logits /
ConfusionMatrix.add_logits.

Parameter names are those of a plain nn.Sequential of nn.Conv3d /
nn.BatchNorm3d (/ nn.Dropout3d) modules, so such a state dict loads.

norm='group' (min(norm_groups, channels) groups) or 'instance' replaces the
BatchNorm by the per-sample norms of ops/groupnorm.py, ReLU fused, at the
same positions (nn.GroupNorm / affine nn.InstanceNorm3d parameter names).
"""
import torch.nn as nn

from ..ops.groupnorm import norm_relu3d
from ..ops.conv import OpsConv3d


class MeshNet(nn.Module):
    def __init__(self, in_channels=1, num_class=2, channels=32,
                 dilations=(1, 2, 4, 8, 16, 8, 4, 2, 1), dropout=0.0,
                 norm='batch', norm_groups=8):
        super().__init__()
        layers = []
        c_in = in_channels
        for d in dilations:
            layers.append(OpsConv3d(c_in, channels, 3, padding=d, dilation=d,
                                    bias=False))
            layers.append(norm_relu3d(norm, channels, norm_groups))
            if dropout > 0:
                layers.append(nn.Dropout3d(dropout))
            c_in = channels
        layers.append(OpsConv3d(channels, num_class, 1))
        self.layers = nn.Sequential(*layers)

    def forward(self, x):
        return self.layers(x)
