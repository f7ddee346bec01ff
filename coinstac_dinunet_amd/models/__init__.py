from .icalstm import ICALstm
from .icatransformer import ICATransformer
from .meshnet import MeshNet
from .mlp import FreeSurferMLP
from .resnet import ResNet18
from .unet import UNet3D
from .vbm import VBMNet

__all__ = ['FreeSurferMLP', 'VBMNet', 'ResNet18', 'UNet3D', 'MeshNet',
           'ICALstm', 'ICATransformer']
