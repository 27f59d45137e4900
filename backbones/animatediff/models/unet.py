from univst_amd.backbones.animatediff.models.unet import *  # noqa: F401,F403
from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel, UNet3DConditionOutput, InflatedConv3d, InflatedGroupNorm  # noqa: F401
