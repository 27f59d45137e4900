from univst_amd.backbones.animatediff.models.motion_module import *  # noqa: F401,F403
from univst_amd.backbones.animatediff.models.motion_module import get_motion_module, VanillaTemporalModule, zero_module  # noqa: F401
