from univst_amd.backbones.animatediff.utils.util import *  # noqa: F401,F403
from univst_amd.backbones.animatediff.utils.util import load_weights, save_videos_grid  # noqa: F401
