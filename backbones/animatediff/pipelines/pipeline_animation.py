from univst_amd.backbones.animatediff.pipelines.pipeline_animation import *  # noqa: F401,F403
from univst_amd.backbones.animatediff.pipelines.pipeline_animation import AnimationPipeline, AnimationPipelineOutput, register_time, latent_adain  # noqa: F401
