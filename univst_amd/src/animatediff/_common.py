"""Shared pieces of the three AnimateDiff command-line entry points (mirrors of src/animatediff/run_*_animatediff.py of the reference).

As on the SD path (src/sd/_common.py): CLIP stays a stock PyTorch-ROCm module unless ``UNIVST_TEXT_ENCODER=native``, the SVD temporal VAE runs on
the native library unless ``UNIVST_VAE=stock``; both must be available locally.  The UNet is the native AnimateDiff UNet3D
(``UNet3DConditionModel.from_pretrained_2d`` + ``load_weights`` for the motion checkpoint).

``animatediff-v2.yaml`` of the reference is not carried: its seven ``unet_additional_kwargs`` and four ``noise_scheduler_kwargs`` are the constants
below.  A ``backbones/animatediff/animatediff-v2.yaml`` in the working directory (the reference's checkout) is read instead when it is there,
with PyYAML (the reference reads it with omegaconf, which is not required here).

The pipeline's scheduler is ``DDIMScheduler(**noise_scheduler_kwargs)`` (run_*_animatediff.py:56): diffusers' when importable, else the native
one.  The yaml does not set ``set_alpha_to_one``; the reference therefore runs on diffusers' default True (the last step returns x0), which is
passed explicitly here since the native scheduler's default is the SD-v1.5 file's False.  The INVERSION scheduler is another object,
``DDIMScheduler.from_pretrained(model, subfolder="scheduler")``: the SD-v1.5 file (scaled_linear, set_alpha_to_one false)."""
import os

import torch

from ..sd._common import load_text_encoder

UNET_ADDITIONAL_KWARGS = {
    "use_inflated_groupnorm": True,
    "use_motion_module": True,
    "motion_module_resolutions": [1, 2, 4, 8],
    "motion_module_mid_block": True,
    "motion_module_type": "Vanilla",
    "motion_module_kwargs": {"num_attention_heads": 8, "num_transformer_block": 1, "attention_block_types": ["Temporal_Self", "Temporal_Self"],
                             "temporal_position_encoding": True, "temporal_attention_dim_div": 1, "zero_initialize": True},
}
NOISE_SCHEDULER_KWARGS = {"beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "linear", "steps_offset": 1, "clip_sample": False}
INFERENCE_CONFIG = os.path.join("backbones", "animatediff", "animatediff-v2.yaml")


def inference_config():
    """(unet_additional_kwargs, noise_scheduler_kwargs): the file in the working directory when there is one, else the constants"""
    if os.path.isfile(INFERENCE_CONFIG):
        import yaml
        with open(INFERENCE_CONFIG) as f:
            cfg = yaml.safe_load(f)
        return dict(cfg["unet_additional_kwargs"]), dict(cfg["noise_scheduler_kwargs"])
    return ({k: (dict(v) if isinstance(v, dict) else v) for k, v in UNET_ADDITIONAL_KWARGS.items()}, dict(NOISE_SCHEDULER_KWARGS))


def build_pipeline(pretrained_model_path, motion_module_path, weight_dtype=torch.float16, vae_path="stabilityai/stable-video-diffusion-img2vid"):
    """The objects run_*_animatediff.py build (:43-63).  Returns (pipe, DDIMScheduler class for the inversion scheduler)."""
    from transformers import CLIPTokenizer
    from ...backbones.animatediff.models.unet import UNet3DConditionModel
    from ...backbones.animatediff.pipelines.pipeline_animation import AnimationPipeline
    from ...backbones.animatediff.utils.util import load_weights
    from ...vae import NativeTemporalVAE
    try:
        from diffusers import DDIMScheduler
    except ImportError:
        from ...schedulers import DDIMScheduler
    tokenizer = CLIPTokenizer.from_pretrained(pretrained_model_path, subfolder="tokenizer")
    text_encoder = load_text_encoder(pretrained_model_path, "text_encoder", weight_dtype, projected=False)
    vae = None
    stock = os.environ.get("UNIVST_VAE", "native") == "stock"
    if not stock and weight_dtype != torch.float16:
        print(f"[univst_amd] weight_dtype {weight_dtype}: the native temporal VAE is fp16-only, using the stock AutoencoderKLTemporalDecoder", flush=True)
        stock = True
    if not stock and os.path.isdir(os.path.join(vae_path, "vae")):
        vae = NativeTemporalVAE.from_pretrained(vae_path, subfolder="vae")
    if vae is None:
        try:
            from diffusers import AutoencoderKLTemporalDecoder
        except ImportError as e:  # pragma: no cover
            raise RuntimeError(f"the temporal VAE could not be loaded: {vae_path}/vae is not a local diffusers-format directory and `diffusers` (which would "
                               "resolve it from the hub cache) is not installed") from e
        vae = AutoencoderKLTemporalDecoder.from_pretrained(vae_path, subfolder="vae").requires_grad_(False).to(weight_dtype).cuda()
        if not stock:
            vae = NativeTemporalVAE.from_module(vae)
    unet_kwargs, sched_kwargs = inference_config()
    unet = UNet3DConditionModel.from_pretrained_2d(pretrained_model_path, subfolder="unet", unet_additional_kwargs=unet_kwargs).requires_grad_(False)
    sched_kwargs.setdefault("set_alpha_to_one", True)         # diffusers' default, which the reference's DDIMScheduler(**kwargs) runs on
    pipe = AnimationPipeline(vae=vae, text_encoder=text_encoder.to(weight_dtype).cuda(), tokenizer=tokenizer, unet=unet.to(weight_dtype).cuda(),
                             scheduler=DDIMScheduler(**sched_kwargs))
    pipe = load_weights(pipe, motion_module_path=motion_module_path, device="cuda", dtype=weight_dtype)
    return pipe, DDIMScheduler


def add_common_args(parser):
    parser.add_argument("--pretrained_model_path", type=str, default="stable-diffusion-v1-5/stable-diffusion-v1-5")
    parser.add_argument("--motion_module_path", type=str, default="ckpts/mm_sd_v15_v2.ckpt")
    parser.add_argument("--weight_dtype", type=torch.dtype, default=torch.float16)
    parser.add_argument("--time_steps", type=int, default=50)
    parser.add_argument("--seed", type=int, default=33)
    return parser
