"""CLI mirror of src/animatediff/run_video_style_transfer_animatediff.py (reference :78-88 flags).  As the reference's script, and unlike the SD
one, it starts from the content inversion's last latent as it is (:60-69: no initial latent AdaIN)."""
import argparse
import os

from ._common import add_common_args, build_pipeline
from ...backbones.animatediff.pnp_utils import register_spatial_attention_pnp
from ..util import load_ddim_latents_at_t, save_folder, seed_everything


def main(a):
    if a.seed is not None:
        seed_everything(a.seed)
    pipe, _ = build_pipeline(a.pretrained_model_path, a.motion_module_path, a.weight_dtype)
    content_noise = load_ddim_latents_at_t(a.time_steps, ddim_latents_path=a.content_inv_path).to(a.weight_dtype).cuda()
    register_spatial_attention_pnp(pipe)                                   # PnP: AdaIN-guided attention injection
    sample = pipe.video_style_transfer("", latents=content_noise, num_inference_steps=a.time_steps, content_inv_path=a.content_inv_path,
                                       style_inv_path=a.style_inv_path, mask_path=a.mask_path or None).images
    sample = sample.permute(0, 4, 1, 2, 3).contiguous()
    out = os.path.join(a.output_path, "animatediff", f'{a.content_inv_path.split("/")[-2]}_{a.style_inv_path.split("/")[-2]}')
    os.makedirs(out, exist_ok=True)
    save_folder(sample, out)


def parser():
    p = add_common_args(argparse.ArgumentParser())
    p.add_argument("--content_inv_path", type=str, default="results/contents-inv/animatediff/mallard-fly/inversion")
    p.add_argument("--style_inv_path", type=str, default="results/styles-inv/animatediff/00033/inversion")
    p.add_argument("--mask_path", type=str, default="results/masks/animatediff/mallard-fly")
    p.add_argument("--output_path", type=str, default="results/stylizations")
    return p


if __name__ == "__main__":
    main(parser().parse_args())
