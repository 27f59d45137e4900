"""CLI mirror of src/sd3/run_style_inversion_sd3.py (reference :90-106 flags)."""
import argparse
import os

import torch

from ._common import add_common_args, build_pipeline
from ...inversion_tools.flow_inversion import style_inversion_reconstruction
from ..util import seed_everything


def main(a):
    if a.seed is not None:
        seed_everything(a.seed)
    pipe = build_pipeline(a.pretrained_model_path, a.weight_dtype, qkv_dtype=a.qkv_dtype)
    out = os.path.join(a.output_path, "sd3", a.style_path.split("/")[-1].split(".")[0])
    paths = {k: os.path.join(out, k) for k in ("inversion", "reconstruction")}
    for p in paths.values():
        os.makedirs(p, exist_ok=True)
    frames = a.num_frames
    if a.static_style:
        # the style is one image and the MM-DiT couples frames only through the key set ['first', f-1, f], which for identical frames is the frame's own
        # keys three times: ONE frame is inverted, as a clip of its own (the processors' class default of 16 is not a divisor of a one-frame batch).
        # The files keep their names and hold [1, 16, h, w]; run_video_style_transfer_sd3.py --static_style reads them
        frames = 1
        for proc in pipe.transformer.attn_processors.values():
            if hasattr(proc, "clip_length"):
                proc.clip_length = frames
    with torch.no_grad():
        style_inversion_reconstruction(pipe, a.style_path, paths["inversion"], paths["reconstruction"], frames, a.height, a.width,
                                       a.time_steps, a.weight_dtype, is_rf_solver=a.is_rf_solver, reconstruct=not a.skip_reconstruction)


def parser():
    p = add_common_args(argparse.ArgumentParser())
    p.add_argument("--style_path", type=str, default="examples/styles/00033.png")
    p.add_argument("--output_path", type=str, default="results/styles-inv")
    p.add_argument("--num_frames", type=int, default=16)
    p.add_argument("--height", type=int, default=1024)
    p.add_argument("--width", type=int, default=1024)
    p.add_argument("--is_rf_solver", action="store_true", help="use rf-solver")
    p.add_argument("--static_style", action="store_true",
                   help="extra: invert ONE style frame instead of num_frames copies; the ddim_latents_*.pt files then hold [1, 16, h, w]")
    p.add_argument("--skip_reconstruction", action="store_true", help="extra: skip the preview reconstruction (50 transformer calls)")
    return p


if __name__ == "__main__":
    main(parser().parse_args())
