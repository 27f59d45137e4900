#!/usr/bin/env bash
# The four-step recipe of the AnimateDiff backbone on the MI355X-native implementation: content inversion (with the feature dump of
# up_blocks[2] at t = 301), style inversion, mask propagation on the dumped feature, localized video style transfer.
# Needs a local SD-v1.5 directory, the motion checkpoint ckpts/mm_sd_v15_v2.ckpt and the SVD VAE; nothing is downloaded.
export PYTHONPATH=$(pwd)
set -e
python src/animatediff/run_content_inversion_animatediff.py --content_path examples/contents/mallard-fly --output_path results/contents-inv --is_opt
python src/animatediff/run_style_inversion_animatediff.py --style_path examples/styles/00033.png --output_path results/styles-inv
python src/mask_propagation.py --feature_path results/contents-inv/animatediff/mallard-fly/features/inversion_feature_map_2_block_301_step.pt \
       --backbone animatediff --mask_path examples/masks/mallard-fly.png --output_path results/masks
python src/animatediff/run_video_style_transfer_animatediff.py --content_inv_path results/contents-inv/animatediff/mallard-fly/inversion \
       --style_inv_path results/styles-inv/animatediff/00033/inversion --mask_path results/masks/animatediff/mallard-fly --output_path results/stylizations
