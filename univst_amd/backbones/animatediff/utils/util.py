"""Mirror of backbones/animatediff/utils/util.py of the reference: ``load_weights`` (:89-176) and ``save_videos_grid``.

``load_weights`` loads a motion-module checkpoint into ``animation_pipeline.unet`` exactly as the reference does (:106-121): ``state_dict`` is
unwrapped, only names that contain ``motion_modules.`` and not ``pos_encoder.pe`` are kept, ``load_state_dict(strict=False)``, no unexpected key.
Nothing is ever downloaded (the reference's ``auto_download`` fetches a missing file from the hub): a missing file is a ``FileNotFoundError``
that names it.  The image-layer paths — DreamBooth checkpoints, LoRA, the domain adapter, motion LoRAs — need the reference's converters
(``utils/convert_from_ckpt.py``, ``utils/convert_lora_safetensor_to_diffusers.py``), which are not built: asking for one raises
``NotImplementedError`` naming the converter."""
import os

import torch

from ....src.util import save_videos_grid  # noqa: F401  (re-exported: the reference module defines its own copy, :59-71)


def _not_built(arg, converter):
    raise NotImplementedError(f"load_weights({arg}=...) is not built: it needs the reference's backbones/animatediff/utils/{converter}, "
                              "which this repository does not carry; convert the checkpoint to diffusers format with the reference first")


def load_weights(animation_pipeline,
                 # motion module
                 motion_module_path="", motion_module_lora_configs=[],
                 # domain adapter
                 adapter_lora_path="", adapter_lora_scale=1.0,
                 # image layers
                 dreambooth_model_path="", lora_model_path="", lora_alpha=0.8,
                 device="cpu", dtype=torch.float16):
    if dreambooth_model_path != "":
        _not_built("dreambooth_model_path", "convert_from_ckpt.py (convert_ldm_unet_checkpoint / convert_ldm_clip_checkpoint)")
    if lora_model_path != "":
        _not_built("lora_model_path", "convert_lora_safetensor_to_diffusers.py (convert_lora)")
    if adapter_lora_path != "":
        _not_built("adapter_lora_path", "convert_lora_safetensor_to_diffusers.py (load_diffusers_lora)")
    if motion_module_lora_configs:
        _not_built("motion_module_lora_configs", "convert_lora_safetensor_to_diffusers.py (load_diffusers_lora)")
    unet_state_dict = {}
    if motion_module_path != "":
        if not os.path.isfile(motion_module_path):
            raise FileNotFoundError(f"load_weights: motion module checkpoint {motion_module_path} does not exist (nothing is downloaded: "
                                    "place the file there)")
        print(f"load motion module from {motion_module_path}")
        sd = torch.load(motion_module_path, map_location="cpu", weights_only=True)
        sd = sd["state_dict"] if "state_dict" in sd else sd
        for name, param in sd.items():
            if "motion_modules." not in name:
                continue
            if "pos_encoder.pe" in name:
                continue
            unet_state_dict[name] = param
    missing, unexpected = animation_pipeline.unet.load_state_dict(unet_state_dict, strict=False)
    assert len(unexpected) == 0, f"load_weights: keys the UNet does not have: {list(unexpected)[:4]}"
    return animation_pipeline
