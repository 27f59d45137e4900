"""Shared pieces of the three SD3 / SD3.5 command-line entry points (mirrors of src/sd3/run_*_sd3.py of the reference).

The CLIP / T5 text encoders (transformers) and the VAE (diffusers AutoencoderKL) are third-party models and stay stock
PyTorch-ROCm modules by default (``UNIVST_TEXT_ENCODER=native`` runs the two CLIP towers on the native library, univst_amd.text.NativeCLIPText, and
``UNIVST_T5_ENCODER=native`` the T5 encoder, univst_amd.text.NativeT5Encoder, ``UNIVST_SD3_VAE=native`` the VAE, univst_amd.vae.NativeAutoencoderKL — with all
three set nothing here needs diffusers); they must be available locally — there is no hub access on the target boxes.  The MM-DiT, the processors, the
rectified-flow inversions and the transfer loop run on the native HIP library."""
import json
import os

import torch


def load_transformer(pretrained_model_path, weight_dtype=torch.float16):
    """``transformer/`` of a local SD3 / SD3.5 checkpoint folder -> the native CustomSD3Transformer2DModel (config.json keys are
    diffusers'; weights from *.safetensors under diffusers' parameter names)."""
    from ...backbones.video_diffusion_sd3.models.transformer_3D_model import CustomSD3Transformer2DModel
    root = os.path.join(pretrained_model_path, "transformer")
    with open(os.path.join(root, "config.json")) as f:
        cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
    keys = ("sample_size", "patch_size", "in_channels", "num_layers", "attention_head_dim", "num_attention_heads", "joint_attention_dim",
            "caption_projection_dim", "pooled_projection_dim", "out_channels", "pos_embed_max_size", "dual_attention_layers", "qk_norm")
    model = CustomSD3Transformer2DModel(**{k: cfg[k] for k in keys if k in cfg})
    from safetensors.torch import load_file
    sd = {}
    for fn in sorted(os.listdir(root)):
        if fn.endswith(".safetensors"):
            sd.update(load_file(os.path.join(root, fn)))
    model.load_state_dict(sd, strict=True)
    if weight_dtype != torch.float16:
        print(f"[univst_amd] the native MM-DiT computes in fp16; --weight_dtype {weight_dtype} applies to the stock VAE / text encoders only")
    return model.half().cuda().requires_grad_(False)


def load_t5_encoder(pretrained_model_path, subfolder, weight_dtype):
    """``UNIVST_T5_ENCODER=native``: the T5 encoder on the native library (fp16 with an fp32 residual stream, read from the local
    ``<model>/<subfolder>`` directory without importing the transformers model class).  Default ``stock``: transformers' T5EncoderModel, as the
    reference builds it."""
    mode = os.environ.get("UNIVST_T5_ENCODER", "stock")
    if mode not in ("stock", "native"):
        raise ValueError(f"UNIVST_T5_ENCODER={mode!r}: 'stock' or 'native'")
    if mode == "native":
        if weight_dtype != torch.float16:
            raise ValueError(f"UNIVST_T5_ENCODER=native computes in fp16 only; weight_dtype is {weight_dtype}")
        if not os.path.isdir(os.path.join(pretrained_model_path, subfolder)):
            raise FileNotFoundError(f"UNIVST_T5_ENCODER=native needs a local directory {os.path.join(pretrained_model_path, subfolder)}")
        from ...text import NativeT5Encoder
        return NativeT5Encoder.from_pretrained(pretrained_model_path, subfolder=subfolder)
    from transformers import T5EncoderModel
    return T5EncoderModel.from_pretrained(pretrained_model_path, subfolder=subfolder).requires_grad_(False)


def load_sd3_vae(pretrained_model_path, weight_dtype):
    """``UNIVST_SD3_VAE=native``: the 16-channel AutoencoderKL on the native library (fp16 with fp32 accumulation, read from the local ``<model>/vae``
    directory without importing diffusers; univst_amd.vae.NativeAutoencoderKL).  Default ``stock``: diffusers' AutoencoderKL, as the reference builds it."""
    mode = os.environ.get("UNIVST_SD3_VAE", "stock")
    if mode not in ("stock", "native"):
        raise ValueError(f"UNIVST_SD3_VAE={mode!r}: 'stock' or 'native'")
    if mode == "native":
        if weight_dtype != torch.float16:
            raise ValueError(f"UNIVST_SD3_VAE=native computes in fp16 only; weight_dtype is {weight_dtype}")
        if not os.path.isdir(os.path.join(pretrained_model_path, "vae")):
            raise FileNotFoundError(f"UNIVST_SD3_VAE=native needs a local directory {os.path.join(pretrained_model_path, 'vae')}")
        from ...vae import NativeAutoencoderKL
        return NativeAutoencoderKL.from_pretrained(pretrained_model_path, subfolder="vae")
    try:
        from diffusers import AutoencoderKL
    except ImportError as e:
        raise RuntimeError("UNIVST_SD3_VAE=stock (the default) needs `diffusers` for the SD3 VAE; UNIVST_SD3_VAE=native runs it on the native "
                           "library without diffusers") from e
    return AutoencoderKL.from_pretrained(pretrained_model_path, subfolder="vae").requires_grad_(False).to(weight_dtype).cuda()


def _flow_match_scheduler():
    """diffusers' FlowMatchEulerDiscreteScheduler where it can be imported, else the restated tables of univst_amd.schedulers (the arrangement
    src/sd/_common.py has for DDIM)"""
    try:
        from diffusers import FlowMatchEulerDiscreteScheduler
    except ImportError:
        from ...schedulers import FlowMatchEulerDiscreteScheduler
    return FlowMatchEulerDiscreteScheduler


def build_pipeline(pretrained_model_path, weight_dtype=torch.float16, qkv_dtype="fp16"):
    from transformers import CLIPTokenizer, T5TokenizerFast
    from ..sd._common import load_text_encoder
    from ...backbones.video_diffusion_sd3.pipelines.custom_pipeline import CustomStableDiffusion3Pipeline
    from ...backbones.video_diffusion_sd3.pnp_utils import CrossFrameProcessor
    vae = load_sd3_vae(pretrained_model_path, weight_dtype)        # first: the stock branch without diffusers fails before anything is loaded
    sub = lambda cls, name: cls.from_pretrained(pretrained_model_path, subfolder=name)          # noqa: E731
    transformer = load_transformer(pretrained_model_path, weight_dtype)
    transformer.set_attn_processor({n: CrossFrameProcessor() for n in transformer.attn_processors})      # run_*_sd3.py:58-69
    if getattr(transformer, "qkv_dtype", "fp16") != qkv_dtype:     # --qkv_dtype (an addition) decides here: it outranks UNIVST_SD3_QKV
        transformer.set_qkv_dtype(qkv_dtype)
    clip = lambda name: load_text_encoder(pretrained_model_path, name, weight_dtype, projected=True).to(weight_dtype).cuda()      # noqa: E731
    return CustomStableDiffusion3Pipeline(
        tokenizer=sub(CLIPTokenizer, "tokenizer"), tokenizer_2=sub(CLIPTokenizer, "tokenizer_2"), tokenizer_3=sub(T5TokenizerFast, "tokenizer_3"),
        text_encoder=clip("text_encoder"), text_encoder_2=clip("text_encoder_2"),
        text_encoder_3=load_t5_encoder(pretrained_model_path, "text_encoder_3", weight_dtype).to(weight_dtype).cuda(), vae=vae, transformer=transformer,
        scheduler=sub(_flow_match_scheduler(), "scheduler"))


def add_common_args(parser, weight_dtype=torch.float16):
    parser.add_argument("--pretrained_model_path", type=str, default="stabilityai/stable-diffusion-3.5-medium")
    parser.add_argument("--weight_dtype", type=torch.dtype, default=weight_dtype)
    parser.add_argument("--time_steps", type=int, default=50)
    parser.add_argument("--seed", type=int, default=33)
    # an addition to the reference's flags: the q | k | v projections of the MM-DiT in OCP MX-fp8 (CustomSD3Transformer2DModel.set_qkv_dtype)
    # (in these scripts the flag, given or not, outranks the UNIVST_SD3_QKV environment switch)
    parser.add_argument("--qkv_dtype", type=str, default="fp16", choices=("fp16", "mxfp8"))
    return parser
