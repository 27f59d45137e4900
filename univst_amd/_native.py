"""ctypes binding of libunivst_hip.so (include/univst.h).

There is NO fallback: if the shared library is missing or a call fails, a RuntimeError is raised.  torch is
used only as the owner of device memory and of the current HIP stream.
"""
import ctypes as C
import os
from typing import Optional

import torch

# UNIVST_LIB: another build of the same library (A/B measurements of kernel variants inside one process tree; tools/README.md)
_LIB_PATH = os.environ.get("UNIVST_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libunivst_hip.so")
_lib = None


class UnetCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("block_out_channels", C.c_int * 4),
                ("layers_per_block", C.c_int), ("cross_attention_dim", C.c_int), ("attention_heads", C.c_int * 4),
                ("norm_num_groups", C.c_int), ("norm_eps", C.c_float), ("flip_sin_to_cos", C.c_int),
                ("freq_shift", C.c_float)]


class ClipCfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int),
                ("max_positions", C.c_int), ("hidden_act", C.c_int), ("layer_norm_eps", C.c_float), ("projection_dim", C.c_int), ("eos_token_id", C.c_int)]


class T5Cfg(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("d_model", C.c_int), ("d_ff", C.c_int), ("num_layers", C.c_int), ("num_heads", C.c_int), ("d_kv", C.c_int),
                ("num_buckets", C.c_int), ("max_distance", C.c_int), ("layer_norm_eps", C.c_float)]


class MotionCfg(C.Structure):
    _fields_ = [("channels", C.c_int), ("num_heads", C.c_int), ("num_blocks", C.c_int), ("attn_per_block", C.c_int), ("norm_groups", C.c_int),
                ("max_len", C.c_int), ("position_encoding", C.c_int), ("gn_eps", C.c_float), ("ln_eps", C.c_float)]


class AnimateDiffCfg(C.Structure):
    _fields_ = [("inflated_groupnorm", C.c_int), ("motion_levels_mask", C.c_int), ("motion_mid_block", C.c_int), ("motion", MotionCfg)]


class VaeCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int), ("block_out_channels", C.c_int * 4),
                ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int)]


class KlVaeCfg(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int), ("block_out_channels", C.c_int * 4),
                ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int), ("use_quant_conv", C.c_int), ("use_post_quant_conv", C.c_int),
                ("attn_score_bytes", C.c_int64), ("pass_bytes", C.c_int64)]


class PnP(C.Structure):
    _fields_ = [("registered", C.c_int), ("idx", C.c_int), ("eta1", C.c_float), ("eta2", C.c_float),
                ("alpha", C.c_float), ("gamma", C.c_float)]


class Sd3AttnWeights(C.Structure):
    _NAMES = ("to_q", "to_q_bias", "to_k", "to_k_bias", "to_v", "to_v_bias", "norm_q", "norm_k", "add_q", "add_q_bias", "add_k", "add_k_bias",
              "add_v", "add_v_bias", "norm_added_q", "norm_added_k", "to_out", "to_out_bias", "to_add_out", "to_add_out_bias")
    _fields_ = [(n, C.c_void_p) for n in _NAMES]


class Sd3MxWeights(C.Structure):
    _fields_ = [("qkv", C.c_void_p), ("qkv_scale", C.c_void_p), ("add_qkv", C.c_void_p), ("add_qkv_scale", C.c_void_p)]


class Sd3GatedResidual(C.Structure):
    _fields_ = [("res_img", C.c_void_p), ("gate_img", C.c_void_p), ("res_txt", C.c_void_p), ("gate_txt", C.c_void_p), ("ld_gate_img", C.c_int64),
                ("ld_gate_txt", C.c_int64)]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int)
KVEXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64)

# name -> (restype, argtypes); kept in sync with include/univst.h (tests/test_abi.py checks both ways)
_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
SIGNATURES = {
    "univst_last_error": (C.c_char_p, []),
    "univst_abi_version": (_I, []),
    "univst_sd3_shift_window": (_I, [_I, C.c_double, C.c_double, C.POINTER(_I), C.POINTER(_F)]),
    "univst_unet_create": (_I, [C.POINTER(UnetCfg), C.POINTER(_P)]),
    "univst_unet_create_animatediff": (_I, [C.POINTER(UnetCfg), C.POINTER(AnimateDiffCfg), C.POINTER(_P)]),
    "univst_unet_destroy": (_I, [_P]),
    "univst_unet_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(_L), _I, _P]),
    "univst_unet_finalize": (_I, [_P, _P]),
    "univst_unet_reserve": (_I, [_P, _I, _I, _I, _I]),
    "univst_unet_forward": (_I, [_P, _P, _F, _P, _I, _I, _I, _I, _I, C.POINTER(PnP), _P, _P, _I, _P]),
    "univst_unet_forward_tap": (_I, [_P, _P, _F, _P, _I, _I, _I, _I, _I, C.POINTER(PnP), _P, _P, _I, _P]),
    "univst_unet_style_bank_bytes": (_L, [_P, _I, _I]),
    "univst_unet_style_bank": (_I, [_P, _P, _F, _P, _I, _I, _I, C.POINTER(PnP), _P, _L, C.POINTER(_I), _P]),
    "univst_unet_forward_static_style": (_I, [_P, _P, _F, _P, _I, _I, _I, _I, C.POINTER(PnP), _P, _L, _P, _P]),
    "univst_unet_set_comm": (_I, [_P, _I, _I, _P, _L, ALLREDUCE_FN, KVEXCHANGE_FN, _P]),
    "univst_unet_set_option": (_I, [_P, C.c_char_p, _I]),
    "univst_unet_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "univst_comm_create": (_I, [_I, _I, _L, C.POINTER(_P)]),
    "univst_comm_handle_bytes": (_I, []),
    "univst_comm_export": (_I, [_P, _P]),
    "univst_comm_connect": (_I, [_P, _P]),
    "univst_comm_connect_local": (_I, [_P, C.POINTER(_P)]),
    "univst_comm_connect_emulated": (_I, [_P, C.c_double, C.c_double]),
    "univst_comm_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "univst_comm_destroy": (_I, [_P]),
    "univst_comm_allreduce_f32": (_I, [_P, _P, _I, _P]),
    "univst_comm_status": (_I, [_P]),
    "univst_unet_set_comm_native": (_I, [_P, _P]),
    "univst_linear": (_I, [_P, _L, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _P]),
    "univst_mxfp8_quantize": (_I, [_P, _L, _L, _I, _P, _P, _P]),
    "univst_linear_mxfp8": (_I, [_P, _P, _P, _P, _P, _P, _L, _L, _I, _I, _P]),
    "univst_linear_ln": (_I, [_P, _L, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _P, _F, _P, _P, _P, _P]),
    "univst_geglu_xres_permute": (_I, [_P, _P, _I, _I, _P]),
    "univst_frag_pack": (_I, [_P, _P, _I, _I, _P]),
    "univst_vae_create": (_I, [_P, C.POINTER(_P)]),
    "univst_vae_destroy": (_I, [_P]),
    "univst_vae_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I, _P]),
    "univst_vae_finalize": (_I, [_P, _P]),
    "univst_vae_decode": (_I, [_P, _P, _L, _I, _I, _I, _P, _P]),
    "univst_vae_encode": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "univst_klvae_create": (_I, [_P, C.POINTER(_P)]),
    "univst_klvae_destroy": (_I, [_P]),
    "univst_klvae_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I, _P]),
    "univst_klvae_finalize": (_I, [_P, _P]),
    "univst_klvae_decode": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "univst_klvae_encode": (_I, [_P, _P, _L, _I, _I, _P, _P]),
    "univst_klvae_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "univst_clip_create": (_I, [_P, C.POINTER(_P)]),
    "univst_clip_destroy": (_I, [_P]),
    "univst_clip_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I, _P]),
    "univst_clip_finalize": (_I, [_P, _P]),
    "univst_clip_encode": (_I, [_P, _P, _I, _I, _P, _P, _P, _P]),
    "univst_clip_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "univst_clip_attention": (_I, [_P, _I, _I, _I, _P, _P]),
    "univst_t5_create": (_I, [_P, C.POINTER(_P)]),
    "univst_t5_destroy": (_I, [_P]),
    "univst_t5_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I, _P]),
    "univst_t5_finalize": (_I, [_P, _P]),
    "univst_t5_encode": (_I, [_P, _P, _I, _I, _P, _P]),
    "univst_t5_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "univst_motion_create": (_I, [_P, C.POINTER(_P)]),
    "univst_motion_destroy": (_I, [_P]),
    "univst_motion_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I, _P]),
    "univst_motion_finalize": (_I, [_P, _P]),
    "univst_motion_forward": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "univst_motion_query": (_I, [_P, C.c_char_p, C.POINTER(C.c_double)]),
    "univst_temporal_attention": (_I, [_P, C.c_int64, _P, _I, _I, _I, _I, _I, _P, C.c_int64, _P]),
    "univst_t5_attention": (_I, [_P, _P, _I, _I, _I, _P, _P]),
    "univst_debug_t5_buckets": (_I, [_I, _I, _I, C.POINTER(_I)]),
    "univst_raft_create": (_I, [C.POINTER(_P)]),
    "univst_raft_destroy": (_I, [_P]),
    "univst_raft_load_tensor": (_I, [_P, C.c_char_p, _P, _I, C.POINTER(C.c_int64), _I, _P]),
    "univst_raft_forward": (_I, [_P, _P, _P, _I, _I, _P, _P]),
    "univst_raft_encode": (_I, [_P, _P, _P, _I, _I, _P, _P, _P, _P]),
    "univst_raft_gru": (_I, [_P, _P, _P, _P, _I, _I, _P]),
    "univst_raft_pyramid_floats": (_L, [_I, _I]),
    "univst_raft_corr_pyramid": (_I, [_P, _P, _I, _I, _P, _P]),
    "univst_raft_corr_lookup": (_I, [_P, _P, _I, _I, _P, _P, _P]),
    "univst_raft_convex_upsample": (_I, [_P, _P, _I, _I, _P, _P]),
    "univst_attn2_fused_workspace_bytes": (_L, [_I, _I, _I]),
    "univst_attn12_fused": (_I, [_P, _L, _P, _P, _P, _L, _F, _P, _P, _P, _I, _P, _I, _I, _L, _P, _P, _P, _L, _L, _I, _I, _P, _P, _P]),
    "univst_attn2_fused": (_I, [_P, _L, _P, _F, _P, _P, _P, _I, _P, _I, _I, _L, _P, _P, _P, _L, _P, _L, _L, _I, _I, _P, _P, _P]),
    "univst_conv_nhwc": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _I, _P]),
    "univst_conv_nhwc_tapinner": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _I, _P]),
    "univst_conv3x3_patch": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P, _I, _P]),
    "univst_conv_up2_phase_weights": (_I, [_P, _I, _I, _P, _P]),
    "univst_linear_compose": (_I, [_P, _P, _P, _P, _P, _I, _I, _P, _P, _P]),
    "univst_conv3x3_up2_phase": (_I, [_P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _I, _P]),
    "univst_groupnorm_fold_linear": (_I, [_P, _I, _L, _I, _I, _F, _P, _P, _P, _P, _I, _P, _P, _P, _P]),
    "univst_linear_sets": (_I, [_P, _L, _P, _P, _I, _P, _L, _P, _L, _I, _I, _I, _P, _P]),
    "univst_groupnorm_workspace_bytes": (_L, [_L, _I, _I]),
    "univst_groupnorm_nhwc": (_I, [_P, _P, _I, _I, _L, _I, _I, _F, _P, _P, _I, _P, _P, _P]),
    "univst_layernorm": (_I, [_P, _P, _P, _P, _L, _I, _F, _P]),
    "univst_attention": (_I, [_P, _L, _P, _P, _L, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P]),
    "univst_attention_phase": (_I, [_P, _L, _P, _P, _L, _P, _L, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P]),
    "univst_sd3_joint_attention": (_I, [C.POINTER(Sd3AttnWeights), _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P,
                                        C.POINTER(Sd3GatedResidual), _P, _P]),
    "univst_sd3_joint_attention_mx": (_I, [C.POINTER(Sd3AttnWeights), _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P,
                                           C.POINTER(Sd3GatedResidual), _P, _P, C.POINTER(Sd3MxWeights)]),
    "univst_sd3_adain_shift": (_I, [_P, _L, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "univst_sd3_adain_shift_static": (_I, [_P, _L, _P, _L, _I, _I, _I, _I, _F, _F, _F, _P, _P]),
    "univst_sd3_joint_attention_static": (_I, [C.POINTER(Sd3AttnWeights), _P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _F, _P, _P,
                                               C.POINTER(Sd3GatedResidual), _P, C.POINTER(Sd3MxWeights), _P, _L, _I]),
    "univst_rmsnorm_heads": (_I, [_P, _L, _L, _I, _I, _P, _F, _P]),
    "univst_rmsnorm_heads_pair": (_I, [_P, _L, _L, _I, _I, _L, _P, _L, _P, _F, _F, _P]),
    "univst_linear_gated": (_I, [_P, _L, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _P, _L, _I, _P]),
    "univst_linear_epi": (_I, [_P, _L, _P, _P, _P, _L, _P, _L, _I, _I, _I, _I, _P, _I, _L, _P, _P, _L, _P]),
    "univst_adaln_modulate": (_I, [_P, _P, _P, _P, _L, _L, _L, _I, _F, _P, _P, _P, _P]),
    "univst_gate_residual": (_I, [_P, _P, _L, _P, _P, _L, _L, _I, _P]),
    "univst_activation": (_I, [_P, _P, _L, _I, _P]),
    "univst_timestep_embedding": (_I, [_P, _P, _I, _I, _I, _F, _F, _P]),
    "univst_sd3_patchify": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "univst_sd3_unpatchify": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "univst_axpbypcz": (_I, [_P, _P, _P, _P, _F, _F, _F, _L, _P]),
    "univst_attention_adain_shift": (_I, [_P, _L, _I, _I, _I, _F, _F, _F, _P, _P]),
    "univst_attention_adain_shift_static": (_I, [_P, _L, _P, _L, _I, _I, _I, _F, _F, _F, _P, _P]),
    "univst_latent_adain": (_I, [_P, _P, _P, _I, _I, _I, _P]),
    "univst_latent_adain_stats": (_I, [_P, _P, _I, _I, _I, _P]),
    "univst_latent_adain_apply": (_I, [_P, _P, _P, _L, _P, _I, _I, _I, _P]),
    "univst_axpby": (_I, [_P, _P, _P, _F, _F, _L, _P]),
    "univst_mask_blend": (_I, [_P, _P, _P, _P, _I, _L, _P]),
    "univst_mask_resize": (_I, [_P, _P, _I, _I, _I, _I, _I, _P]),
    "univst_maskprop_workspace_bytes": (_L, [_I, _I, _I]),
    "univst_maskprop_frame": (_I, [_P, _P, _P, _P, _I, _I, _I, _I, _F, _I, _P, _P]),
    "univst_maskprop_finalize": (_I, [_P, _P, _I, _I, _I, _I, _I, _P, _P]),
    "univst_warp_accumulate": (_I, [_P, _P, _P, _P, _P, _I, _I, _F, _P]),
    "univst_warp_window_key": (_I, [_P, _P, _I, _I, _I, _I, _I, _I, _F, _P]),
    "univst_latent_window_smooth": (_I, [_P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "univst_accumulate_u8": (_I, [_P, _P, _L, _P]),
    "univst_window_store": (_I, [_P, _F, _P, _L, _P]),
    "univst_debug_tr16": (_I, [_P, _P]),
    "univst_debug_delay_us": (_I, [C.c_double, _P]),
    "univst_debug_gemm_plan": (_I, [_I] * 16 + [C.c_char_p, _I]),
    "univst_debug_attention_plan": (_I, [_I] * 9 + [C.c_char_p, _I]),
    "univst_debug_groupnorm_plan": (_I, [_I, _I, _L, _I, _I, _I, _I, _I, _P]),
    "univst_profile_enable": (_I, [_I]),
    "univst_profile_symbols": (_I, [_I, C.c_char_p, _I]),
    "univst_profile_collect": (_I, [C.POINTER(C.c_double), C.POINTER(_L), C.POINTER(C.c_double), C.POINTER(C.c_double), _I]),
    "univst_profile_collect_aux": (_I, [C.POINTER(C.c_double), _I]),
}


ABI_VERSION = 3      # include/univst.h UNIVST_ABI_VERSION


def lib_path() -> str:
    return _LIB_PATH


def load():
    """Load the shared library (no GPU needed for loading)."""
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} not found: build it with `python __graft_entry__.py build` (or `make`); "
                               "univst_amd has no CPU or eager-PyTorch fallback")
        lib = C.CDLL(_LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.univst_abi_version() != ABI_VERSION:
            raise RuntimeError(f"{_LIB_PATH} has ABI version {lib.univst_abi_version()}, this binding was written against {ABI_VERSION} "
                               "(include/univst.h UNIVST_ABI_VERSION): rebuild the library (`make`)")
        _lib = lib
    return _lib


def check(rc: int, what: str = "", lib=None):
    if rc != 0:
        msg = (lib or load()).univst_last_error().decode(errors="replace")
        raise RuntimeError(f"libunivst_hip {what} failed (code {rc}): {msg}")


def stream_ptr() -> int:
    return torch.cuda.current_stream().cuda_stream


def ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _f16(t: torch.Tensor, name="tensor"):
    if not (t.is_cuda and t.dtype == torch.float16 and t.is_contiguous()):
        raise ValueError(f"{name}: expected a contiguous fp16 CUDA/HIP tensor, got {t.dtype} {t.device} "
                         f"contiguous={t.is_contiguous()}")
    return t


# --------------------------------------------------------------------------- model handles
def build_handle(lib, kind, create_args, items, stream, synchronize, *, other_dtype, device=None, create=None, load_what=None):
    """A loaded handle of ``univst_<kind>_*``: create (``create``: another entry than ``univst_<kind>_create``), one ``load_tensor`` per (key, tensor) of
    ``items`` on ``stream`` (the raw pointer), ``finalize`` where the ABI has one, and ``synchronize()`` for that stream, since the sources may be
    temporaries.  fp16 and fp32 tensors go up as they are, every other dtype as ``other_dtype``; ``device`` moves host tensors first.  Whatever raises on
    the way, the handle is destroyed before the exception goes on.  ``load_what``: the prefix of a failed load's message (default
    ``<kind>_load_tensor``).  ``lib``, ``stream`` and ``synchronize`` are arguments so that a stub can drive this without a GPU."""
    create = create or f"univst_{kind}_create"
    h = C.c_void_p()
    check(getattr(lib, create)(*create_args, C.byref(h)), create[len("univst_"):], lib)
    try:
        load_tensor, finalize = getattr(lib, f"univst_{kind}_load_tensor"), getattr(lib, f"univst_{kind}_finalize", None)
        for key, t in items:
            t = t.detach() if device is None else t.detach().to(device=device)
            t = t.to(t.dtype if t.dtype in (torch.float16, torch.float32) else other_dtype).contiguous()
            shape = (C.c_int64 * max(1, t.dim()))(*t.shape)      # (a 0-dim tensor still gets a valid pointer)
            check(load_tensor(h, key.encode(), t.data_ptr(), 0 if t.dtype == torch.float16 else 1, shape, t.dim(), stream),
                  f"{load_what or kind + '_load_tensor'}({key})", lib)
        if finalize is not None:
            check(finalize(h, stream), f"{kind}_finalize", lib)
        synchronize()
    except BaseException:
        getattr(lib, f"univst_{kind}_destroy")(h)
        raise
    return h


def load_handle(kind, create_args, items, **kw):
    """``build_handle`` on the library and torch's current stream"""
    return build_handle(load(), kind, create_args, items, stream_ptr(), torch.cuda.current_stream().synchronize, **kw)


class NativeHandle:
    """What the wrappers of a model handle share: the handle ``_h`` of ``univst_<_kind>_*`` is destroyed with the object, ``query`` reads it out, and
    ``_gpu_only`` refuses what is not a device tensor (``_noun``: the model's name in that message)."""
    _kind = _noun = None
    _h = None

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            try:
                getattr(load(), f"univst_{self._kind}_destroy")(h)
            except Exception:      # interpreter shutdown: the module's own attributes may already be gone
                pass
            self._h = None

    def query(self, name):
        """a read-out of the handle (include/univst.h ``univst_<kind>_query``): ``arena_high_water``, ``arena_bytes``, ``weight_bytes`` and the handle's own"""
        out = C.c_double()
        check(getattr(load(), f"univst_{self._kind}_query")(self._h, name.encode(), C.byref(out)), f"{self._kind}_query({name})")
        return int(out.value)

    def _gpu_only(self, t, what):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.{what}: the native {self._noun} runs on the GPU only (no CPU / eager fallback); got "
                               f"{'a ' + str(t.device) + ' tensor' if torch.is_tensor(t) else type(t).__name__}")
        return t

    @staticmethod
    def merge_config(defaults, config, keep_none=False):
        """``defaults`` with the entries a dict or an object ``config`` has for its keys; other keys are dropped, and so are ``None`` values unless
        ``keep_none``"""
        cfg = dict(defaults)
        if config is not None:
            for k in defaults:
                if (k in config) if isinstance(config, dict) else hasattr(config, k):
                    v = config[k] if isinstance(config, dict) else getattr(config, k)
                    if v is not None or keep_none:
                        cfg[k] = v
        return cfg


class NativeModuleFacade(NativeHandle):
    """``NativeHandle`` plus what the call sites touch of an nn.Module, for the wrappers that are none"""

    @property
    def dtype(self):
        return torch.float16

    def to(self, *a, **k):
        return self

    def cuda(self, *a, **k):
        return self

    def requires_grad_(self, *a, **k):
        return self

    def eval(self):
        return self


# --------------------------------------------------------------------------- stand-alone operator wrappers
def temporal_attention(qkv, B, F, N, heads, head_dim, pe_qkv=None, out=None):
    """softmax attention along the frame axis (univst_temporal_attention): qkv fp16 [B*F*N, >= 3*heads*head_dim] rows q | k | v in the order
    (b*F + f)*N + n (row stride = qkv.stride(0); q carries the score scale), pe_qkv None or fp16 [F, 3*heads*head_dim] -> out fp16
    [B*F*N, heads*head_dim] (or the rows of a given ``out``, stride out.stride(0))."""
    Cw = heads * head_dim
    if out is None:
        out = torch.empty(qkv.shape[0], Cw, device=qkv.device, dtype=torch.float16)
    for name, t in (("qkv", qkv), ("out", out)):
        if not (t.is_cuda and t.dtype == torch.float16 and t.dim() == 2 and t.stride(1) == 1):
            raise ValueError(f"temporal_attention: {name} must be fp16 CUDA/HIP rows with contiguous columns, got {t.dtype} {t.device} strides {t.stride()}")
    if qkv.shape[0] < B * F * N or out.shape[0] < B * F * N:
        raise ValueError(f"temporal_attention: B*F*N = {B * F * N} rows, qkv has {qkv.shape[0]} and out {out.shape[0]}")
    if pe_qkv is not None:
        _f16(pe_qkv, "pe_qkv")
        if tuple(pe_qkv.shape) != (F, 3 * Cw):
            raise ValueError(f"temporal_attention: pe_qkv must be [F, 3*heads*head_dim] = [{F}, {3 * Cw}], got {tuple(pe_qkv.shape)}")
    check(load().univst_temporal_attention(ptr(qkv), qkv.stride(0), ptr(pe_qkv), B, F, N, heads, head_dim, ptr(out), out.stride(0), stream_ptr()),
          "temporal_attention")
    return out


def linear(x, w, bias=None, residual=None, geglu=False, out=None):
    """y[M,N] = x[M,K] w[N,K]^T (+bias)(+residual); geglu: w/bias rows pre-interleaved (True / 1: [16 x | 16 gate] blocks; 2: the
    X-resident order for K = 320, see geglu_xres_permute), N/2 output columns."""
    _f16(x), _f16(w)
    M, K = x.shape
    N = w.shape[0]
    No = N // 2 if geglu else N
    if out is None:
        out = torch.empty(M, No, device=x.device, dtype=torch.float16)
    check(load().univst_linear(ptr(x), K, ptr(w), ptr(bias), ptr(residual), No, ptr(out), No, M, N, K, int(geglu),
                               stream_ptr()), "linear")
    return out


def mxfp8_quantize(x):
    """OCP MX quantisation of fp16 rows (include/univst.h univst_mxfp8_quantize): x fp16 [rows, K] with unit column stride (a column slice of a wider
    buffer is fine) -> (e4m3fn bytes uint8 [rows, K], E8M0 scale bytes uint8 [rows, K/32])."""
    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError(f"mxfp8_quantize: expected fp16 CUDA/HIP rows with contiguous columns, got {x.dtype} {x.device} strides {tuple(x.stride())}")
    rows, K = x.shape
    if K % 32:
        raise ValueError(f"mxfp8_quantize: K = {K} is not a multiple of the 32-element MX block")
    q = torch.empty(rows, K, device=x.device, dtype=torch.uint8)
    s = torch.empty(rows, K // 32, device=x.device, dtype=torch.uint8)
    check(load().univst_mxfp8_quantize(ptr(x), x.stride(0), rows, K, ptr(q), ptr(s), stream_ptr()), "mxfp8_quantize")
    return q, s


def linear_mxfp8(xq, xs, wq, ws, bias=None, out=None):
    """y[M,N] = deq(xq, xs) deq(wq, ws)^T (+bias) on the block-scaled MFMA (univst_linear_mxfp8): xq [M, K] / wq [N, K] e4m3fn bytes, xs [M, K/32] /
    ws [N, K/32] scale bytes (what mxfp8_quantize returns), bias fp16 [N] -> fp16 [M, N], or the rows of a given ``out`` (stride out.stride(0))."""
    for name, t in (("xq", xq), ("xs", xs), ("wq", wq), ("ws", ws)):
        if not (t.is_cuda and t.dtype == torch.uint8 and t.dim() == 2 and t.is_contiguous()):
            raise ValueError(f"linear_mxfp8: {name} must be a contiguous uint8 CUDA/HIP matrix, got {t.dtype} {t.device} {tuple(t.shape)}")
    M, K = xq.shape
    N = wq.shape[0]
    if wq.shape[1] != K or tuple(xs.shape) != (M, K // 32) or tuple(ws.shape) != (N, K // 32):
        raise ValueError(f"linear_mxfp8: xq {tuple(xq.shape)} xs {tuple(xs.shape)} wq {tuple(wq.shape)} ws {tuple(ws.shape)} do not fit together")
    if bias is not None:
        _f16(bias, "bias")
    if out is None:
        out = torch.empty(M, N, device=xq.device, dtype=torch.float16)
    elif not (out.is_cuda and out.dtype == torch.float16 and out.dim() == 2 and out.stride(1) == 1 and out.shape[0] >= M and out.shape[1] >= N):
        raise ValueError(f"linear_mxfp8: out must be fp16 CUDA/HIP rows [>= {M}, >= {N}] with contiguous columns")
    check(load().univst_linear_mxfp8(ptr(xq), ptr(xs), ptr(wq), ptr(ws), ptr(bias), ptr(out), out.stride(0), M, N, K, stream_ptr()), "linear_mxfp8")
    return out


def linear_epi(x, w, bias=None, residual=None, rowbias=None, rows_per_rowbias=1, bias2=None, workspace=None, out=None):
    """y[M,N] = fp16(fp16(x w^T + bias + rowbias[m // rows_per_rowbias] + residual) + bias2) (univst_linear_epi); rowbias a [B, N] row view;
    workspace: a float32 tensor for the partials of a split-K launch (too small: the launcher takes its own scratch)."""
    _f16(x), _f16(w)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float16)
    check(load().univst_linear_epi(ptr(x), K, ptr(w), ptr(bias), ptr(residual), N, ptr(out), N, M, N, K, 0, ptr(rowbias), rows_per_rowbias,
                                   0 if rowbias is None else rowbias.stride(0), ptr(bias2), ptr(workspace),
                                   0 if workspace is None else workspace.numel() * workspace.element_size(), stream_ptr()), "linear_epi")
    return out


def linear_gated(x, w, bias=None, residual=None, act=None, gate=None, rows_per_gate=1, out=None):
    """y[M,N] = residual + gate[m // rows_per_gate] * act(x w^T + bias); act None or ACT_GELU_TANH; gate a [B, N] row view."""
    _f16(x), _f16(w)
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, device=x.device, dtype=torch.float16)
    check(load().univst_linear_gated(ptr(x), K, ptr(w), ptr(bias), ptr(residual), N, ptr(out), N, M, N, K, -1 if act is None else act,
                                     ptr(gate), 0 if gate is None else _mod_ld(gate), rows_per_gate, stream_ptr()), "linear_gated")
    return out


def geglu_xres_permute(w):
    """GEGLU projection weight [N, K] (or bias [N]) from the checkpoint's [x rows | gate rows] order into the row order ``linear(...,
    geglu=2)`` expects (the X-resident kernel for K = 320)."""
    _f16(w)
    w = w.contiguous()
    out = torch.empty_like(w)
    check(load().univst_geglu_xres_permute(ptr(w), ptr(out), w.shape[0], 1 if w.dim() == 1 else w.shape[1], stream_ptr()), "geglu_xres_permute")
    return out


def frag_pack(w):
    """[N, K] weight -> MFMA A-operand order [N/16][K/32][64][8] (same numel)."""
    _f16(w)
    w = w.contiguous()
    out = torch.empty_like(w)
    check(load().univst_frag_pack(ptr(w), ptr(out), w.shape[0], w.shape[1], stream_ptr()), "frag_pack")
    return out


def attn2_fused(x, wq_frag, kv, wo_frag, bias_o, rows_per_branch, heads, residual=None, ln=None, q_prescaled=False, stats_out=None, out=None,
                eps=1e-5):
    """The text cross-attention of a transformer block in one launch: x [M, C] (raw rows when ``ln = (stats [M, C/160, 2], wsum [C], lnb [C])``
    folds the LayerNorm), kv [B*T, 2C] text K | V rows -> to_out(attention) + bias + residual (default: x)."""
    _f16(x), _f16(wq_frag), _f16(kv), _f16(wo_frag)
    M, C_ = x.shape
    B = -(-M // rows_per_branch)
    T = kv.shape[0] // B
    residual = x if residual is None else residual
    out = torch.empty(M, C_, device=x.device, dtype=torch.float16) if out is None else out
    st, ws, lb = ln if ln is not None else (None, None, None)
    for t in (st, ws, lb, stats_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    wsb = torch.empty(max(int(load().univst_attn2_fused_workspace_bytes(B, heads, C_ // heads)), 16), device=x.device, dtype=torch.uint8)
    check(load().univst_attn2_fused(ptr(x), x.stride(0), ptr(st), eps, ptr(ws), ptr(lb), ptr(wq_frag), int(q_prescaled), ptr(kv), B, T,
                                    rows_per_branch, ptr(wo_frag), ptr(bias_o), ptr(residual), residual.stride(0), ptr(out), out.stride(0), M, C_,
                                    heads, ptr(stats_out), ptr(wsb), stream_ptr()), "attn2_fused")
    return out


def attn12_fused(attn_out, wp_frag, bias_p, residual_in, wq_frag, wsum, lnb, kv, wo_frag, bias_o, rows_per_branch, heads, q_prescaled=False, stats_out=None,
                 eps=1e-5):
    """attn1.to_out + residual -> LayerNorm -> text cross-attention -> to_out + residual in one launch (univst_attn12_fused)."""
    _f16(attn_out), _f16(wp_frag), _f16(residual_in), _f16(wq_frag), _f16(kv), _f16(wo_frag)
    M, C_ = attn_out.shape
    B = -(-M // rows_per_branch)
    T = kv.shape[0] // B
    out = torch.empty(M, C_, device=attn_out.device, dtype=torch.float16)
    wsb = torch.empty(max(int(load().univst_attn2_fused_workspace_bytes(B, heads, C_ // heads)), 16), device=attn_out.device, dtype=torch.uint8)
    check(load().univst_attn12_fused(ptr(attn_out), attn_out.stride(0), ptr(wp_frag), ptr(bias_p), ptr(residual_in), residual_in.stride(0), eps, ptr(wsum), ptr(lnb),
                                     ptr(wq_frag), int(q_prescaled), ptr(kv), B, T, rows_per_branch, ptr(wo_frag), ptr(bias_o), ptr(out), out.stride(0), M, C_, heads,
                                     ptr(stats_out), ptr(wsb), stream_ptr()), "attn12_fused")
    return out


def linear_ln(x, w, bias=None, residual=None, geglu=False, out=None, ln=None, stats_out=None, eps=1e-5):
    """``linear`` through the LayerNorm-fold entry: ``stats_out`` fp32 [M, N/160, 2] receives the row statistics of the output;
    ``ln = (stats [M, K/160, 2], wsum [N], lnb [N])`` folds LayerNorm(x) into this linear (w = gamma-scaled weight)."""
    _f16(x), _f16(w)
    M, K = x.shape
    N = w.shape[0]
    No = N // 2 if geglu else N
    if out is None:
        out = torch.empty(M, No, device=x.device, dtype=torch.float16)
    st, ws, lb = ln if ln is not None else (None, None, None)
    for t in (st, ws, lb, stats_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    check(load().univst_linear_ln(ptr(x), K, ptr(w), ptr(bias), ptr(residual), No, ptr(out), No, M, N, K, int(geglu), ptr(st), eps,
                                  ptr(ws), ptr(lb), ptr(stats_out), stream_ptr()), "linear_ln")
    return out


def conv_nhwc(x1, w, bias=None, x2=None, upsample=False, stride=1, rowbias=None, rows_per_rowbias=1, residual=None):
    """x1 [imgs,Hs,Ws,C1] (+ x2 [imgs,Hs,Ws,C2]) NHWC, w [Cout,taps,C1+C2] -> [imgs,Ho,Wo,Cout]."""
    _f16(x1), _f16(w)
    imgs, Hs, Ws, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    Cout, taps, _ = w.shape
    He, We = (Hs * 2, Ws * 2) if upsample else (Hs, Ws)
    Ho = (He - 1) // stride + 1 if taps == 9 else He
    Wo = (We - 1) // stride + 1 if taps == 9 else We
    out = torch.empty(imgs, Ho, Wo, Cout, device=x1.device, dtype=torch.float16)
    check(load().univst_conv_nhwc(ptr(x1), ptr(x2), C1, C2, imgs, Hs, Ws, int(upsample), stride, taps, ptr(w), ptr(bias),
                                  ptr(rowbias), rows_per_rowbias, ptr(residual), ptr(out), Cout, stream_ptr()), "conv_nhwc")
    return out


def conv_nhwc_tapinner(x1, w_ti, bias=None, x2=None, upsample=False, stride=1, rowbias=None, rows_per_rowbias=1, residual=None):
    """3x3 conv with the tap-inner weight layout [Cout, Cin/64, 9, 64]."""
    _f16(x1), _f16(w_ti)
    imgs, Hs, Ws, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    Cout = w_ti.shape[0]
    He, We = (Hs * 2, Ws * 2) if upsample else (Hs, Ws)
    Ho, Wo = (He - 1) // stride + 1, (We - 1) // stride + 1
    out = torch.empty(imgs, Ho, Wo, Cout, device=x1.device, dtype=torch.float16)
    check(load().univst_conv_nhwc_tapinner(ptr(x1), ptr(x2), C1, C2, imgs, Hs, Ws, int(upsample), stride, ptr(w_ti), ptr(bias),
                                           ptr(rowbias), rows_per_rowbias, ptr(residual), ptr(out), Cout, stream_ptr()), "conv_tapinner")
    return out


def conv3x3_patch(x1, w_t32, bias=None, x2=None, rowbias=None, rows_per_rowbias=1, residual=None, upsample=False):
    """3x3 / stride-1 conv through the LDS-patch kernel, weight layout [Cout, Cin/32, 9, 32]; raises when the problem is
    not eligible for that kernel (it never falls back silently)."""
    _f16(x1), _f16(w_t32)
    imgs, Hs, Ws, C1 = x1.shape
    C2 = 0 if x2 is None else x2.shape[-1]
    Cout = w_t32.shape[0]
    He, We = (Hs * 2, Ws * 2) if upsample else (Hs, Ws)
    out = torch.empty(imgs, He, We, Cout, device=x1.device, dtype=torch.float16)
    check(load().univst_conv3x3_patch(ptr(x1), ptr(x2), C1, C2, imgs, Hs, Ws, int(upsample), ptr(w_t32), ptr(bias), ptr(rowbias), rows_per_rowbias,
                                      ptr(residual), ptr(out), Cout, stream_ptr()), "conv3x3_patch")
    return out


def linear_compose(wp, w2, b2, tb, bp):
    """Wp [C, C], W2 [C, K2], biases [C] (tb may be None) -> ([Wp W2 | Wp] as [C, K2 + C], Wp (b2 + tb) + bp as [C]): the second linear of a chain with a
    residual in between folded into the first one's K loop (fp32 accumulation, one fp16 rounding)."""
    for t in (wp, w2, b2, bp):
        _f16(t)
    C_, K2 = w2.shape
    w = torch.empty(C_, K2 + C_, device=wp.device, dtype=torch.float16)
    b = torch.empty(C_, device=wp.device, dtype=torch.float16)
    check(load().univst_linear_compose(ptr(wp.contiguous()), ptr(w2.contiguous()), ptr(b2), ptr(tb), ptr(bp), C_, K2, ptr(w), ptr(b), stream_ptr()),
          "linear_compose")
    return w, b


def conv_up2_phase_weights(w):
    """[Cout, Cin, 3, 3] -> the phase copy [4, Cout, Cin/32, 4, 32] of an upsampler conv: per phase (a, b) of the output pixel (2y+a, 2x+b) the sums of the
    original taps that fall on one of its 2x2 source pixels (fp32 sums, one fp16 rounding)."""
    _f16(w)
    Co, Ci = w.shape[:2]
    w4 = torch.empty(4, Co, Ci // 32, 4, 32, device=w.device, dtype=torch.float16)
    check(load().univst_conv_up2_phase_weights(ptr(w.contiguous()), Co, Ci, ptr(w4), stream_ptr()), "conv_up2_phase_weights")
    return w4


def conv3x3_up2_phase(x, w4, bias=None, gn_group_width=0):
    """3x3 conv over the nearest x2 upsampled x [imgs, Hs, Ws, C] as four 2x2-tap phase convs (conv_patch_kernel's phase mode) -> [imgs, 2Hs, 2Ws, Cout];
    with gn_group_width also the GroupNorm statistics [Cout / width, rows / 16, 2] of the stored rows.  Raises when the problem is not eligible."""
    _f16(x), _f16(w4)
    imgs, Hs, Ws, C_ = x.shape
    Cout = w4.shape[1]
    out = torch.empty(imgs, 2 * Hs, 2 * Ws, Cout, device=x.device, dtype=torch.float16)
    gst = torch.zeros(Cout // gn_group_width, imgs * 4 * Hs * Ws // 16, 2, device=x.device, dtype=torch.float32) if gn_group_width else None
    check(load().univst_conv3x3_up2_phase(ptr(x), C_, imgs, Hs, Ws, ptr(w4), ptr(bias), ptr(out), Cout, ptr(gst), gn_group_width, stream_ptr()),
          "conv3x3_up2_phase")
    return (out, gst) if gn_group_width else out


def groupnorm_fold_linear(x, gamma, beta, groups, eps, rows_per_stat, w, bias=None):
    """-> (W_sets [S, N, C] fp16, bias32 [S, N] fp32): the GroupNorm of x [rows, C] folded into the linear (w [N, C], bias) that consumes it."""
    _f16(x), _f16(w)
    rows, C_ = x.shape
    S, N = rows // rows_per_stat, w.shape[0]
    ws = torch.empty(max(1, load().univst_groupnorm_workspace_bytes(rows, rows_per_stat, groups) // 4), device=x.device, dtype=torch.float32)
    wsets = torch.empty(S, N, C_, device=x.device, dtype=torch.float16)
    b32 = torch.empty(S, N, device=x.device, dtype=torch.float32)
    check(load().univst_groupnorm_fold_linear(ptr(x), C_, rows, rows_per_stat, groups, eps, ptr(gamma), ptr(beta), ptr(w), ptr(bias), N, ptr(wsets), ptr(b32),
                                              ptr(ws), stream_ptr()), "groupnorm_fold_linear")
    return wsets, b32


def linear_sets(x, wsets, bias32, rows_per_set, residual=None, stats_out=None):
    _f16(x), _f16(wsets)
    M, K = x.shape
    N = wsets.shape[1]
    out = torch.empty(M, N, device=x.device, dtype=torch.float16)
    check(load().univst_linear_sets(ptr(x), K, ptr(wsets), ptr(bias32), rows_per_set, ptr(residual), N, ptr(out), N, M, N, K, ptr(stats_out), stream_ptr()), "linear_sets")
    return out


def groupnorm_nhwc(x1, gamma, beta, groups, eps, rows_per_stat, silu=False, x2=None):
    _f16(x1)
    C1 = x1.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    rows = x1.numel() // C1
    ws = torch.empty(max(1, load().univst_groupnorm_workspace_bytes(rows, rows_per_stat, groups) // 4), device=x1.device,
                     dtype=torch.float32)
    out = torch.empty(*x1.shape[:-1], C1 + C2, device=x1.device, dtype=torch.float16)
    check(load().univst_groupnorm_nhwc(ptr(x1), ptr(x2), C1, C2, rows, rows_per_stat, groups, eps, ptr(gamma), ptr(beta),
                                       int(silu), ptr(out), ptr(ws), stream_ptr()), "groupnorm")
    return out


def layernorm(x, gamma, beta, eps=1e-5):
    _f16(x)
    C_ = x.shape[-1]
    out = torch.empty_like(x)
    check(load().univst_layernorm(ptr(x), ptr(out), ptr(gamma), ptr(beta), x.numel() // C_, C_, eps, stream_ptr()),
          "layernorm")
    return out


def attention(q, k, v, src_idx, heads, ldq=None, ldkv=None, Nq=None, Nkv=None, C_=None, src_cnt=None, src_logw=None, q_prescaled=False):
    """q [BF,Nq,C], k/v [S,Nkv,C] (S source blocks), src_idx int32 [BF,nsrc] -> [BF,Nq,C].
    q_prescaled: q already multiplied by log2(e)/sqrt(head_dim)."""
    BF, Nq_, Cq = q.shape
    C_ = C_ or Cq
    out = torch.empty(BF, Nq_, C_, device=q.device, dtype=torch.float16)
    check(load().univst_attention(ptr(q), ldq or q.stride(1), ptr(k), ptr(v), ldkv or k.stride(1), ptr(out), C_,
                                  ptr(src_idx), ptr(src_cnt), ptr(src_logw), src_idx.shape[1], BF, Nq_, Nkv or k.shape[1], heads, C_ // heads,
                                  int(bool(q_prescaled)), stream_ptr()), "attention")
    return out


def attention_phase(q, k, v, src_idx, src_cnt, heads, out=None, state_out=None, state_in=None, ldq=None, ldkv=None, Nq=None, Nkv=None, C_=None, src_logw=None,
                    q_prescaled=False):
    """one launch of a TWO-PHASE attention (include/univst.h univst_attention_phase): phase 1 returns (out, state) with state [BF, heads, Nq, 2] fp32;
    phase 2 takes them (state_in=, out=) and returns the merged rows in `out`."""
    BF, Nq_, Cq = q.shape[0], (Nq or q.shape[1]), q.shape[2]
    C_ = C_ or Cq
    if out is None:
        out = torch.empty(BF, Nq_, C_, device=q.device, dtype=torch.float16)
    first = state_in is None
    if first and state_out is None:
        state_out = torch.empty(BF, heads, Nq_, 2, device=q.device, dtype=torch.float32)
    check(load().univst_attention_phase(ptr(q), ldq or q.stride(1), ptr(k), ptr(v), ldkv or k.stride(1), ptr(out), C_,
                                        ptr(src_idx), ptr(src_cnt), ptr(src_logw), src_idx.shape[1], BF, Nq_, Nkv or k.shape[1], heads, C_ // heads,
                                        int(bool(q_prescaled)), ptr(state_out) if first else None, None if first else ptr(state_in), stream_ptr()), "attention_phase")
    return (out, state_out) if first else out


_SD3_KEYS = {"to_q": "to_q.weight", "to_q_bias": "to_q.bias", "to_k": "to_k.weight", "to_k_bias": "to_k.bias", "to_v": "to_v.weight",
             "to_v_bias": "to_v.bias", "norm_q": "norm_q.weight", "norm_k": "norm_k.weight", "add_q": "add_q_proj.weight",
             "add_q_bias": "add_q_proj.bias", "add_k": "add_k_proj.weight", "add_k_bias": "add_k_proj.bias", "add_v": "add_v_proj.weight",
             "add_v_bias": "add_v_proj.bias", "norm_added_q": "norm_added_q.weight", "norm_added_k": "norm_added_k.weight",
             "to_out": "to_out.0.weight", "to_out_bias": "to_out.0.bias", "to_add_out": "to_add_out.weight", "to_add_out_bias": "to_add_out.bias"}


class Sd3AttnParams(dict):
    """the fp16 device tensors behind a univst_sd3_attn_weights struct, keyed by its field names.  q | k | v (and the added
    q | k | v) weights and biases are kept as views of ONE [3C, Cin] / [3C] tensor each, so that the library runs one projection
    per stream (csrc/sd3.hip checks that the three pointers are consecutive).  Build once per attention module and pass it in
    place of the state dict (backbones/video_diffusion_sd3/pnp_utils.py caches it, keyed by the parameters' storage and version)."""

    def __init__(self, state, device):
        super().__init__()
        t = {k: state[v].detach().to(device=device, dtype=torch.float16).contiguous() for k, v in _SD3_KEYS.items() if state.get(v) is not None}
        for trio in (("to_q", "to_k", "to_v"), ("add_q", "add_k", "add_v")):
            for suf in ("", "_bias"):
                names = [n + suf for n in trio]
                if all(n in t for n in names) and len({tuple(t[n].shape) for n in names}) == 1:
                    fused = torch.cat([t[n] for n in names]).contiguous()
                    rows = t[names[0]].shape[0]
                    for i, n in enumerate(names):
                        t[n] = fused[i * rows:(i + 1) * rows]
        self.update(t)
        self._mx = None

    def _fused_rows(self, first):
        """the [3C, Cin] tensor the three views first | k | v are slices of, or None when they are not consecutive"""
        q = self.get(first)
        if q is None:
            return None
        k, v = self.get(first.replace("q", "k")), self.get(first.replace("q", "v"))
        step = q.numel() * q.element_size()
        if k is None or v is None or k.data_ptr() - q.data_ptr() != step or v.data_ptr() - k.data_ptr() != step:
            return None
        return torch.as_strided(q, (3 * q.shape[0], q.shape[1]), (q.shape[1], 1))

    def mx(self):
        """the MX-fp8 copies of the fused q | k | v weights (``univst_sd3_mx_weights``), quantised on first use and kept with this object: a rebuild of
        the fp16 tensors is a new Sd3AttnParams, and so a new quantisation.  -> dict(qkv, qkv_scale[, add_qkv, add_qkv_scale]) of uint8 tensors."""
        if self._mx is None:
            w = self._fused_rows("to_q")
            if w is None:
                raise RuntimeError("Sd3AttnParams.mx: MX-fp8 q | k | v needs to_q / to_k / to_v of one shape (the fused [3C, Cin] layout)")
            if w.shape[1] % 128:
                raise RuntimeError(f"Sd3AttnParams.mx: MX-fp8 q | k | v needs an input width that is a multiple of 128, got {w.shape[1]}")
            mx = {}
            mx["qkv"], mx["qkv_scale"] = mxfp8_quantize(w)
            a = self._fused_rows("add_q")
            if a is not None:
                mx["add_qkv"], mx["add_qkv_scale"] = mxfp8_quantize(a)
            self._mx = mx
        return self._mx


def sd3_joint_attention(params, hidden, enc, heads, clip_length=16, shift=False, idx=-1, eta1=0.0, eta2=0.6, rms_eps=1e-6, fuse=None, comm=None,
                        qkv_dtype="fp16", style_kv=None, static_role=None):
    """CrossFrameProcessor / AttentionShiftProcessor of the reference's SD3 plugin on the native kernels.  params: the state dict
    of diffusers' Attention module (to_q.weight, ..., to_add_out.bias; missing entries = absent).  hidden [B, N, Cin],
    enc [B, Nt, Cin] or None -> (img [B, N, Cin], txt [B, Nt, Cin]) or img alone.  clip_length 0: no cross-frame keys.
    fuse (optional): dict(res_img, gate_img[, res_txt, gate_txt]) — the block's gated residuals computed in the out-projections'
    epilogue: the returned tensors are then res + gate[:, None] * attention output.
    comm (optional): pointer of a connected univst_comm — the batch is this rank's clip_length frames of every branch (frame shard).
    qkv_dtype: "fp16", or "mxfp8" for the two q | k | v projections on the block-scaled fp8 MFMA (univst_sd3_joint_attention_mx; params' quantised
    weights are made on first use; input width a multiple of 128, no frame shard).
    static_role (optional, univst_sd3_joint_attention_static): 0 = the bank call — the ordinary joint attention of the style frame, which also writes
    frame 0's post-norm K | V image rows into ``style_kv`` [N, >= 2C] (fp16, unit column stride; no shift); 1 = the apply call — the batch is
    [content | stylised] (B = 2 * clip_length) and, inside the window, the shift runs against ``style_kv`` (outside it ``style_kv`` may be None).
    No communicator in either role."""
    if static_role is not None:
        if static_role not in (0, 1):
            raise ValueError(f"sd3_joint_attention: static_role must be None, 0 (bank) or 1 (apply), got {static_role!r}")
        if comm is not None:
            raise ValueError("sd3_joint_attention: static_role and comm (a frame shard) cannot be combined")
        if style_kv is not None and not (style_kv.is_cuda and style_kv.dtype == torch.float16 and style_kv.dim() == 2 and style_kv.stride(1) == 1
                                         and style_kv.shape[0] == hidden.shape[1]):
            raise ValueError(f"sd3_joint_attention: style_kv must be an fp16 CUDA/HIP [N = {hidden.shape[1]}, >= 2C] tensor or row view with a unit "
                             f"column stride, got {style_kv.dtype} {tuple(style_kv.shape)} strides {tuple(style_kv.stride())}")
    elif style_kv is not None:
        raise ValueError("sd3_joint_attention: style_kv needs static_role")
    if qkv_dtype not in ("fp16", "mxfp8"):
        raise ValueError(f"sd3_joint_attention: qkv_dtype must be 'fp16' or 'mxfp8', got {qkv_dtype!r}")
    _f16(hidden)
    B, N, Cin = hidden.shape
    keep = params if isinstance(params, Sd3AttnParams) else Sd3AttnParams(params, hidden.device)
    w = Sd3AttnWeights(**{k: (keep[k].data_ptr() if k in keep else None) for k in Sd3AttnWeights._NAMES})
    inner = keep["to_q"].shape[0]
    out_i = torch.empty_like(hidden)
    Nt = 0
    out_t = None
    if enc is not None:
        _f16(enc)
        Nt = enc.shape[1]
        out_t = torch.empty(B, Nt, Cin if "to_add_out" in keep else inner, device=hidden.device, dtype=torch.float16)
    gr = None
    if fuse is not None:
        gt = fuse.get("gate_txt")
        gr = Sd3GatedResidual(ptr(_f16(fuse["res_img"])), ptr(fuse["gate_img"]), ptr(fuse.get("res_txt")), ptr(gt), _mod_ld(fuse["gate_img"]),
                              0 if gt is None else _mod_ld(gt))
    # pnp_utils.py:183-186 in Python double, like the reference: in fp32 eta1 = 0.3 gives 0.3f * 50 = 15.000001 and idx 15 drops out
    active = bool(shift) and idx >= eta1 * 50 and idx <= eta2 * 50
    beta = ((0.9 - 0.1) / (eta1 * 50 - eta2 * 50) * (idx - eta2 * 50) + 0.1) if active else 0.0
    args = (C.byref(w), ptr(hidden), ptr(enc), B, N, Nt, Cin, heads, inner // heads, clip_length, int(active), float(beta), rms_eps, ptr(out_i),
            ptr(out_t), C.byref(gr) if gr is not None else None, comm, stream_ptr())
    mx = None
    if qkv_dtype == "mxfp8":
        m = keep.mx()
        mx = Sd3MxWeights(ptr(m["qkv"]), ptr(m["qkv_scale"]), ptr(m.get("add_qkv")), ptr(m.get("add_qkv_scale")))
    if static_role is not None:
        check(load().univst_sd3_joint_attention_static(*args[:-2], stream_ptr(), C.byref(mx) if mx is not None else None, ptr(style_kv),
                                                       0 if style_kv is None else style_kv.stride(0), static_role), "sd3_joint_attention_static")
    elif mx is not None:
        check(load().univst_sd3_joint_attention_mx(*args, C.byref(mx)), "sd3_joint_attention_mx")
    else:
        check(load().univst_sd3_joint_attention(*args), "sd3_joint_attention")
    return (out_i, out_t) if enc is not None else out_i


def _qkv_ld(qkv, F, N):
    """row stride of a fused [3*F*N, >= 3C] q | k | v buffer: a column-sliced view of a wider buffer is fine, a column stride is not."""
    if not (qkv.is_cuda and qkv.dtype == torch.float16):
        raise ValueError(f"adain shift: expected an fp16 CUDA/HIP tensor, got {qkv.dtype} {qkv.device}")
    if qkv.dim() != 2 or qkv.shape[0] != 3 * F * N or qkv.stride(1) != 1:
        raise ValueError(f"adain shift: expected a [3*F*N = {3 * F * N}, >= 3C] buffer with unit column stride, got {tuple(qkv.shape)} "
                         f"strides {tuple(qkv.stride())}")
    return qkv.stride(0)


def sd3_adain_shift_(qkv, F, N, C_, heads, alpha, beta, gamma):
    """in place on the fused [3*F*N, 3C] buffer (SD3 plugin's AdaIN shift); qkv may be a column-sliced view (row stride >= 3C)."""
    ld = _qkv_ld(qkv, F, N)
    ws = torch.empty(4 * F * 2 * C_ + 2 * F * 2 * heads, device=qkv.device, dtype=torch.float32)
    check(load().univst_sd3_adain_shift(ptr(qkv), ld, F, N, C_, heads, alpha, beta, gamma, ptr(ws), stream_ptr()), "sd3_adain_shift")
    return qkv


def sd3_adain_shift_static_(qkv2, style_kv, F, N, C_, heads, alpha, beta, gamma):
    """in place on the stylised rows of the fused TWO-branch [2*F*N, 3C] buffer (content, stylised) against one style frame's K | V rows
    style_kv [N, 2C]; both may be column-sliced views (row strides >= 3C / 2C, unit column stride)."""
    for what, t, rows in (("qkv2", qkv2, 2 * F * N), ("style_kv", style_kv, N)):
        if not (t.is_cuda and t.dtype == torch.float16):
            raise ValueError(f"sd3 static shift: {what}: expected an fp16 CUDA/HIP tensor, got {t.dtype} {t.device}")
        if t.dim() != 2 or t.shape[0] != rows or t.stride(1) != 1:
            raise ValueError(f"sd3 static shift: {what}: expected {rows} rows with unit column stride, got {tuple(t.shape)} strides {tuple(t.stride())}")
    ws = torch.empty((2 + 2 * F) * 2 * C_ + 2 * F * 2 * heads, device=qkv2.device, dtype=torch.float32)
    check(load().univst_sd3_adain_shift_static(ptr(qkv2), qkv2.stride(0), ptr(style_kv), style_kv.stride(0), F, N, C_, heads, alpha, beta, gamma,
                                               ptr(ws), stream_ptr()), "sd3_adain_shift_static")
    return qkv2


def rmsnorm_heads_(x, heads, weight, eps=1e-6):
    """in place on [rows, heads*d] fp16."""
    _f16(x)
    rows, Cc = x.shape
    check(load().univst_rmsnorm_heads(ptr(x), x.stride(0), rows, heads, Cc // heads, ptr(weight), eps, stream_ptr()), "rmsnorm_heads")
    return x


def rmsnorm_heads_pair_(x, heads, head_dim, c0, w0, c1, w1, eps=1e-6, scale0=1.0):
    """in place on the column blocks [c0, c0 + heads*d) (weight w0, times scale0) and [c1, c1 + heads*d) (weight w1) of x [rows, ld] fp16:
    the q | k normalisation of a fused q | k | v buffer."""
    if not (x.is_cuda and x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1):
        raise ValueError("rmsnorm_heads_pair_: x must be an fp16 CUDA/HIP [rows, ld] tensor or row view with a unit column stride")
    check(load().univst_rmsnorm_heads_pair(ptr(x), x.stride(0), x.shape[0], heads, head_dim, c0, ptr(w0), c1, ptr(w1), eps, scale0, stream_ptr()),
          "rmsnorm_heads_pair")
    return x


def _mod_ld(*ts):
    """scale / shift / gate operands are [B, C] views into one [B, k*C] adaLN output: same row stride, unit column stride."""
    ld = ts[0].stride(0)
    for t in ts:
        if not (t.is_cuda and t.dtype == torch.float16):
            raise ValueError(f"modulation operand: expected an fp16 CUDA/HIP tensor, got {t.dtype} {t.device}")
        if t.dim() != 2 or t.stride(1) != 1 or t.stride(0) != ld:
            raise ValueError("modulation operands must be [B, C] row views with a common row stride")
    return ld


def adaln_modulate(x, scale, shift, eps=1e-6, scale2=None, shift2=None):
    """x [B, N, C], scale / shift [B, C] (row views allowed) -> LayerNorm(x) * (1 + scale) + shift; with scale2 / shift2 also the
    second modulation of the same normalised rows (AdaLayerNormZeroX) -> (y, y2)."""
    _f16(x)
    B, N, Cc = x.shape
    if not x.is_contiguous():
        raise ValueError("adaln_modulate: x must be contiguous")
    two = scale2 is not None
    ld = _mod_ld(scale, shift, *([scale2, shift2] if two else []))
    out = torch.empty_like(x)
    out2 = torch.empty_like(x) if two else None
    check(load().univst_adaln_modulate(ptr(x), ptr(out), ptr(scale), ptr(shift), ld, B * N, N, Cc, eps, ptr(out2), ptr(scale2), ptr(shift2),
                                       stream_ptr()), "adaln_modulate")
    return (out, out2) if two else out


def gate_residual(x, gate, y, out=None):
    """x + gate[:, None] * y for x, y [B, N, C], gate [B, C] (row view allowed)."""
    _f16(x), _f16(y)
    B, N, Cc = x.shape
    if not (x.is_contiguous() and y.is_contiguous()):
        raise ValueError("gate_residual: x and y must be contiguous")
    out = torch.empty_like(x) if out is None else out
    check(load().univst_gate_residual(ptr(x), ptr(gate), _mod_ld(gate), ptr(y), ptr(out), B * N, N, Cc, stream_ptr()), "gate_residual")
    return out


ACT_SILU, ACT_GELU_TANH = 0, 1


def activation(x, act, out=None):
    _f16(x)
    if not x.is_contiguous():
        raise ValueError("activation: x must be contiguous")
    out = torch.empty_like(x) if out is None else out
    check(load().univst_activation(ptr(x), ptr(out), x.numel(), act, stream_ptr()), "activation")
    return out


def timestep_embedding(t, dim, flip_sin_to_cos=True, downscale_freq_shift=0.0, max_period=10000.0):
    """t [B] (any float dtype, device) -> [B, dim] fp16 sinusoidal embedding (diffusers Timesteps)."""
    t = t.to(torch.float32).contiguous()
    out = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float16)
    check(load().univst_timestep_embedding(ptr(t), ptr(out), t.shape[0], dim, int(flip_sin_to_cos), downscale_freq_shift, max_period, stream_ptr()),
          "timestep_embedding")
    return out


def sd3_patchify(latents, patch):
    """[B, C, H, W] -> [B*(H/p)*(W/p), C*p*p] (k order of the flattened PatchEmbed conv weight)."""
    _f16(latents)
    B, Cc, H, W = latents.shape
    rows = torch.empty(B * (H // patch) * (W // patch), Cc * patch * patch, device=latents.device, dtype=torch.float16)
    check(load().univst_sd3_patchify(ptr(latents.contiguous()), ptr(rows), B, Cc, H, W, patch, stream_ptr()), "sd3_patchify")
    return rows


def sd3_unpatchify(rows, B, Cc, H, W, patch):
    """[B*(H/p)*(W/p), p*p*C] -> [B, C, H, W]."""
    _f16(rows)
    lat = torch.empty(B, Cc, H, W, device=rows.device, dtype=torch.float16)
    check(load().univst_sd3_unpatchify(ptr(rows.contiguous()), ptr(lat), B, Cc, H, W, patch, stream_ptr()), "sd3_unpatchify")
    return lat


def axpbypcz(x, y, z, a, b, c, out=None):
    _f16(x), _f16(y), _f16(z)
    out = torch.empty_like(x) if out is None else out
    check(load().univst_axpbypcz(ptr(x), ptr(y), ptr(z), ptr(out), a, b, c, x.numel(), stream_ptr()), "axpbypcz")
    return out


def attention_adain_shift_(qkv, F, N, C_, alpha, beta, gamma, return_stats=False):
    """in place on the fused [3*F*N, 3C] buffer; qkv may be a column-sliced view (row stride >= 3C).  return_stats: also the style
    branch's per-(frame, channel) statistics the kernel used, (mean, unbiased std) each [F, 2C] (K columns then V columns)."""
    ld = _qkv_ld(qkv, F, N)
    ws = torch.empty(4 * F * 2 * C_, device=qkv.device, dtype=torch.float32)
    check(load().univst_attention_adain_shift(ptr(qkv), ld, F, N, C_, alpha, beta, gamma, ptr(ws), stream_ptr()),
          "attention_adain_shift")
    if return_stats:
        return qkv, ws[:F * 2 * C_].view(F, 2 * C_), ws[F * 2 * C_:2 * F * 2 * C_].view(F, 2 * C_)
    return qkv


def attention_adain_shift_static_(qkv, style_kv, F, N, C_, alpha, beta, gamma):
    """in place on the fused TWO-branch buffer [2*F*N, >= 3C] (content rows, then stylised rows) against ONE frame of style K | V rows
    [N, >= 2C] that serves every frame; both may be column-sliced views of wider buffers (unit column stride)."""
    for t, rows, what in ((qkv, 2 * F * N, "qkv"), (style_kv, N, "style_kv")):
        if not (t.is_cuda and t.dtype == torch.float16):
            raise ValueError(f"adain shift: {what}: expected an fp16 CUDA/HIP tensor, got {t.dtype} {t.device}")
        if t.dim() != 2 or t.shape[0] != rows or t.stride(1) != 1:
            raise ValueError(f"adain shift: {what}: expected {rows} rows with unit column stride, got {tuple(t.shape)} strides {tuple(t.stride())}")
    ws = torch.empty(4 * C_, device=qkv.device, dtype=torch.float32)
    check(load().univst_attention_adain_shift_static(ptr(qkv), qkv.stride(0), ptr(style_kv), style_kv.stride(0), F, N, C_, alpha, beta, gamma,
                                                     ptr(ws), stream_ptr()), "attention_adain_shift_static")
    return qkv


def latent_adain(cnt, sty, out=None):
    _f16(cnt), _f16(sty)
    _, Cl, F, H, W = cnt.shape
    out = torch.empty_like(cnt) if out is None else out
    check(load().univst_latent_adain(ptr(cnt), ptr(sty), ptr(out), Cl, F, H * W, stream_ptr()), "latent_adain")
    return out


def latent_adain_stats(cnt):
    """frame-shard half 1 of latent_adain: per-channel (sum, sum of squares) of the local content frames [1, C, Fl, h, w] -> [C, 2] fp32,
    to be summed over the ranks."""
    _f16(cnt)
    _, Cl, Fl, H, W = cnt.shape
    st = torch.empty(Cl, 2, device=cnt.device, dtype=torch.float32)
    check(load().univst_latent_adain_stats(ptr(cnt), ptr(st), Cl, Fl, H * W, stream_ptr()), "latent_adain_stats")
    return st


def latent_adain_apply(cnt, sty, stats, n_total, out=None):
    """frame-shard half 2: latent_adain of the local frames with the content statistics of the whole clip (stats [C, 2] fp32 summed
    over the ranks, n_total = F * h * w of the clip)."""
    _f16(cnt), _f16(sty)
    if sty.shape != cnt.shape:
        raise ValueError(f"latent_adain_apply: cnt {tuple(cnt.shape)} and sty {tuple(sty.shape)} differ in shape")
    _, Cl, Fl, H, W = cnt.shape
    if not (stats.is_cuda and stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() == 2 * Cl):
        raise ValueError(f"latent_adain_apply: stats must be {Cl} x 2 contiguous fp32 on the GPU")
    out = torch.empty_like(cnt) if out is None else out
    check(load().univst_latent_adain_apply(ptr(cnt), ptr(sty), ptr(stats), int(n_total), ptr(out), Cl, Fl, H * W, stream_ptr()), "latent_adain_apply")
    return out


def axpby(x, e, cx, ce, out=None):
    _f16(x), _f16(e)
    out = torch.empty_like(x) if out is None else out
    check(load().univst_axpby(ptr(x), ptr(e), ptr(out), cx, ce, x.numel(), stream_ptr()), "axpby")
    return out


def mask_blend(a, b, m, out=None):
    """(1-m)*a + m*b with a,b [1,C,F,h,w], m [F,h,w] fp16 or None."""
    _f16(a), _f16(b)
    out = torch.empty_like(a) if out is None else out
    Cl = a.shape[1]
    check(load().univst_mask_blend(ptr(a), ptr(b), ptr(m), ptr(out), Cl, a.numel() // Cl, stream_ptr()), "mask_blend")
    return out


def mask_resize(mask_u8, h, w):
    """uint8 {0,1} [F,H,W] -> fp16 [F,h,w] (torch bilinear, align_corners=False)."""
    F, H, W = mask_u8.shape
    out = torch.empty(F, h, w, device=mask_u8.device, dtype=torch.float16)
    check(load().univst_mask_resize(ptr(mask_u8), ptr(out), F, H, W, h, w, stream_ptr()), "mask_resize")
    return out


def debug_tr16():
    out = torch.empty(256, device="cuda", dtype=torch.float32)
    check(load().univst_debug_tr16(ptr(out), stream_ptr()), "debug_tr16")
    return out


def unet_query(handle, name: str) -> float:
    """read-out of a UNet handle (include/univst.h ``univst_unet_query``): "emu_wire_us", "arena_high_water"."""
    out = C.c_double(0.0)
    check(load().univst_unet_query(handle, name.encode(), C.byref(out)), f"unet_query({name})")
    return out.value


def delay_us(us: float):
    check(load().univst_debug_delay_us(float(us), stream_ptr()), "debug_delay_us")


PROFILE_CLASSES = ("gemm_big_kernel<0>", "gemm_big_kernel<1>", "gemm_kernel<*,0>", "gemm_kernel<*,1>", "attn_pp40_kernel<true>",
                   "attn_kernel_occ3<96,5,2>", "attn_kernel<other>", "groupnorm", "layernorm", "adain_shift", "attn_kernel<text>",
                   "conv_patch_kernel", "attn2_fused_kernel", "linear_mxfp8_kernel")


def profile_enable(on: bool):
    check(load().univst_profile_enable(int(on)), "profile_enable")


def profile_symbols():
    """-> {class: [kernel symbols launched since profile_enable(True)]}"""
    out = {}
    for i, name in enumerate(PROFILE_CLASSES):
        buf = C.create_string_buffer(2048)
        check(load().univst_profile_symbols(i, buf, 2048), "profile_symbols")
        out[name] = [s for s in buf.value.decode().split(";") if s]
    return out


def profile_collect():
    """-> {class: dict(ms=, launches=, flops=, bytes=, expanded_bytes=)} for everything launched since profile_enable(True)."""
    n = len(PROFILE_CLASSES)
    ms, cnt, fl, by = (C.c_double * n)(), (C.c_int64 * n)(), (C.c_double * n)(), (C.c_double * n)()
    check(load().univst_profile_collect(ms, cnt, fl, by, n), "profile_collect")
    aux = (C.c_double * n)()
    check(load().univst_profile_collect_aux(aux, n), "profile_collect_aux")
    return {PROFILE_CLASSES[i]: dict(ms=ms[i], launches=cnt[i], flops=fl[i], bytes=by[i], expanded_bytes=aux[i]) for i in range(n)}
