"""The AnimateDiff-v2 motion module on the native library.

``NativeMotionModule`` stands where the reference's AnimateDiff UNet keeps a ``VanillaTemporalModule`` (backbones/animatediff/models/motion_module.py,
called as ``motion_module(hidden_states, temb, encoder_hidden_states=...)`` at unet_blocks.py:275): per-frame GroupNorm, proj_in, one or more
transformer blocks of ``Temporal_Self`` attentions along the frame axis and a GEGLU feed-forward, proj_out, plus the input.  It takes that module's
state dict unchanged and runs one C-ABI call per forward (univst_motion_*, csrc/motion.hip).  The Attention / FeedForward layers inside are diffusers'
(third-party): restated from their published definition; tests/motion_ref.py is the yardstick, held to the reference by tests/test_motion_ref.py."""
import ctypes as C
import re
import types

import torch

from . import _native

DEFAULT_CONFIG = dict(channels=None, num_attention_heads=8, num_transformer_block=1, attention_block_types=("Temporal_Self", "Temporal_Self"),
                      norm_num_groups=32, temporal_position_encoding=True, temporal_position_encoding_max_len=24, temporal_attention_dim_div=1,
                      norm_eps=1e-6, layer_norm_eps=1e-5)
MAX_FRAMES = 32
_PE_KEY = re.compile(r"^temporal_transformer\.transformer_blocks\.\d+\.attention_blocks\.\d+\.pos_encoder\.pe$")


def check_supported(cfg):
    """the configurations the native module has: self-attention along the frame axis at the full width"""
    for t in cfg["attention_block_types"]:
        if t != "Temporal_Self":
            raise NotImplementedError(f"NativeMotionModule: attention block type {t!r} is unsupported (the native module has Temporal_Self only; "
                                      "AnimateDiff-v2 uses no _Cross block)")
    if cfg["temporal_attention_dim_div"] != 1:
        raise NotImplementedError(f"NativeMotionModule: temporal_attention_dim_div = {cfg['temporal_attention_dim_div']} is unsupported "
                                  "(the native module attends at the full width: 1)")


class NativeMotionModule(_native.NativeModuleFacade):
    _kind, _noun = "motion", "motion module"

    def __init__(self, state_dict, config=None, prefix="", device="cuda"):
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix) and torch.is_tensor(v) and v.is_floating_point()}
        cfg = self.merge_config(DEFAULT_CONFIG, config)
        if "temporal_transformer.norm.weight" not in sd:
            raise KeyError(f"NativeMotionModule: {prefix}temporal_transformer.norm.weight is not in the state dict (is the prefix right?)")
        cfg["channels"] = int(sd["temporal_transformer.norm.weight"].shape[0])
        pes = [v for k, v in sd.items() if _PE_KEY.match(k)]
        if pes:                                 # a published checkpoint carries its table [1, max_len, C]: it says max_len and replaces the formula
            cfg["temporal_position_encoding"], cfg["temporal_position_encoding_max_len"] = True, int(pes[0].shape[1])
        cfg["attention_block_types"] = tuple(cfg["attention_block_types"])
        check_supported(cfg)
        self.config = types.SimpleNamespace(**cfg)
        self.device = torch.device(device)
        # without position encoding there is no table: the length only has to be one the handle accepts
        max_len = cfg["temporal_position_encoding_max_len"] if cfg["temporal_position_encoding"] else min(cfg["temporal_position_encoding_max_len"], MAX_FRAMES)
        c = _native.MotionCfg(cfg["channels"], cfg["num_attention_heads"], cfg["num_transformer_block"], len(cfg["attention_block_types"]),
                              cfg["norm_num_groups"], max_len, int(bool(cfg["temporal_position_encoding"])),
                              cfg["norm_eps"], cfg["layer_norm_eps"])
        self._h = _native.load_handle("motion", (C.byref(c),), sd.items(), other_dtype=torch.float16, device=device)

    @classmethod
    def from_module(cls, m, device="cuda"):
        """a loaded VanillaTemporalModule (the reference's, or the mirror of univst_amd/backbones/animatediff).  The non-persistent ``pe`` buffers are
        not in its state dict: only their LENGTH is read off the module, their contents are not — the handle computes the sinusoid itself (in
        double, rounded to fp16 once).  A module whose ``pe`` buffer was overwritten with another table must pass that table under the
        ``...pos_encoder.pe`` key of a state dict instead.  Without position encoding the module takes up to 32 frames."""
        blocks = m.temporal_transformer.transformer_blocks
        attn = blocks[0].attention_blocks[0]
        pos = getattr(attn, "pos_encoder", None)
        cfg = dict(num_attention_heads=attn.heads, num_transformer_block=len(blocks),
                   attention_block_types=tuple("Temporal_Cross" if getattr(a, "is_cross_attention", False) else "Temporal_Self" for a in blocks[0].attention_blocks),
                   norm_num_groups=m.temporal_transformer.norm.num_groups, temporal_position_encoding=pos is not None,
                   temporal_position_encoding_max_len=int(pos.pe.shape[1]) if pos is not None else 24,
                   temporal_attention_dim_div=m.temporal_transformer.norm.num_channels // attn.to_q.weight.shape[0])
        return cls(m.state_dict(), config=cfg, device=device)

    def _check(self, t, what):
        if self._gpu_only(t, what).dtype != torch.float16:
            raise TypeError(f"NativeMotionModule.{what}: fp16 activations only, got {t.dtype}")
        return t

    @torch.no_grad()
    def forward_rows(self, x_rows, B, F, N):
        """the native layout: x_rows fp16 [B * F * N, C] (or [B * F, N, C]), row (b * F + f) * N + n -> a new tensor of the same shape"""
        x = self._check(x_rows, "forward_rows")
        Cw = self.config.channels
        if x.numel() != B * F * N * Cw or x.shape[-1] != Cw:
            raise ValueError(f"NativeMotionModule.forward_rows: expected B*F*N = {B * F * N} rows of {Cw} channels, got {tuple(x.shape)}")
        if self.config.temporal_position_encoding and F > self.config.temporal_position_encoding_max_len:
            raise ValueError(f"NativeMotionModule: {F} frames exceed temporal_position_encoding_max_len {self.config.temporal_position_encoding_max_len}")
        if F > MAX_FRAMES:
            raise ValueError(f"NativeMotionModule: {F} frames (the frame-axis attention kernel holds at most {MAX_FRAMES})")
        x = x.contiguous()
        y = torch.empty_like(x)
        _native.check(_native.load().univst_motion_forward(self._h, _native.ptr(x), _native.ptr(y), B, F, N, _native.stream_ptr()), "motion_forward")
        return y

    @torch.no_grad()
    def __call__(self, input_tensor, temb=None, encoder_hidden_states=None, attention_mask=None, **_):
        """the reference's call: input_tensor fp16 [B, C, F, H, W] -> the same shape; temb and the text are unused by Temporal_Self blocks.  One permute
        into the native row order and one back."""
        x = self._check(input_tensor, "__call__")
        if x.dim() != 5 or x.shape[1] != self.config.channels:
            raise ValueError(f"NativeMotionModule: expected [B, {self.config.channels}, F, H, W], got {tuple(x.shape)}")
        if attention_mask is not None:
            raise NotImplementedError("NativeMotionModule: an attention_mask is not implemented (the AnimateDiff UNet passes none)")
        B, Cw, F, H, W = x.shape
        rows = x.permute(0, 2, 3, 4, 1).reshape(B * F * H * W, Cw)
        y = self.forward_rows(rows, B, F, H * W)
        return y.view(B, F, H, W, Cw).permute(0, 4, 1, 2, 3).contiguous()

    forward = __call__
