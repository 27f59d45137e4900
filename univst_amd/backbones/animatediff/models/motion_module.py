"""AnimateDiff's motion module (backbones/animatediff/models/motion_module.py of the reference) on the native library.

``VanillaTemporalModule`` keeps the reference's constructor signature, call signature and parameter names — a motion-module checkpoint slice loads with
``load_state_dict(strict=True)`` — and its forward is one call of the native handle (univst_amd/motion.py -> univst_motion_*, csrc/motion.hip): there
is no eager path.  The modules below exist to hold the parameters under the reference's names; the handle copies them and is rebuilt when they change.
Supported: ``Temporal_Self`` attention blocks at the full width (``temporal_attention_dim_div = 1``), which is what animatediff-v2.yaml configures."""
import torch
from torch import nn

from ....motion import NativeMotionModule, check_supported


def zero_module(module):
    """all parameters of ``module`` set to zero in place; returns the module"""
    with torch.no_grad():
        for param in module.parameters():
            nn.init.zeros_(param)
    return module


def get_motion_module(in_channels, motion_module_type: str, motion_module_kwargs: dict):
    if motion_module_type == "Vanilla":
        return VanillaTemporalModule(in_channels=in_channels, **motion_module_kwargs)
    raise ValueError(f"motion_module_type {motion_module_type!r}: the reference has \"Vanilla\" only")


def sinusoid_table(max_len, d_model):
    """[1, max_len, d_model] fp32: column pair i of row f holds (sin, cos) of the angle f * 10000^(-2i / d_model)"""
    rate = torch.pow(torch.tensor(10000.0), -torch.arange(0, d_model, 2, dtype=torch.float32) / d_model)       # [d_model / 2]
    angle = torch.arange(max_len, dtype=torch.float32)[:, None] * rate[None, :]                                 # [max_len, d_model / 2]
    return torch.stack((angle.sin(), angle.cos()), dim=-1).flatten(-2).unsqueeze(0)


class PositionalEncoding(nn.Module):
    """holder of the table as a NON-persistent buffer ``pe`` (absent from the state dict, as in the reference).  The native handle reads its LENGTH
    only: it computes the same sinusoid itself (csrc/motion.hip finalize), unless a state dict carries a table under ``pos_encoder.pe``."""

    def __init__(self, d_model, dropout=0.0, max_len=24):
        super().__init__()
        self.register_buffer("pe", sinusoid_table(max_len, d_model), persistent=False)


class VersatileAttention(nn.Module):
    """parameter holder of one Temporal_Self attention: to_q / to_k / to_v without bias, to_out = [Linear, Dropout]"""

    def __init__(self, query_dim, heads, dim_head, temporal_position_encoding=False, temporal_position_encoding_max_len=24):
        super().__init__()
        inner = heads * dim_head
        self.heads = heads
        self.scale = dim_head ** -0.5
        self.attention_mode = "Temporal"
        self.is_cross_attention = False
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(query_dim, inner, bias=False)
        self.to_v = nn.Linear(query_dim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, query_dim), nn.Dropout(0.0)])
        self.pos_encoder = PositionalEncoding(query_dim, max_len=temporal_position_encoding_max_len) if temporal_position_encoding else None


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):
    """parameter holder of diffusers' FeedForward(geglu): net = [GEGLU, Dropout, Linear]"""

    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.ModuleList([GEGLU(dim, dim * mult), nn.Dropout(0.0), nn.Linear(dim * mult, dim)])


class TemporalTransformerBlock(nn.Module):
    def __init__(self, dim, num_attention_heads, attention_head_dim, attention_block_types, temporal_position_encoding, temporal_position_encoding_max_len):
        super().__init__()
        self.attention_blocks = nn.ModuleList([VersatileAttention(dim, num_attention_heads, attention_head_dim, temporal_position_encoding,
                                                                  temporal_position_encoding_max_len) for _ in attention_block_types])
        self.norms = nn.ModuleList([nn.LayerNorm(dim) for _ in attention_block_types])
        self.ff = FeedForward(dim)
        self.ff_norm = nn.LayerNorm(dim)


class TemporalTransformer3DModel(nn.Module):
    def __init__(self, in_channels, num_attention_heads, attention_head_dim, num_layers, attention_block_types, temporal_position_encoding,
                 temporal_position_encoding_max_len, norm_num_groups=32):
        super().__init__()
        inner_dim = num_attention_heads * attention_head_dim
        self.norm = nn.GroupNorm(num_groups=norm_num_groups, num_channels=in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Linear(in_channels, inner_dim)
        self.transformer_blocks = nn.ModuleList([TemporalTransformerBlock(inner_dim, num_attention_heads, attention_head_dim, attention_block_types,
                                                                          temporal_position_encoding, temporal_position_encoding_max_len)
                                                 for _ in range(num_layers)])
        self.proj_out = nn.Linear(inner_dim, in_channels)


class VanillaTemporalModule(nn.Module):
    def __init__(self, in_channels, num_attention_heads=8, num_transformer_block=2, attention_block_types=("Temporal_Self", "Temporal_Self"),
                 cross_frame_attention_mode=None, temporal_position_encoding=False, temporal_position_encoding_max_len=24,
                 temporal_attention_dim_div=1, zero_initialize=True):
        super().__init__()
        check_supported(dict(attention_block_types=tuple(attention_block_types), temporal_attention_dim_div=temporal_attention_dim_div))
        if cross_frame_attention_mode is not None:
            raise NotImplementedError(f"VanillaTemporalModule: cross_frame_attention_mode = {cross_frame_attention_mode!r} is unsupported "
                                      "(the reference's attention ignores it; AnimateDiff-v2 leaves it None)")
        head_dim = in_channels // (num_attention_heads * temporal_attention_dim_div)
        self.temporal_transformer = TemporalTransformer3DModel(in_channels, num_attention_heads, head_dim, num_transformer_block, tuple(attention_block_types),
                                                               temporal_position_encoding, temporal_position_encoding_max_len)
        if zero_initialize:         # the module starts as the identity: proj_out(h) + x = x
            zero_module(self.temporal_transformer.proj_out)
        self._native = None
        self._native_fp = None

    def _fingerprint(self):
        """(storage address, version counter) of every parameter: an edit through the tensor itself or a re-allocation (``.half()``, ``.cuda()``,
        ``load_state_dict``) changes it; edits through ``p.data`` do not — call ``invalidate_native()`` after those"""
        acc = 0
        for t in self.state_dict(keep_vars=True).values():
            acc = (acc * 1000003 + t.data_ptr() + 7919 * t._version) & 0xFFFFFFFFFFFFFFFF
        return acc

    def __getstate__(self):
        """copies and pickles carry the parameters, not the handle (a pointer into the library): the copy builds its own at its first forward"""
        state = dict(self.__dict__)
        state["_native"], state["_native_fp"] = None, None
        return state

    def invalidate_native(self):
        """force a rebuild of the native weight copy at the next forward"""
        self._native_fp = None

    def _sync_native(self):
        fp = self._fingerprint()
        if self._native is None or fp != self._native_fp:
            self._native = NativeMotionModule.from_module(self)
            self._native_fp = fp
        return self._native

    def forward(self, input_tensor, temb=None, encoder_hidden_states=None, attention_mask=None, anchor_frame_idx=None):
        if not torch.is_tensor(input_tensor) or not input_tensor.is_cuda:
            raise RuntimeError("VanillaTemporalModule.forward runs only on an AMD GPU: move the module and its input there with .cuda() "
                               "(univst_amd has no CPU path)")
        return self._sync_native()(input_tensor, temb, encoder_hidden_states, attention_mask=attention_mask)
