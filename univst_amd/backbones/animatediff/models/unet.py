"""Host-side mirror of AnimateDiff's ``UNet3DConditionModel`` (backbones/animatediff/models/unet.py of the reference, as animatediff-v2.yaml
configures it) on the native library.

Kept, so that the class drops into the reference's scripts: the module tree and therefore every ``state_dict()`` key in the reference's order
(``down_blocks.i.resnets.j.*``, ``...attentions.j.transformer_blocks.0.*``, ``down_blocks.i.motion_modules.j.temporal_transformer.*``,
``mid_block.motion_modules.0.*``, ``conv_norm_out``), the config keys, ``from_pretrained_2d(path, subfolder, unet_additional_kwargs)`` over a local
``config.json`` plus weights, ``load_state_dict(strict=False)`` for a motion checkpoint (``utils/util.py load_weights``) and
``forward(sample, timestep, encoder_hidden_states).sample``.

Different: the modules carry parameters only.  The forward is ONE call of the native graph (csrc/unet.hip behind ``univst_unet_create_animatediff``:
the SD-v1.5 2-D UNet per frame, a motion module behind every resnet / transformer pair); there is no PyTorch fallback and no CPU path.  Not built:
``unet_use_cross_frame_attention`` / ``unet_use_temporal_attention`` (animatediff-v2.yaml leaves both off), ``motion_module_decoder_only``,
SparseControlNet inputs.  The feature dump (``ft_indices`` / ``ft_timesteps`` / ``ft_path``, unet.py:453-459) is one ``univst_unet_forward_tap`` call and
writes the reference's file, as the SD mirror does: one block per call, ``last_feature_map`` keeps the tensor."""
import ctypes as C
import json
import os
from typing import Optional, Tuple, Union

import torch
import torch.nn as nn

from .... import _native
from ...video_diffusion_sd.models.unet_3d_condition import (Attention, FeedForward, TimestepEmbedding, UNetPseudo3DConditionOutput, _Config, _ParamOnly,
                                                            _REGISTRATION_EPOCH)
from .motion_module import get_motion_module

UNet3DConditionOutput = UNetPseudo3DConditionOutput
_DOWN = ("CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "CrossAttnDownBlock3D", "DownBlock3D")
_UP = ("UpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D", "CrossAttnUpBlock3D")
WEIGHTS_NAME = "diffusion_pytorch_model.bin"          # diffusers.utils.WEIGHTS_NAME


class InflatedConv3d(nn.Conv2d):
    """resnet.py:10-18 (parameters of a Conv2d, applied per frame by the native graph)"""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("InflatedConv3d runs as part of the native UNet graph")


class InflatedGroupNorm(nn.GroupNorm):
    """resnet.py:21-29 (statistics per frame)"""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("InflatedGroupNorm runs as part of the native UNet graph")


def _norm(inflated, groups, channels, eps):
    return (InflatedGroupNorm if inflated else nn.GroupNorm)(num_groups=groups, num_channels=channels, eps=eps, affine=True)


class ResnetBlock3D(_ParamOnly):
    """resnet.py:109-180 (ctor)"""

    def __init__(self, in_channels, out_channels, temb_channels, groups, eps, inflated):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1 = _norm(inflated, groups, in_channels, eps)
        self.conv1 = InflatedConv3d(in_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.time_emb_proj = nn.Linear(temb_channels, out_channels)
        self.norm2 = _norm(inflated, groups, out_channels, eps)
        self.dropout = nn.Dropout(0.0)
        self.conv2 = InflatedConv3d(out_channels, out_channels, kernel_size=3, stride=1, padding=1)
        self.conv_shortcut = None
        if in_channels != out_channels:
            self.conv_shortcut = InflatedConv3d(in_channels, out_channels, kernel_size=1, stride=1, padding=0)


class BasicTransformerBlock(_ParamOnly):
    """attention.py:215-283 (ctor; no cross-frame attn1, no attn_temp)"""

    def __init__(self, dim, heads, dim_head, cross_attention_dim):
        super().__init__()
        self.attn1 = Attention(query_dim=dim, heads=heads, dim_head=dim_head)
        self.norm1 = nn.LayerNorm(dim)
        self.attn2 = Attention(query_dim=dim, cross_attention_dim=cross_attention_dim, heads=heads, dim_head=dim_head)
        self.norm2 = nn.LayerNorm(dim)
        self.ff = FeedForward(dim)
        self.norm3 = nn.LayerNorm(dim)


class Transformer3DModel(_ParamOnly):
    """attention.py:101-163 (ctor; 1x1-conv projections)"""

    def __init__(self, heads, dim_head, in_channels, cross_attention_dim, groups):
        super().__init__()
        inner = heads * dim_head
        self.norm = nn.GroupNorm(num_groups=groups, num_channels=in_channels, eps=1e-6, affine=True)
        self.proj_in = nn.Conv2d(in_channels, inner, kernel_size=1, stride=1, padding=0)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, heads, dim_head, cross_attention_dim)])
        self.proj_out = nn.Conv2d(inner, in_channels, kernel_size=1, stride=1, padding=0)


class Downsample3D(_ParamOnly):
    def __init__(self, channels):
        super().__init__()
        self.conv = InflatedConv3d(channels, channels, 3, stride=2, padding=1)


class Upsample3D(_ParamOnly):
    def __init__(self, channels):
        super().__init__()
        self.conv = InflatedConv3d(channels, channels, 3, padding=1)


def _motion(channels, on, mtype, kwargs):
    return get_motion_module(in_channels=channels, motion_module_type=mtype, motion_module_kwargs=kwargs) if on else None


class _Block(_ParamOnly):
    has_cross_attention = False


class CrossAttnDownBlock3D(_Block):
    has_cross_attention = True

    def __init__(self, in_c, out_c, temb, layers, groups, eps, heads, xdim, add_downsample, inflated, motion):
        super().__init__()
        resnets, attns, mms = [], [], []
        for i in range(layers):
            resnets.append(ResnetBlock3D(in_c if i == 0 else out_c, out_c, temb, groups, eps, inflated))
            attns.append(Transformer3DModel(heads, out_c // heads, out_c, xdim, groups))
            mms.append(_motion(out_c, *motion))
        self.attentions = nn.ModuleList(attns)
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList(mms)
        self.downsamplers = nn.ModuleList([Downsample3D(out_c)]) if add_downsample else None


class DownBlock3D(_Block):
    def __init__(self, in_c, out_c, temb, layers, groups, eps, add_downsample, inflated, motion):
        super().__init__()
        self.resnets = nn.ModuleList([ResnetBlock3D(in_c if i == 0 else out_c, out_c, temb, groups, eps, inflated) for i in range(layers)])
        self.motion_modules = nn.ModuleList([_motion(out_c, *motion) for _ in range(layers)])
        self.downsamplers = nn.ModuleList([Downsample3D(out_c)]) if add_downsample else None


class UNetMidBlock3DCrossAttn(_Block):
    has_cross_attention = True

    def __init__(self, c, temb, groups, eps, heads, xdim, inflated, motion):
        super().__init__()
        resnets = [ResnetBlock3D(c, c, temb, groups, eps, inflated)]
        attns = [Transformer3DModel(heads, c // heads, c, xdim, groups)]
        mms = [_motion(c, *motion)]
        resnets.append(ResnetBlock3D(c, c, temb, groups, eps, inflated))
        self.attentions = nn.ModuleList(attns)
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList(mms)


class CrossAttnUpBlock3D(_Block):
    has_cross_attention = True

    def __init__(self, in_c, out_c, prev_c, temb, layers, groups, eps, heads, xdim, add_upsample, inflated, motion):
        super().__init__()
        resnets, attns, mms = [], [], []
        for i in range(layers):
            skip = in_c if i == layers - 1 else out_c
            rin = prev_c if i == 0 else out_c
            resnets.append(ResnetBlock3D(rin + skip, out_c, temb, groups, eps, inflated))
            attns.append(Transformer3DModel(heads, out_c // heads, out_c, xdim, groups))
            mms.append(_motion(out_c, *motion))
        self.attentions = nn.ModuleList(attns)
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList(mms)
        self.upsamplers = nn.ModuleList([Upsample3D(out_c)]) if add_upsample else None


class UpBlock3D(_Block):
    def __init__(self, in_c, out_c, prev_c, temb, layers, groups, eps, add_upsample, inflated, motion):
        super().__init__()
        resnets = []
        for i in range(layers):
            skip = in_c if i == layers - 1 else out_c
            rin = prev_c if i == 0 else out_c
            resnets.append(ResnetBlock3D(rin + skip, out_c, temb, groups, eps, inflated))
        self.resnets = nn.ModuleList(resnets)
        self.motion_modules = nn.ModuleList([_motion(out_c, *motion) for _ in range(layers)])
        self.upsamplers = nn.ModuleList([Upsample3D(out_c)]) if add_upsample else None


class UNet3DConditionModel(nn.Module):
    def __init__(self, sample_size: Optional[int] = None, in_channels: int = 4, out_channels: int = 4, center_input_sample: bool = False,
                 flip_sin_to_cos: bool = True, freq_shift: int = 0, down_block_types: Tuple[str] = _DOWN, mid_block_type: str = "UNetMidBlock3DCrossAttn",
                 up_block_types: Tuple[str] = _UP, only_cross_attention=False, block_out_channels: Tuple[int] = (320, 640, 1280, 1280),
                 layers_per_block: int = 2, downsample_padding: int = 1, mid_block_scale_factor: float = 1, act_fn: str = "silu",
                 norm_num_groups: int = 32, norm_eps: float = 1e-5, cross_attention_dim: int = 1280, attention_head_dim: Union[int, Tuple[int]] = 8,
                 dual_cross_attention: bool = False, use_linear_projection: bool = False, class_embed_type=None, num_class_embeds=None,
                 upcast_attention: bool = False, resnet_time_scale_shift: str = "default", use_inflated_groupnorm=False, use_motion_module=False,
                 motion_module_resolutions=(1, 2, 4, 8), motion_module_mid_block=False, motion_module_decoder_only=False, motion_module_type=None,
                 motion_module_kwargs=None, unet_use_cross_frame_attention=False, unet_use_temporal_attention=False, **kwargs):
        super().__init__()
        motion_module_kwargs = dict(motion_module_kwargs or {})
        cfg = dict(locals())
        for k in ("self", "kwargs", "__class__"):
            cfg.pop(k, None)
        cfg.update(kwargs)
        self._internal_dict = _Config(cfg)
        unsupported = []
        if tuple(down_block_types) != _DOWN or tuple(up_block_types) != _UP or mid_block_type != "UNetMidBlock3DCrossAttn":
            unsupported.append("block types other than the SD-v1.x layout")
        if class_embed_type is not None or num_class_embeds is not None:
            unsupported.append("class embeddings")
        if center_input_sample or dual_cross_attention or only_cross_attention or use_linear_projection or resnet_time_scale_shift != "default":
            unsupported.append("center_input_sample / dual_cross_attention / only_cross_attention / use_linear_projection / scale_shift")
        if act_fn not in ("silu", "swish") or len(block_out_channels) != 4 or downsample_padding != 1 or mid_block_scale_factor != 1:
            unsupported.append("act_fn / depth / padding / scale-factor variants")
        if unet_use_cross_frame_attention or unet_use_temporal_attention:
            unsupported.append("unet_use_cross_frame_attention / unet_use_temporal_attention (animatediff-v2.yaml leaves both off)")
        if use_motion_module and motion_module_decoder_only:
            unsupported.append("motion_module_decoder_only")
        if unsupported:
            raise NotImplementedError("univst_amd native AnimateDiff UNet does not implement: " + "; ".join(unsupported))
        boc, groups, eps, xdim, infl = tuple(block_out_channels), norm_num_groups, norm_eps, cross_attention_dim, bool(use_inflated_groupnorm)
        hl = (attention_head_dim,) * 4 if isinstance(attention_head_dim, int) else tuple(attention_head_dim)        # head COUNT per level
        if len(hl) != 4:
            raise NotImplementedError("attention_head_dim must be an int or a 4-tuple")
        self._heads_per_level = hl
        res_on = [bool(use_motion_module) and (2 ** i in tuple(motion_module_resolutions)) for i in range(4)]
        self._motion_mask = sum(1 << i for i in range(4) if res_on[i])
        self._motion_mid = bool(use_motion_module and motion_module_mid_block)
        mm = lambda on: (on, motion_module_type, motion_module_kwargs)      # noqa: E731
        ted = boc[0] * 4
        self.sample_size = sample_size
        self.conv_in = InflatedConv3d(in_channels, boc[0], kernel_size=3, padding=(1, 1))
        self.time_embedding = TimestepEmbedding(boc[0], ted)
        self.class_embedding = None
        self.down_blocks = nn.ModuleList([])
        self.mid_block = None
        self.up_blocks = nn.ModuleList([])
        out_c = boc[0]
        for i, bt in enumerate(down_block_types):
            in_c, out_c = out_c, boc[i]
            final = i == 3
            if bt == "DownBlock3D":
                blk = DownBlock3D(in_c, out_c, ted, layers_per_block, groups, eps, not final, infl, mm(res_on[i]))
            else:
                blk = CrossAttnDownBlock3D(in_c, out_c, ted, layers_per_block, groups, eps, hl[i], xdim, not final, infl, mm(res_on[i]))
            self.down_blocks.append(blk)
        self.mid_block = UNetMidBlock3DCrossAttn(boc[-1], ted, groups, eps, hl[-1], xdim, infl, mm(self._motion_mid))
        self.num_upsamplers = 0
        rev = list(reversed(boc))
        out_c = rev[0]
        for i, bt in enumerate(up_block_types):
            final = i == 3
            prev_c, out_c = out_c, rev[i]
            in_c = rev[min(i + 1, 3)]
            if not final:
                self.num_upsamplers += 1
            if bt == "UpBlock3D":
                blk = UpBlock3D(in_c, out_c, prev_c, ted, layers_per_block + 1, groups, eps, not final, infl, mm(res_on[3 - i]))
            else:
                blk = CrossAttnUpBlock3D(in_c, out_c, prev_c, ted, layers_per_block + 1, groups, eps, hl[3 - i], xdim, not final, infl, mm(res_on[3 - i]))
            self.up_blocks.append(blk)
        self.conv_norm_out = _norm(infl, groups, boc[0], eps)
        self.conv_act = nn.SiLU()
        self.conv_out = InflatedConv3d(boc[0], out_channels, kernel_size=3, padding=1)
        self._native_handle = None
        self._native_dirty = True
        self._native_fp = None

    # ------------------------------------------------------------------ nn.Module plumbing
    @property
    def config(self):
        return self._internal_dict

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    def _apply(self, fn, *a, **k):
        self._native_dirty = True
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        self._native_dirty = True
        return super().load_state_dict(*a, **k)

    def __getstate__(self):
        """copies and pickles carry the parameters, not the handle (a pointer into the library): the copy builds its own at its first forward"""
        state = dict(self.__dict__)
        state["_native_handle"], state["_native_dirty"], state["_native_fp"] = None, True, None
        state.pop("_native_tensors", None)
        return state

    def __del__(self):
        h = getattr(self, "_native_handle", None)
        if h is not None:
            try:
                _native.load().univst_unet_destroy(h)
            except Exception:
                pass

    # ------------------------------------------------------------------ native handle
    def _motion_cfg(self):
        kw = self.config.motion_module_kwargs
        types_ = tuple(kw.get("attention_block_types", ("Temporal_Self", "Temporal_Self")))
        pe = bool(kw.get("temporal_position_encoding", False))
        max_len = int(kw.get("temporal_position_encoding_max_len", 24))
        return _native.MotionCfg(0, int(kw.get("num_attention_heads", 8)), int(kw.get("num_transformer_block", 2)), len(types_), 32,
                                 max_len if pe else min(max_len, 32), int(pe), 1e-6, 1e-5)

    def _weights_fingerprint(self):
        """(storage address, autograd version counter) of every parameter: see UNetPseudo3DConditionModel._weights_fingerprint.  Edits through
        ``p.data`` are not seen: call ``invalidate_native()`` after them."""
        ts = self.__dict__.get("_native_tensors")
        if ts is None or self._native_dirty or self.__dict__.get("_native_epoch") != _REGISTRATION_EPOCH[0]:
            self.__dict__["_native_epoch"] = _REGISTRATION_EPOCH[0]
            ts = self.__dict__["_native_tensors"] = list(self.state_dict(keep_vars=True).values())
        acc = 0
        for t in ts:
            acc = (acc * 1000003 + t.data_ptr() + 7919 * t._version) & 0xFFFFFFFFFFFFFFFF
        return acc

    def invalidate_native(self):
        """force a rebuild of the native weight copy at the next forward"""
        self._native_dirty = True

    def set_native_option(self, name: str, value: int):
        """tuning switch of the native graph (include/univst.h ``univst_unet_set_option``); survives rebuilds"""
        if getattr(self, "_native_handle", None) is not None:      # (a value the library refuses is not recorded: a later rebuild would raise on it)
            _native.check(_native.load().univst_unet_set_option(self._native_handle, name.encode(), int(value)), f"unet_set_option({name})")
        if not hasattr(self, "_native_options"):
            self._native_options = {}
        self._native_options[name] = int(value)

    def native_query(self, name: str) -> float:
        """read-out of the handle (``univst_unet_query``): "arena_high_water" """
        self._sync_native()
        return _native.unet_query(self._native_handle, name)

    def _sync_native(self):
        lib = _native.load()
        if self.device.type != "cuda":
            raise RuntimeError("UNet3DConditionModel.forward runs only on an AMD GPU: call .cuda() first (univst_amd has no CPU path)")
        fp = self._weights_fingerprint()
        if self._native_handle is not None and not self._native_dirty and fp == self._native_fp:
            return
        if self._native_handle is not None:
            lib.univst_unet_destroy(self._native_handle)
            self._native_handle = None
        c = self.config
        cfg = _native.UnetCfg(c.in_channels, c.out_channels, (C.c_int * 4)(*c.block_out_channels), c.layers_per_block, c.cross_attention_dim,
                              (C.c_int * 4)(*self._heads_per_level), c.norm_num_groups, c.norm_eps, int(c.flip_sin_to_cos), float(c.freq_shift))
        ad = _native.AnimateDiffCfg(int(bool(c.use_inflated_groupnorm)), self._motion_mask, int(self._motion_mid), self._motion_cfg())
        h = _native.load_handle("unet", (C.byref(cfg), C.byref(ad)), self.state_dict().items(), other_dtype=torch.float32,
                                create="univst_unet_create_animatediff", load_what="load_tensor")
        try:
            for k, v in list(getattr(self, "_native_options", {}).items()):
                if lib.univst_unet_set_option(h, k.encode(), int(v)) != 0:
                    del self._native_options[k]      # (recorded before a handle existed: refused now, and not to be met again by the next rebuild)
                    _native.check(-1, f"unet_set_option({k})")
        except Exception:
            lib.univst_unet_destroy(h)
            raise
        self._native_handle = h
        self._native_dirty = False
        self._native_fp = fp

    def _pnp_state(self):
        """read back what pnp_utils.register_spatial_attention_pnp / register_time of this backbone poked into the modules"""
        from ..pnp_utils import ALPHA, GAMMA, PNP_LAYERS
        mods = [self.up_blocks[r].attentions[b].transformer_blocks[0].attn1 for r, bs in PNP_LAYERS.items() for b in bs]
        for m in mods:
            if "forward" in m.__dict__ and not getattr(m, "_univst_native_pnp", False):
                raise RuntimeError("attn1.forward was replaced by a foreign closure; the native UNet cannot call it. "
                                   "Use univst_amd's backbones.animatediff.pnp_utils.register_spatial_attention_pnp instead.")
        reg = [getattr(m, "_univst_native_pnp", False) for m in mods]
        if not any(reg):
            return None
        if not all(reg):
            raise NotImplementedError("PnP registered on a subset of the 8 decoder layers")
        vals = {(getattr(m, "idx", None), float(m.eta1), float(m.eta2)) for m in mods}
        if len(vals) != 1:
            raise NotImplementedError(f"per-layer differing PnP state is not supported: {vals}")
        idx, eta1, eta2 = vals.pop()
        if idx is None:
            raise RuntimeError("PnP registered but register_time() was never called (attn1.idx missing)")
        return _native.PnP(1, int(idx), eta1, eta2, ALPHA, GAMMA)

    # ------------------------------------------------------------------ forward
    @torch.no_grad()
    def forward(self, sample: torch.Tensor, timestep, encoder_hidden_states: torch.Tensor, class_labels=None, attention_mask=None, ft_indices=None,
                ft_timesteps=None, ft_path=None):
        if attention_mask is not None or class_labels is not None:
            raise NotImplementedError("attention_mask / class_labels are not used on the UniVST path")
        if sample.dim() != 5:
            raise ValueError(f"sample must be [B,C,F,H,W], got {tuple(sample.shape)}")
        self._sync_native()
        lib = _native.load()
        B, _, F_, H, W = sample.shape
        x = sample.to(torch.float16).contiguous()
        txt = encoder_hidden_states.to(torch.float16).contiguous()
        if txt.shape[0] != B:
            raise ValueError(f"encoder_hidden_states batch {txt.shape[0]} != sample batch {B}")
        if torch.is_tensor(timestep):
            tv = timestep.reshape(-1)
            if tv.numel() > 1 and not bool((tv == tv[0]).all()):
                raise NotImplementedError("per-sample timesteps are not implemented: the native graph takes one timestep per call")
            t = float(tv[0].item())
        else:
            t = float(timestep)
        eps = torch.empty(B, self.config.out_channels, F_, H, W, device=x.device, dtype=torch.float16)
        feat, ft_index = None, -1
        if ft_indices is not None and ft_timesteps is not None and ft_path is not None:          # unet.py:453-459; as the SD mirror: one block per call
            hits = [i for i in ft_indices if i is not None and 0 <= i < 4]
            tt = int(t) if float(int(t)) == t else t
            if hits and any(tt == v for v in ft_timesteps):
                if len(hits) > 1:
                    raise NotImplementedError("one feature-dump block per call")
                ft_index = hits[0]
                lvl = min(ft_index + 1, 3)
                feat = torch.empty(F_, (H >> 3) << lvl, (W >> 3) << lvl, list(reversed(self.config.block_out_channels))[ft_index], device=x.device,
                                   dtype=torch.float16)
        pnp = self._pnp_state()
        args = (self._native_handle, x.data_ptr(), t, txt.data_ptr(), B, F_, H, W, txt.shape[1], C.byref(pnp) if pnp is not None else None, eps.data_ptr())
        if feat is not None:
            _native.check(lib.univst_unet_forward_tap(*args, feat.data_ptr(), ft_index, _native.stream_ptr()), "unet_forward_tap")
            save_path = os.path.join(ft_path, f"inversion_feature_map_{ft_index}_block_{tt}_step.pt")
            torch.save(feat, save_path)
            print(f"save feature map at: {save_path}")
            self.last_feature_map = feat
        else:
            _native.check(lib.univst_unet_forward(*args, None, -1, _native.stream_ptr()), "unet_forward")
        return UNet3DConditionOutput(sample=eps.to(sample.dtype) if sample.dtype != torch.float16 else eps)

    # ------------------------------------------------------------------ loading (unet.py:468-506)
    @classmethod
    def from_pretrained_2d(cls, pretrained_model_path, subfolder=None, unet_additional_kwargs=None):
        if subfolder is not None:
            pretrained_model_path = os.path.join(pretrained_model_path, subfolder)
        print(f"loaded 3D unet's pretrained weights from {pretrained_model_path} ...")
        config_file = os.path.join(pretrained_model_path, "config.json")
        if not os.path.isfile(config_file):
            raise RuntimeError(f"{config_file} does not exist")
        with open(config_file, "r") as f:
            config = json.load(f)
        config["_class_name"] = cls.__name__
        config["down_block_types"] = list(_DOWN)
        config["up_block_types"] = list(_UP)
        config.pop("mid_block_type", None)           # (a 2-D config names UNetMidBlock2DCrossAttn; the reference's from_config drops what differs in kind)
        config.update(unet_additional_kwargs or {})
        known = set(cls.__init__.__code__.co_varnames)
        model = cls(**{k: v for k, v in config.items() if k in known})
        model_file = os.path.join(pretrained_model_path, WEIGHTS_NAME)
        if not os.path.isfile(model_file):
            raise RuntimeError(f"{model_file} does not exist")
        state_dict = torch.load(model_file, map_location="cpu", weights_only=True)
        m, u = model.load_state_dict(state_dict, strict=False)
        print(f"### missing keys: {len(m)}; \n### unexpected keys: {len(u)};")
        params = [p.numel() if "motion_modules." in n else 0 for n, p in model.named_parameters()]
        print(f"### Motion Module Parameters: {sum(params) / 1e6} M")
        return model
