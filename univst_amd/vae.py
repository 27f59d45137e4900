"""The temporal VAE behind the pipeline's call sites, on the native library.

``NativeTemporalVAE`` stands where the reference keeps diffusers' ``AutoencoderKLTemporalDecoder`` (src/sd/run_video_style_transfer_sd.py:36-42;
used at pipelines/stable_diffusion.py:369-394, :793-834 and inversion_tools/ddim_inversion.py:28-31,52-55): ``.decode(z, num_frames=F).sample``,
``.encode(x).latent_dist.sample()``, ``.config.scaling_factor``, ``.parameters()`` / ``.dtype``, a ``forward`` whose signature carries ``num_frames``
(the pipeline inspects it).  It takes that class's state dict unchanged (``from_module`` wraps a loaded stock VAE, ``from_state_dict`` a checkpoint
dict) and runs one C-ABI call per decode / encode (univst_vae_*, csrc/vae.hip).  The network is third-party: restated from its published definition,
parity unpinned by the reference (see csrc/vae.hip)."""
import ctypes as C
import types

import torch

from . import _native

DEFAULT_CONFIG = dict(in_channels=3, out_channels=3, latent_channels=4, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                      norm_num_groups=32, scaling_factor=0.18215, force_upcast=True)


class _LatentDist:
    """diffusers DiagonalGaussianDistribution over the native encoder's moments (sampling consumes torch's RNG exactly like the stock class)"""

    def __init__(self, moments):
        self.parameters = moments
        self.mean, self.logvar = torch.chunk(moments, 2, dim=1)
        self.logvar = torch.clamp(self.logvar, -30.0, 20.0)
        self.std = torch.exp(0.5 * self.logvar)
        self.var = torch.exp(self.logvar)

    def sample(self, generator=None):
        noise = torch.randn(self.mean.shape, generator=generator, device=self.parameters.device, dtype=self.parameters.dtype)
        return self.mean + self.std * noise

    def mode(self):
        return self.mean


class NativeTemporalVAE(_native.NativeHandle, torch.nn.Module):
    _kind, _noun = "vae", "VAE"

    def __init__(self, state_dict, config=None, device="cuda"):
        super().__init__()
        cfg = self.merge_config(DEFAULT_CONFIG, config, keep_none=True)
        self.config = types.SimpleNamespace(**cfg)
        self._dummy = torch.nn.Parameter(torch.zeros(1, device=device, dtype=torch.float16), requires_grad=False)   # .parameters() / .dtype / .device for the call sites
        c = _native.VaeCfg(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], (C.c_int * 4)(*cfg["block_out_channels"]),
                           cfg["layers_per_block"], cfg["norm_num_groups"])
        self._h = _native.load_handle("vae", (C.byref(c),), state_dict.items(), other_dtype=torch.float16, device=device)

    @classmethod
    def from_module(cls, vae, device="cuda"):
        return cls(vae.state_dict(), config=getattr(vae, "config", None), device=device)

    from_state_dict = classmethod(lambda cls, sd, config=None, device="cuda": cls(sd, config=config, device=device))

    @classmethod
    def from_pretrained(cls, path, subfolder="vae", device="cuda", **_):
        """Load a diffusers-format VAE directory WITHOUT diffusers: ``<path>/<subfolder>/config.json`` + ``diffusion_pytorch_model[.fp16].safetensors``
        (or ``.bin``) — what ``AutoencoderKLTemporalDecoder.from_pretrained(path, subfolder="vae")`` reads (src/sd/run_*_sd.py:36-42).  Local directories
        only (the target boxes have no hub access); raises FileNotFoundError otherwise so that a caller can fall back to diffusers."""
        import json
        import os
        d = os.path.join(path, subfolder) if subfolder else path
        cfg_file = os.path.join(d, "config.json")
        if not os.path.isfile(cfg_file):
            raise FileNotFoundError(f"{cfg_file} not found (NativeTemporalVAE.from_pretrained needs a local diffusers-format directory)")
        with open(cfg_file) as f:
            cfg = {k: v for k, v in json.load(f).items() if not k.startswith("_")}
        cls_name = json.load(open(cfg_file)).get("_class_name", "AutoencoderKLTemporalDecoder")
        if cls_name != "AutoencoderKLTemporalDecoder":
            raise ValueError(f"{cfg_file}: _class_name = {cls_name}; the native VAE restates AutoencoderKLTemporalDecoder only")
        for name in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors", "diffusion_pytorch_model.bin"):
            w = os.path.join(d, name)
            if os.path.isfile(w):
                if name.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(w)
                else:
                    sd = torch.load(w, map_location="cpu")
                return cls(sd, config=cfg, device=device)
        raise FileNotFoundError(f"no diffusion_pytorch_model.safetensors / .bin under {d}")

    @property
    def dtype(self):
        return torch.float16

    @property
    def device(self):
        return self._dummy.device

    def _check(self, t, what):
        return self._gpu_only(t, what).to(torch.float16).contiguous()

    @torch.no_grad()
    def decode(self, z, num_frames=1, return_dict=True, **_):
        z = self._check(z, "decode")
        n, c, h, w = z.shape
        out = torch.empty(n, self.config.out_channels, 8 * h, 8 * w, device=z.device, dtype=torch.float16)
        _native.check(_native.load().univst_vae_decode(self._h, _native.ptr(z), n, int(num_frames), h, w, _native.ptr(out), _native.stream_ptr()), "vae_decode")
        return types.SimpleNamespace(sample=out) if return_dict else (out,)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        x = self._check(x, "encode")
        n, c, H, W = x.shape
        mom = torch.empty(n, 2 * self.config.latent_channels, H // 8, W // 8, device=x.device, dtype=torch.float16)
        _native.check(_native.load().univst_vae_encode(self._h, _native.ptr(x), n, H, W, _native.ptr(mom), _native.stream_ptr()), "vae_encode")
        d = _LatentDist(mom)
        return types.SimpleNamespace(latent_dist=d) if return_dict else (d,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None, num_frames=1):
        d = self.encode(sample).latent_dist
        z = d.sample(generator=generator) if sample_posterior else d.mode()
        return self.decode(z, num_frames=num_frames, return_dict=return_dict)

    def enable_slicing(self):
        pass

    def disable_slicing(self):
        pass


# ---------------------------------------------------------------------------------------------- the plain AutoencoderKL (SD3 / SD3.5, SD-v1.5's image VAE)
KL_DEFAULT_CONFIG = dict(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=(128, 256, 512, 512), layers_per_block=2,
                         norm_num_groups=32, scaling_factor=1.5305, shift_factor=0.0609, use_quant_conv=False, use_post_quant_conv=False,
                         force_upcast=True)

_OLD_ATTENTION_NAMES = {"query": "to_q", "key": "to_k", "value": "to_v", "proj_attn": "to_out.0"}


def kl_tensors(state_dict):
    """The tensors of an ``AutoencoderKL`` checkpoint as the handle takes them (a pure function; runs before upload).  Checkpoints written before
    diffusers 0.18 — SD-v1.5's ``vae/`` among them — name the mid-block attention ``query / key / value / proj_attn`` and sometimes keep its weights
    as 1x1 convolutions ``[C, C, 1, 1]``: they become ``to_q / to_k / to_v / to_out.0`` with ``[C, C]`` weights, as diffusers does on load.  Entries
    that are not floating point (integer buffers) are dropped; everything else passes through untouched."""
    out = {}
    for k, t in state_dict.items():
        if not torch.is_floating_point(t):
            continue
        parts = k.split(".")
        if ".attentions." in k:
            if len(parts) >= 2 and parts[-2] in _OLD_ATTENTION_NAMES:
                k = ".".join(parts[:-2] + [_OLD_ATTENTION_NAMES[parts[-2]], parts[-1]])
            if k.endswith(".weight") and t.dim() == 4 and t.shape[2] == t.shape[3] == 1 and ".group_norm." not in k:
                t = t.reshape(t.shape[0], t.shape[1])
        out[k] = t
    return out


def kl_config_from_dir(path, subfolder="vae"):
    """``<path>/<subfolder>/config.json`` of a diffusers-format directory -> (directory, config without the underscore keys); refuses anything but a
    plain ``AutoencoderKL`` with attention in its mid block.  No diffusers import."""
    import json
    import os
    d = os.path.join(path, subfolder) if subfolder else path
    cfg_file = os.path.join(d, "config.json")
    if not os.path.isfile(cfg_file):
        raise FileNotFoundError(f"{cfg_file} not found (NativeAutoencoderKL.from_pretrained needs a local diffusers-format directory)")
    with open(cfg_file) as f:
        raw = json.load(f)
    cls_name = raw.get("_class_name", "AutoencoderKL")
    if cls_name != "AutoencoderKL":
        raise ValueError(f"{cfg_file}: _class_name = {cls_name}; the native VAE of the SD3 path restates AutoencoderKL only")
    for key, want in (("down_block_types", "DownEncoderBlock2D"), ("up_block_types", "UpDecoderBlock2D")):
        got = raw.get(key, [want] * 4)
        if list(got) != [want] * 4:
            raise ValueError(f"{cfg_file}: {key} = {list(got)}; only four plain {want} blocks are restated")
    if not raw.get("mid_block_add_attention", True):
        raise ValueError(f"{cfg_file}: mid_block_add_attention = false; the restated mid block has its attention")
    return d, {k: v for k, v in raw.items() if not k.startswith("_")}


class NativeAutoencoderKL(_native.NativeHandle, torch.nn.Module):
    """Stands where the SD3 pipeline keeps diffusers' ``AutoencoderKL`` (src/sd3/run_*_sd3.py; used at custom_pipeline.py ``_decode`` and
    inversion_tools/flow_inversion.py ``_img_latents``): ``.decode(z, return_dict=False)[0]`` / ``.decode(z).sample``, ``.encode(x).latent_dist.sample()``,
    ``.config.scaling_factor`` / ``.shift_factor``, ``.parameters()``.  It takes that class's state dict (old attention names included, ``kl_tensors``) and
    runs one C-ABI call per decode / encode (univst_klvae_*, csrc/vae.hip).  The scale and shift stay with the call sites.

    ``force_upcast`` is read and ignored: the handle computes in fp16 with fp32 accumulation, as the reference's ``vae.to(weight_dtype)`` does.
    ``attn_score_bytes`` / ``pass_bytes`` (0: 128 MiB / 8 GiB) bound the attention's score matrix and the activation arena (include/univst.h).
    The network is third-party: restated from its published definition, parity unpinned (tests/klvae_ref.py is a second restatement)."""

    _kind, _noun = "klvae", "VAE"

    def __init__(self, state_dict, config=None, device="cuda", attn_score_bytes=0, pass_bytes=0):
        super().__init__()
        cfg = self.merge_config(KL_DEFAULT_CONFIG, config, keep_none=True)
        if cfg["shift_factor"] is None:      # SD-v1.5's config
            cfg["shift_factor"] = 0.0
        cfg["block_out_channels"] = tuple(cfg["block_out_channels"])
        self.config = types.SimpleNamespace(**cfg)
        self._dummy = torch.nn.Parameter(torch.zeros(1, device=device, dtype=torch.float16), requires_grad=False)   # .parameters() / .dtype / .device for the call sites
        c = _native.KlVaeCfg(cfg["in_channels"], cfg["out_channels"], cfg["latent_channels"], (C.c_int * 4)(*cfg["block_out_channels"]),
                             cfg["layers_per_block"], cfg["norm_num_groups"], int(bool(cfg["use_quant_conv"])), int(bool(cfg["use_post_quant_conv"])),
                             int(attn_score_bytes), int(pass_bytes))
        self._h = _native.load_handle("klvae", (C.byref(c),), kl_tensors(state_dict).items(), other_dtype=torch.float16, device=device)

    @classmethod
    def from_module(cls, vae, device="cuda", **kw):
        return cls(vae.state_dict(), config=getattr(vae, "config", None), device=device, **kw)

    from_state_dict = classmethod(lambda cls, sd, config=None, device="cuda", **kw: cls(sd, config=config, device=device, **kw))

    @classmethod
    def from_pretrained(cls, path, subfolder="vae", device="cuda", attn_score_bytes=0, pass_bytes=0, **_):
        """Load a diffusers-format VAE directory WITHOUT diffusers: ``<path>/<subfolder>/config.json`` + ``diffusion_pytorch_model[.fp16].safetensors``
        (or ``.bin``) — what ``AutoencoderKL.from_pretrained(path, subfolder="vae")`` reads.  Local directories only."""
        import os
        d, cfg = kl_config_from_dir(path, subfolder)
        for name in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.fp16.safetensors", "diffusion_pytorch_model.bin"):
            w = os.path.join(d, name)
            if os.path.isfile(w):
                if name.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(w)
                else:
                    sd = torch.load(w, map_location="cpu")
                return cls(sd, config=cfg, device=device, attn_score_bytes=attn_score_bytes, pass_bytes=pass_bytes)
        raise FileNotFoundError(f"no diffusion_pytorch_model.safetensors / .bin under {d}")

    @property
    def dtype(self):
        return torch.float16

    @property
    def device(self):
        return self._dummy.device

    def _check(self, t, what):
        return self._gpu_only(t, what).to(torch.float16).contiguous()

    @torch.no_grad()
    def decode(self, z, return_dict=True, **_):
        z = self._check(z, "decode")
        n, c, h, w = z.shape
        if c != self.config.latent_channels:
            raise RuntimeError(f"NativeAutoencoderKL.decode: latents have {c} channels, the VAE has latent_channels = {self.config.latent_channels}")
        out = torch.empty(n, self.config.out_channels, 8 * h, 8 * w, device=z.device, dtype=torch.float16)
        _native.check(_native.load().univst_klvae_decode(self._h, _native.ptr(z), n, h, w, _native.ptr(out), _native.stream_ptr()), "klvae_decode")
        return types.SimpleNamespace(sample=out) if return_dict else (out,)

    @torch.no_grad()
    def encode(self, x, return_dict=True):
        x = self._check(x, "encode")
        n, c, H, W = x.shape
        if c != self.config.in_channels:
            raise RuntimeError(f"NativeAutoencoderKL.encode: images have {c} channels, the VAE has in_channels = {self.config.in_channels}")
        mom = torch.empty(n, 2 * self.config.latent_channels, H // 8, W // 8, device=x.device, dtype=torch.float16)
        _native.check(_native.load().univst_klvae_encode(self._h, _native.ptr(x), n, H, W, _native.ptr(mom), _native.stream_ptr()), "klvae_encode")
        d = _LatentDist(mom)
        return types.SimpleNamespace(latent_dist=d) if return_dict else (d,)

    def forward(self, sample, sample_posterior=False, return_dict=True, generator=None):
        d = self.encode(sample).latent_dist
        z = d.sample(generator=generator) if sample_posterior else d.mode()
        return self.decode(z, return_dict=return_dict)

    def enable_slicing(self):
        pass

    def disable_slicing(self):
        pass

    def enable_tiling(self, *a, **kw):
        pass

    def disable_tiling(self):
        pass
