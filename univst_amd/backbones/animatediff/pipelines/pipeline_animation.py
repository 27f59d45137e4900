"""Host-side mirror of ``AnimationPipeline`` (backbones/animatediff/pipelines/pipeline_animation.py:50-603 of the reference).

Same constructor, same ``reconstruction`` / ``video_style_transfer`` signatures, result in ``.images``.  The denoising loops run through
univst_amd.engine on the native AnimateDiff UNet (one C-ABI call per step); the inversion latents and the masks are read ONCE before the loop
and stay on the device (the reference re-reads 2 x 51 latent files and 16 mask PNGs on every step, :505-517).  What this backbone's loop has
that the SD loop has not, and what ``engine.transfer_loop`` is told:

    latent AdaIN window   0.8 n <= i <= 0.9 n (:515, inclusive at the bottom; the SD loop starts after 0.8 n)
    register_time         this backbone's (backbones/animatediff/pnp_utils.py: the window eta1 * 50 <= idx < eta2 * 50, alpha 0.8, gamma 2.0)
    skip_dead_branches    the window is closed from i >= eta2 * 50 on (exclusive at the top)

Extras, as on the SD mirror (reference defaults unchanged): ``content_inv_latents`` / ``style_inv_latents`` / ``masks`` take in-memory tensors
instead of paths, ``output_type='latent'`` skips the VAE, ``skip_dead_branches``.

Not built for this pipeline and refused by name: the sliding-window ``smoother`` (dead code in the reference, ``smoother = None`` at :540),
frame sharding (``shard``: the frame-axis attention of the motion modules needs every frame on one GPU), ``eta != 0``, and a ``controlnet``
(SparseControlNet is constructed by nothing and called by neither loop of the reference)."""
import inspect

import torch

from .... import engine
from ....src.util import load_ddim_latents_at_t, load_mask
from ..pnp_utils import latent_adain, register_time  # noqa: F401  (re-exported like the reference module)


class AnimationPipelineOutput:
    def __init__(self, images):
        self.images = images


def _window_closed(i, eta2):
    return i >= eta2 * 50


class AnimationPipeline:
    _optional_components = []

    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, controlnet=None):
        if controlnet is not None:
            raise NotImplementedError("AnimationPipeline(controlnet=...): SparseControlNet (models/sparse_controlnet.py) is not built; "
                                      "neither loop of the reference calls it")
        if hasattr(scheduler.config, "steps_offset") and scheduler.config.steps_offset != 1:
            raise ValueError("scheduler.config.steps_offset must be 1 (animatediff-v2.yaml noise_scheduler_kwargs)")
        if hasattr(scheduler.config, "clip_sample") and scheduler.config.clip_sample is True:
            raise ValueError("scheduler.config.clip_sample must be False")
        self.vae, self.text_encoder, self.tokenizer, self.unet, self.scheduler = vae, text_encoder, tokenizer, unet, scheduler
        self.controlnet = None
        boc = getattr(getattr(vae, "config", None), "block_out_channels", (1, 1, 1, 1))
        self.vae_scale_factor = 2 ** (len(boc) - 1)

    @property
    def device(self):
        return self.unet.device

    @property
    def _execution_device(self):
        return self.device

    def enable_vae_slicing(self):
        self.vae.enable_slicing()

    def disable_vae_slicing(self):
        self.vae.disable_slicing()

    # ------------------------------------------------------------------ prompt (:160-247)
    def _encode_prompt(self, prompt, device, num_videos_per_prompt, do_classifier_free_guidance, negative_prompt):
        batch_size = len(prompt) if isinstance(prompt, list) else 1
        ti = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True, return_tensors="pt")
        am = None
        if getattr(getattr(self.text_encoder, "config", None), "use_attention_mask", False):
            am = ti.attention_mask.to(device)
        emb = self.text_encoder(ti.input_ids.to(device), attention_mask=am)[0]
        bs, seq, _ = emb.shape
        emb = emb.repeat(1, num_videos_per_prompt, 1).view(bs * num_videos_per_prompt, seq, -1)
        if do_classifier_free_guidance:
            if negative_prompt is None:
                un = [""] * batch_size
            elif type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} != {type(prompt)}.")
            elif isinstance(negative_prompt, str):
                un = [negative_prompt]
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`: {prompt} has batch size"
                                 f" {batch_size}. Please make sure that passed `negative_prompt` matches the batch size of `prompt`.")
            else:
                un = negative_prompt
            ui = self.tokenizer(un, padding="max_length", max_length=ti.input_ids.shape[-1], truncation=True, return_tensors="pt")
            if am is not None:
                am = ui.attention_mask.to(device)
            ue = self.text_encoder(ui.input_ids.to(device), attention_mask=am)[0]
            ue = ue.repeat(1, num_videos_per_prompt, 1).view(batch_size * num_videos_per_prompt, ue.shape[1], -1)
            emb = torch.cat([ue, emb])
        return emb

    # ------------------------------------------------------------------ VAE (:249-274)
    def decode_latents(self, latents, num_frames=16, decode_chunk_size=16):
        """[b,4,F,h,w] -> numpy [b,F,H,W,3] in [0,1].  The frames are regrouped by the clip's OWN frame count ``latents.shape[2]``; the reference
        hard-codes ``f=16`` there (:270), so the two are equal at 16 frames, the only length the reference's loops run.  ``num_frames`` is kept
        for the signature and, as in the reference, not used."""
        F_ = latents.shape[2]
        z = latents.permute(0, 2, 1, 3, 4).contiguous().flatten(0, 1)
        z = 1 / self.vae.config.scaling_factor * z
        accepts = "num_frames" in set(inspect.signature(self.vae.forward).parameters.keys())
        frames = []
        for i in range(0, z.shape[0], decode_chunk_size):
            zi = z[i:i + decode_chunk_size].to(next(self.vae.parameters()).dtype)
            frames.append(self.vae.decode(zi, **({"num_frames": zi.shape[0]} if accepts else {})).sample)
        frames = (torch.cat(frames, dim=0) / 2 + 0.5).clamp(0, 1)
        n, c, h, w = frames.shape
        return frames.view(n // F_, F_, c, h, w).permute(0, 1, 3, 4, 2).cpu().float().numpy()

    def prepare_extra_step_kwargs(self, generator, eta):
        keys = set(inspect.signature(self.scheduler.step).parameters.keys())
        kw = {}
        if "eta" in keys:
            kw["eta"] = eta
        if "generator" in keys:
            kw["generator"] = generator
        return kw

    def check_inputs(self, prompt, height, width, callback_steps):
        """:293-306: same conditions, same messages."""
        if not isinstance(prompt, str) and not isinstance(prompt, list):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if (callback_steps is None) or (callback_steps is not None and (not isinstance(callback_steps, int) or callback_steps <= 0)):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type {type(callback_steps)}.")

    def prepare_latents(self, batch_size, num_channels_latents, video_length, height, width, dtype, device, generator, latents=None):
        """:308-335 (a list of generators draws the FULL shape once per generator and concatenates, as the reference does)."""
        shape = (batch_size, num_channels_latents, video_length, height // self.vae_scale_factor, width // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            if isinstance(generator, list):
                latents = torch.cat([torch.randn(shape, generator=generator[i], device=device, dtype=dtype) for i in range(batch_size)], dim=0)
            else:
                latents = torch.randn(shape, generator=generator, device=device, dtype=dtype)
        else:
            if tuple(latents.shape) != shape:
                raise ValueError(f"Unexpected latents shape, got {latents.shape}, expected {shape}")
            latents = latents.to(device)
        return latents * getattr(self.scheduler, "init_noise_sigma", 1.0)

    def _finish(self, latents, output_type, return_dict):
        if output_type == "latent":
            video = latents
        else:
            video = self.decode_latents(latents)
            if output_type == "tensor":
                video = torch.from_numpy(video)
        if not return_dict:
            return video
        return AnimationPipelineOutput(images=video)

    # ------------------------------------------------------------------ reconstruction (:337-446)
    @torch.no_grad()
    def reconstruction(self, prompt, video_length, height=None, width=None, num_inference_steps=50, guidance_scale=7.5, negative_prompt=None,
                       num_videos_per_prompt=1, eta=0.0, generator=None, latents=None, output_type="tensor", return_dict=True, callback=None,
                       callback_steps=1, **kwargs):
        if eta != 0.0:
            raise NotImplementedError("AnimationPipeline.reconstruction: eta != 0 is not built (the DDIM update is the deterministic one)")
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, height, width, callback_steps)
        batch_size = 1
        if latents is not None:
            batch_size = latents.shape[0]
        if isinstance(prompt, list):
            batch_size = len(prompt)
        device = self._execution_device
        cfg = guidance_scale > 1.0
        prompt = prompt if isinstance(prompt, list) else [prompt] * batch_size
        if negative_prompt is not None:
            negative_prompt = negative_prompt if isinstance(negative_prompt, list) else [negative_prompt] * batch_size
        text = self._encode_prompt(prompt, device, num_videos_per_prompt, cfg, negative_prompt)
        self.scheduler.set_timesteps(num_inference_steps)
        latents = self.prepare_latents(batch_size * num_videos_per_prompt, self.unet.config.in_channels, video_length, height, width, text.dtype,
                                       device, generator, latents)
        latents = latents.to(device=device, dtype=torch.float16).contiguous()
        timesteps = [int(t) for t in self.scheduler.timesteps.tolist()]
        for i, t in enumerate(timesteps):
            x = torch.cat([latents] * 2) if cfg else latents
            eps = self.unet(x, t, encoder_hidden_states=text).sample
            if cfg:
                eu, et = eps.chunk(2)
                eps = (eu.float() + guidance_scale * (et.float() - eu.float())).to(torch.float16)
            latents = engine.ddim_step(self.scheduler, eps, t, latents)
            if callback is not None and i % callback_steps == 0:
                callback(i, self.scheduler.timesteps[i], latents)
        return self._finish(latents, output_type, return_dict)

    # ------------------------------------------------------------------ video_style_transfer (:448-603)
    @torch.no_grad()
    def video_style_transfer(self, prompt, num_inference_steps=50, negative_prompt=None, num_videos_per_prompt=1, eta=0.0, generator=None,
                             latents=None, output_type="tensor", return_dict=True, callback=None, callback_steps=1, content_inv_path=None,
                             style_inv_path=None, mask_path=None, content_inv_latents=None, style_inv_latents=None, masks=None,
                             skip_dead_branches=False, smoother=None, shard=None, **kwargs):
        if eta != 0.0:
            raise NotImplementedError("AnimationPipeline.video_style_transfer: eta != 0 is not built (the DDIM update is the deterministic one)")
        if smoother is not None:
            raise NotImplementedError("AnimationPipeline.video_style_transfer: smoother is not built for the AnimateDiff pipeline "
                                      "(the reference hard-wires smoother = None, pipeline_animation.py:540)")
        if shard not in (None, False):
            raise NotImplementedError("AnimationPipeline.video_style_transfer: frame sharding (shard) is not built for the AnimateDiff pipeline: "
                                      "the motion modules attend over all frames of a pixel")
        device = self._execution_device
        n = num_inference_steps
        pe = self._encode_prompt(prompt, device, num_videos_per_prompt, False, negative_prompt)
        ie = self._encode_prompt("", device, num_videos_per_prompt, False, None)
        text3 = torch.cat([ie, ie, pe])
        F_ = latents.shape[2]
        if content_inv_latents is None:
            content_inv_latents = [load_ddim_latents_at_t(k, content_inv_path) for k in range(n + 1)]
        if style_inv_latents is None:
            style_inv_latents = [load_ddim_latents_at_t(k, style_inv_path) for k in range(n + 1)]
        if masks is None and mask_path:
            masks = load_mask(mask_path, n_frames=F_)
        cb = (lambda i, t, l: callback(i, t, l) if i % callback_steps == 0 else None) if callback is not None else None
        latents = engine.transfer_loop(self, latents.to(device), text3, content_inv_latents, style_inv_latents, masks, n, callback=cb,
                                       skip_dead_branches=skip_dead_branches, adain_from_inclusive=True, register_time_fn=register_time,
                                       pnp_window_closed=_window_closed)
        return self._finish(latents, output_type, return_dict)
