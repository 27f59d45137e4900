"""The CLIP text tower behind the pipelines' ``text_encoder`` call sites, on the native library.

``NativeCLIPText`` stands where the reference keeps transformers' ``CLIPTextModel`` (SD-v1.5 / v2.1: src/sd/run_*_sd.py, called at
pipelines/stable_diffusion.py _encode_prompt and inversion_tools/ddim_inversion.py) or ``CLIPTextModelWithProjection`` (SD3 / SD3.5: both CLIP towers,
pipelines/custom_pipeline.py _get_clip_prompt_embeds): ``enc(ids)[0]``, ``enc(ids, output_hidden_states=True).hidden_states[-2]``, ``.config``,
``.dtype``, ``.device``, ``.to(...)``.  It takes that class's state dict unchanged — keys with or without the ``text_model.`` prefix — and runs one
C-ABI call per encode (univst_clip_*, csrc/clip.hip).  The network is third-party: restated from its published definition; tests/clip_ref.py is the
yardstick, held to transformers by tests/test_clip_ref.py.  The tokenizers stay transformers' (host code).

``NativeT5Encoder`` (below) does the same for SD3 / SD3.5's ``text_encoder_3`` (transformers' ``T5EncoderModel``; univst_t5_*, csrc/t5.hip)."""
import ctypes as C
import types

import torch

from . import _native

DEFAULT_CONFIG = dict(vocab_size=49408, hidden_size=768, intermediate_size=3072, num_hidden_layers=12, num_attention_heads=12,
                      max_position_embeddings=77, hidden_act="quick_gelu", layer_norm_eps=1e-5, projection_dim=768, eos_token_id=2)
_ACTS = {"quick_gelu": 0, "gelu": 1}


class CLIPTextOutput:
    """what the call sites read of transformers' BaseModelOutputWithPooling / CLIPTextModelOutput: attributes, and ``out[0]`` = the first field
    (last_hidden_state for the plain model, text_embeds for the projected one)"""

    def __init__(self, fields):
        self._fields = [(k, v) for k, v in fields if v is not None]
        for k, v in fields:
            setattr(self, k, v)

    def to_tuple(self):
        return tuple(v for _, v in self._fields)

    def __getitem__(self, i):
        return dict(self._fields)[i] if isinstance(i, str) else self.to_tuple()[i]

    def __len__(self):
        return len(self._fields)


class NativeCLIPText(_native.NativeModuleFacade):
    _kind, _noun = "clip", "text encoder"

    def __init__(self, state_dict, config=None, with_projection=None, device="cuda"):
        cfg = self.merge_config(DEFAULT_CONFIG, config)
        if with_projection is None:
            with_projection = "text_projection.weight" in state_dict
        if cfg["hidden_act"] not in _ACTS:
            raise ValueError(f"NativeCLIPText: hidden_act {cfg['hidden_act']!r} (the native tower has quick_gelu and gelu)")
        self.with_projection = bool(with_projection)
        self.config = types.SimpleNamespace(use_attention_mask=False, **cfg)
        self.device = torch.device(device)
        c = _native.ClipCfg(cfg["vocab_size"], cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"],
                            cfg["max_position_embeddings"], _ACTS[cfg["hidden_act"]], cfg["layer_norm_eps"],
                            cfg["projection_dim"] if self.with_projection else 0, cfg["eos_token_id"])
        # (old checkpoints carry embeddings.position_ids, an int64 buffer)
        items = [(k, v) for k, v in state_dict.items() if torch.is_tensor(v) and v.is_floating_point() and (self.with_projection or k != "text_projection.weight")]
        self._h = _native.load_handle("clip", (C.byref(c),), items, other_dtype=torch.float16, device=device)

    @classmethod
    def from_module(cls, m, device="cuda"):
        """a loaded transformers CLIPTextModel / CLIPTextModelWithProjection"""
        return cls(m.state_dict(), config=m.config, with_projection=hasattr(m, "text_projection"), device=device)

    from_state_dict = classmethod(lambda cls, sd, config=None, with_projection=None, device="cuda": cls(sd, config, with_projection, device))

    @classmethod
    def from_pretrained(cls, path, subfolder="text_encoder", device="cuda", **_):
        """Load a transformers-format text-encoder directory WITHOUT transformers: ``<path>/<subfolder>/config.json`` + ``model.safetensors`` /
        ``model.fp16.safetensors`` / ``pytorch_model.bin`` — what ``CLIPTextModel.from_pretrained(path, subfolder="text_encoder")`` reads.  Local
        directories only (the target boxes have no hub access); raises FileNotFoundError otherwise.  ``architectures`` (or ``_class_name``) of the
        config says whether the tower carries text_projection."""
        import json
        import os
        d = os.path.join(path, subfolder) if subfolder else path
        cfg_file = os.path.join(d, "config.json")
        if not os.path.isfile(cfg_file):
            raise FileNotFoundError(f"{cfg_file} not found (NativeCLIPText.from_pretrained needs a local transformers-format directory)")
        with open(cfg_file) as f:
            raw = json.load(f)
        if isinstance(raw.get("text_config"), dict):      # a CLIPConfig with the tower's settings nested
            raw = {**raw, **raw["text_config"]}
        names = list(raw.get("architectures") or []) + [raw.get("_class_name") or ""]
        if not any(n in ("CLIPTextModel", "CLIPTextModelWithProjection") for n in names):
            raise ValueError(f"{cfg_file}: architectures = {names}; the native text tower restates CLIPTextModel / CLIPTextModelWithProjection only")
        for name in ("model.safetensors", "model.fp16.safetensors", "pytorch_model.bin"):
            w = os.path.join(d, name)
            if os.path.isfile(w):
                if name.endswith(".safetensors"):
                    from safetensors.torch import load_file
                    sd = load_file(w)
                else:
                    sd = torch.load(w, map_location="cpu")
                return cls(sd, config=raw, with_projection="CLIPTextModelWithProjection" in names, device=device)
        raise FileNotFoundError(f"no model.safetensors / model.fp16.safetensors / pytorch_model.bin under {d}")

    def arena_high_water(self):
        return self.query("arena_high_water")

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True, **_):
        ids = self._gpu_only(input_ids, "__call__")
        if ids.dim() != 2 or ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"NativeCLIPText: input_ids must be an integer tensor [B, S], got {ids.dtype} {tuple(ids.shape)}")
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise NotImplementedError("NativeCLIPText: a padding attention_mask is not implemented (no UniVST configuration sets use_attention_mask)")
        ids = ids.to(torch.int64).contiguous()
        B, S = ids.shape
        cfg = self.config
        if S < 1 or S > cfg.max_position_embeddings:
            raise ValueError(f"NativeCLIPText: sequence length {S} exceeds max_position_embeddings {cfg.max_position_embeddings}")
        lo, hi = int(ids.min()), int(ids.max())       # one range check per call; the kernel clamps regardless
        if lo < 0 or hi >= cfg.vocab_size:
            raise IndexError(f"NativeCLIPText: input id {lo if lo < 0 else hi} is outside the vocabulary [0, {cfg.vocab_size})")
        Cw, L = cfg.hidden_size, cfg.num_hidden_layers
        last = torch.empty(B, S, Cw, device=ids.device, dtype=torch.float16)
        hs = torch.empty(L + 1, B, S, Cw, device=ids.device, dtype=torch.float16) if output_hidden_states else None
        pooled = torch.empty(B, cfg.projection_dim if self.with_projection else Cw, device=ids.device, dtype=torch.float16)
        _native.check(_native.load().univst_clip_encode(self._h, _native.ptr(ids), B, S, _native.ptr(last), _native.ptr(hs), _native.ptr(pooled),
                                                        _native.stream_ptr()), "clip_encode")
        hidden = tuple(hs.unbind(0)) if hs is not None else None
        if self.with_projection:
            out = CLIPTextOutput([("text_embeds", pooled), ("last_hidden_state", last), ("hidden_states", hidden)])
        else:
            out = CLIPTextOutput([("last_hidden_state", last), ("pooler_output", pooled), ("hidden_states", hidden)])
        return out if return_dict else out.to_tuple()

    forward = __call__


# ------------------------------------------------------------------------------------------------------------------------ T5 (SD3 / SD3.5 text_encoder_3)
T5_DEFAULT_CONFIG = dict(vocab_size=32128, d_model=4096, d_ff=10240, num_layers=24, num_heads=64, d_kv=64, relative_attention_num_buckets=32,
                         relative_attention_max_distance=128, layer_norm_epsilon=1e-6, feed_forward_proj="gated-gelu")
T5_MAX_S = 512
_T5_EMBED_KEYS = ("shared.weight", "encoder.embed_tokens.weight")


class T5EncoderOutput(CLIPTextOutput):
    """what the call site reads of transformers' BaseModelOutput: ``out[0]`` and ``out.last_hidden_state`` are the same tensor"""

    def __init__(self, last_hidden_state):
        super().__init__([("last_hidden_state", last_hidden_state)])


def read_weight_files(d):
    """The state dict of a transformers-format model directory, read WITHOUT transformers and without touching the native library: the first of
    ``model.safetensors``, ``model.fp16.safetensors``, the sharded ``model.safetensors.index.json`` / ``model.fp16.safetensors.index.json`` (every
    file its ``weight_map`` names, e.g. ``model-00001-of-00002.safetensors``: SD3 checkpoints ship T5 in two shards) and ``pytorch_model.bin``."""
    import json
    import os
    for name in ("model.safetensors", "model.fp16.safetensors", "model.safetensors.index.json", "model.fp16.safetensors.index.json", "pytorch_model.bin"):
        w = os.path.join(d, name)
        if not os.path.isfile(w):
            continue
        if name.endswith(".index.json"):
            from safetensors.torch import load_file
            with open(w) as f:
                weight_map = json.load(f)["weight_map"]
            sd = {}
            for shard in sorted(set(weight_map.values())):
                part = os.path.join(d, shard)
                if not os.path.isfile(part):
                    raise FileNotFoundError(f"{w} names {shard}, which is not in {d}")
                sd.update(load_file(part))
            lost = sorted(set(weight_map) - set(sd))
            if lost:
                raise KeyError(f"{w}: {lost[0]} (and {len(lost) - 1} more) are in the weight_map but in none of its files")
            return sd
        if name.endswith(".safetensors"):
            from safetensors.torch import load_file
            return load_file(w)
        return torch.load(w, map_location="cpu")
    raise FileNotFoundError(f"no model.safetensors / model.fp16.safetensors / model.safetensors.index.json / pytorch_model.bin under {d}")


def t5_tensors(state_dict):
    """the entries of a T5 state dict the encoder takes: floating-point ``encoder.*`` tensors and ONE copy of the tied embedding (``shared.weight``
    or ``encoder.embed_tokens.weight``, whichever comes first), under the name ``shared.weight``; a full T5's decoder / lm_head are left out"""
    out = {}
    for k, v in state_dict.items():
        if not torch.is_tensor(v) or not v.is_floating_point():
            continue
        if k in _T5_EMBED_KEYS:
            out.setdefault("shared.weight", v)
        elif k.startswith("encoder."):
            out[k] = v
    return out


def t5_config_from_dir(path, subfolder="text_encoder_3"):
    """``<path>/<subfolder>/config.json`` of a local transformers-format T5 encoder directory -> (directory, config dict); refuses other architectures
    and feed-forward forms before any weight is read"""
    import json
    import os
    d = os.path.join(path, subfolder) if subfolder else path
    cfg_file = os.path.join(d, "config.json")
    if not os.path.isfile(cfg_file):
        raise FileNotFoundError(f"{cfg_file} not found (NativeT5Encoder.from_pretrained needs a local transformers-format directory)")
    with open(cfg_file) as f:
        raw = json.load(f)
    names = list(raw.get("architectures") or []) + [raw.get("_class_name") or ""]
    if "T5EncoderModel" not in names:
        raise ValueError(f"{cfg_file}: architectures = {names}; the native encoder restates T5EncoderModel only")
    ffp = raw.get("feed_forward_proj", "relu")
    if ffp != "gated-gelu":
        raise ValueError(f"{cfg_file}: feed_forward_proj = {ffp!r}; the native encoder has the gated-gelu (T5 v1.1) feed-forward only")
    return d, raw


class NativeT5Encoder(_native.NativeModuleFacade):
    """transformers' ``T5EncoderModel`` (SD3 / SD3.5 ``text_encoder_3``, T5 v1.1-XXL) on the native library: ``enc(ids)[0]`` =
    ``enc(ids).last_hidden_state`` fp16 [B, S, d_model], one C-ABI call per encode (univst_t5_*, csrc/t5.hip), with an fp32 residual stream.  It takes
    that class's state dict unchanged.  tests/t5_ref.py is the yardstick, held to transformers by tests/test_t5_ref.py."""

    _kind, _noun = "t5", "text encoder"

    def __init__(self, state_dict, config=None, device="cuda"):
        cfg = self.merge_config(T5_DEFAULT_CONFIG, config)
        if cfg["feed_forward_proj"] != "gated-gelu":
            raise ValueError(f"NativeT5Encoder: feed_forward_proj {cfg['feed_forward_proj']!r} (the native encoder has gated-gelu only)")
        self.config = types.SimpleNamespace(**cfg)
        self.device = torch.device(device)
        c = _native.T5Cfg(cfg["vocab_size"], cfg["d_model"], cfg["d_ff"], cfg["num_layers"], cfg["num_heads"], cfg["d_kv"],
                          cfg["relative_attention_num_buckets"], cfg["relative_attention_max_distance"], cfg["layer_norm_epsilon"])
        self._h = _native.load_handle("t5", (C.byref(c),), t5_tensors(state_dict).items(), other_dtype=torch.float16, device=device)

    @classmethod
    def from_module(cls, m, device="cuda"):
        """a loaded transformers T5EncoderModel"""
        return cls(m.state_dict(), config=m.config, device=device)

    from_state_dict = classmethod(lambda cls, sd, config=None, device="cuda": cls(sd, config, device))

    @classmethod
    def from_pretrained(cls, path, subfolder="text_encoder_3", device="cuda", **_):
        """Load a transformers-format T5 encoder directory WITHOUT transformers: ``<path>/<subfolder>/config.json`` + the weight files
        ``read_weight_files`` knows.  Local directories only; raises FileNotFoundError otherwise."""
        d, raw = t5_config_from_dir(path, subfolder)
        return cls(read_weight_files(d), config=raw, device=device)

    def arena_high_water(self):
        return self.query("arena_high_water")

    @torch.no_grad()
    def __call__(self, input_ids, attention_mask=None, output_hidden_states=False, return_dict=True, **_):
        ids = self._gpu_only(input_ids, "__call__")
        if ids.dim() != 2 or ids.dtype not in (torch.int64, torch.int32):
            raise ValueError(f"NativeT5Encoder: input_ids must be an integer tensor [B, S], got {ids.dtype} {tuple(ids.shape)}")
        if output_hidden_states:
            raise NotImplementedError("NativeT5Encoder: hidden_states outputs are not implemented (the pipeline reads the last hidden state only)")
        if attention_mask is not None and not bool((attention_mask != 0).all()):
            raise NotImplementedError("NativeT5Encoder: a padding attention_mask is not implemented (the pipeline passes none)")
        ids = ids.to(torch.int64).contiguous()
        B, S = ids.shape
        cfg = self.config
        if S < 1 or S > T5_MAX_S:
            raise ValueError(f"NativeT5Encoder: sequence length {S} is outside 1..{T5_MAX_S}")
        lo, hi = int(ids.min()), int(ids.max())       # one range check per call; the kernel clamps regardless
        if lo < 0 or hi >= cfg.vocab_size:
            raise IndexError(f"NativeT5Encoder: input id {lo if lo < 0 else hi} is outside the vocabulary [0, {cfg.vocab_size})")
        last = torch.empty(B, S, cfg.d_model, device=ids.device, dtype=torch.float16)
        _native.check(_native.load().univst_t5_encode(self._h, _native.ptr(ids), B, S, _native.ptr(last), _native.stream_ptr()), "t5_encode")
        out = T5EncoderOutput(last)
        return out if return_dict else out.to_tuple()

    forward = __call__
