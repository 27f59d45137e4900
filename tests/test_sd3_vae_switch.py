"""CPU: the UNIVST_SD3_VAE switch of the SD3 entry points (univst_amd/src/sd3/_common.py load_sd3_vae / build_pipeline) and the parts of
NativeAutoencoderKL.from_pretrained that run before the library is touched: the config checks.  No GPU, no checkpoint."""
import json
import sys

import pytest
import torch

from univst_amd.src.sd3 import _common
from univst_amd.vae import NativeAutoencoderKL, kl_config_from_dir


def test_unknown_mode_is_an_error(monkeypatch, tmp_path):
    monkeypatch.setenv("UNIVST_SD3_VAE", "fast")
    with pytest.raises(ValueError, match="UNIVST_SD3_VAE='fast': 'stock' or 'native'"):
        _common.load_sd3_vae(str(tmp_path), torch.float16)


def test_native_needs_fp16_and_a_local_directory(monkeypatch, tmp_path):
    monkeypatch.setenv("UNIVST_SD3_VAE", "native")
    with pytest.raises(ValueError, match="fp16 only"):
        _common.load_sd3_vae(str(tmp_path), torch.float32)
    with pytest.raises(FileNotFoundError, match="needs a local directory"):
        _common.load_sd3_vae(str(tmp_path), torch.float16)
    (tmp_path / "vae").mkdir()
    with pytest.raises(FileNotFoundError, match="config.json not found"):
        _common.load_sd3_vae(str(tmp_path), torch.float16)


def test_stock_without_diffusers_names_the_switch(monkeypatch, tmp_path):
    monkeypatch.delenv("UNIVST_SD3_VAE", raising=False)
    monkeypatch.setitem(sys.modules, "diffusers", None)          # `import diffusers` raises ImportError, installed or not
    with pytest.raises(RuntimeError, match="UNIVST_SD3_VAE=native"):
        _common.load_sd3_vae(str(tmp_path), torch.float16)


def test_from_pretrained_refuses_other_classes_and_block_types(tmp_path):
    d = tmp_path / "m" / "vae"
    d.mkdir(parents=True)
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKLTemporalDecoder"}))
    with pytest.raises(ValueError, match="_class_name = AutoencoderKLTemporalDecoder"):
        NativeAutoencoderKL.from_pretrained(str(tmp_path / "m"))
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "down_block_types": ["DownEncoderBlock2D"] * 3 + ["AttnDownEncoderBlock2D"]}))
    with pytest.raises(ValueError, match="down_block_types"):
        NativeAutoencoderKL.from_pretrained(str(tmp_path / "m"))
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "up_block_types": ["UpDecoderBlock2D"] * 3}))
    with pytest.raises(ValueError, match="up_block_types"):
        NativeAutoencoderKL.from_pretrained(str(tmp_path / "m"))
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "mid_block_add_attention": False}))
    with pytest.raises(ValueError, match="mid_block_add_attention"):
        NativeAutoencoderKL.from_pretrained(str(tmp_path / "m"))
    (d / "config.json").write_text(json.dumps({"_class_name": "AutoencoderKL", "_diffusers_version": "0.29.0", "down_block_types": ["DownEncoderBlock2D"] * 4,
                                               "up_block_types": ["UpDecoderBlock2D"] * 4, "latent_channels": 16, "use_quant_conv": False}))
    got_dir, raw = kl_config_from_dir(str(tmp_path / "m"))
    assert got_dir == str(d) and raw["latent_channels"] == 16 and raw["use_quant_conv"] is False and "_class_name" not in raw
    with pytest.raises(FileNotFoundError, match="no diffusion_pytorch_model.safetensors"):
        NativeAutoencoderKL.from_pretrained(str(tmp_path / "m"))


def test_config_keys_reach_the_module_config(monkeypatch, tmp_path):
    """use_quant_conv and the other keys of config.json arrive in .config (the handle itself is replaced: no GPU here)"""
    from safetensors.torch import save_file
    from univst_amd import _native, vae
    d = tmp_path / "m" / "vae"
    d.mkdir(parents=True)
    cfg = {"_class_name": "AutoencoderKL", "in_channels": 3, "out_channels": 3, "latent_channels": 4, "block_out_channels": [32, 64, 64, 64], "layers_per_block": 1,
           "norm_num_groups": 8, "scaling_factor": 0.18215, "shift_factor": None, "use_quant_conv": True, "use_post_quant_conv": True, "force_upcast": False,
           "sample_size": 512}
    (d / "config.json").write_text(json.dumps(cfg))
    save_file({"quant_conv.bias": torch.zeros(8)}, str(d / "diffusion_pytorch_model.safetensors"))
    seen = {}

    class Lib:
        def univst_klvae_create(self, c, h):
            c = c._obj
            seen.update(latent=c.latent_channels, boc=tuple(c.block_out_channels), L=c.layers_per_block, G=c.norm_num_groups, q=c.use_quant_conv,
                        pq=c.use_post_quant_conv, score=c.attn_score_bytes, passes=c.pass_bytes)
            return 0

        def univst_klvae_load_tensor(self, h, k, *a):
            seen.setdefault("keys", []).append(k.decode())
            return 0

        univst_klvae_finalize = univst_klvae_destroy = lambda self, *a: 0

    monkeypatch.setattr(_native, "load", lambda: Lib())
    monkeypatch.setattr(_native, "stream_ptr", lambda: 0)
    monkeypatch.setattr(_native, "ptr", lambda t: 0)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda: type("S", (), {"synchronize": lambda self: None})())
    v = vae.NativeAutoencoderKL.from_pretrained(str(tmp_path / "m"), device="cpu", attn_score_bytes=1 << 20)
    c = v.config
    assert (c.latent_channels, c.block_out_channels, c.layers_per_block, c.norm_num_groups) == (4, (32, 64, 64, 64), 1, 8)
    assert c.use_quant_conv is True and c.use_post_quant_conv is True and c.scaling_factor == 0.18215 and c.shift_factor == 0.0 and c.force_upcast is False
    assert seen == dict(latent=4, boc=(32, 64, 64, 64), L=1, G=8, q=1, pq=1, score=1 << 20, passes=0, keys=["quant_conv.bias"])
    assert next(v.parameters()).dtype == torch.float16
    with pytest.raises(RuntimeError, match="GPU only"):
        v.decode(torch.zeros(1, 4, 8, 8))
    # the SD3 defaults
    from univst_amd.vae import KL_DEFAULT_CONFIG as D
    assert (D["latent_channels"], D["block_out_channels"], D["scaling_factor"], D["shift_factor"], D["use_quant_conv"], D["use_post_quant_conv"]) == \
        (16, (128, 256, 512, 512), 1.5305, 0.0609, False, False)


def test_build_pipeline_with_native_switches_does_not_import_diffusers(monkeypatch, tmp_path):
    """UNIVST_SD3_VAE=native: build_pipeline reaches the VAE loader and builds the pipeline object without importing diffusers (every loader is a sentinel)"""
    transformers = pytest.importorskip("transformers")
    monkeypatch.setenv("UNIVST_SD3_VAE", "native")
    had = "diffusers" in sys.modules
    (tmp_path / "vae").mkdir()
    calls = []

    class Sentinel:
        def __init__(self, name):
            self.name = name

        def to(self, *a, **k):
            return self

        cuda = requires_grad_ = to
        attn_processors = {}

        def set_attn_processor(self, p):
            pass

    from univst_amd import vae, schedulers
    from univst_amd.src.sd import _common as sd_common
    monkeypatch.setattr(vae.NativeAutoencoderKL, "from_pretrained", classmethod(lambda cls, path, subfolder="vae", **kw: calls.append((path, subfolder)) or Sentinel("vae")))
    monkeypatch.setattr(_common, "load_transformer", lambda *a: Sentinel("transformer"))
    monkeypatch.setattr(_common, "load_t5_encoder", lambda *a: Sentinel("t5"))
    monkeypatch.setattr(sd_common, "load_text_encoder", lambda *a, **k: Sentinel("clip"))
    for cls in (transformers.CLIPTokenizer, transformers.T5TokenizerFast):
        monkeypatch.setattr(cls, "from_pretrained", classmethod(lambda c, *a, **k: Sentinel("tok")))
    monkeypatch.setattr(schedulers.FlowMatchEulerDiscreteScheduler, "from_pretrained", classmethod(lambda c, *a, **k: Sentinel("sched")))
    pipe = _common.build_pipeline(str(tmp_path), torch.float16)
    assert calls == [(str(tmp_path), "vae")] and pipe.vae.name == "vae" and pipe.text_encoder_3.name == "t5"
    assert ("diffusers" in sys.modules) == had, "build_pipeline imported diffusers with UNIVST_SD3_VAE=native"
    if not had:
        assert pipe.scheduler.name == "sched"
