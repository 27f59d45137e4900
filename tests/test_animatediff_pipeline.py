"""CPU: what the AnimateDiff pipeline adds around the native UNet3D — the drop-in import paths, the three CLIs' flags, the linear-beta DDIM
tables, ``load_weights``' filter and refusals, the pipeline's input checks, the keyword-only parameters of ``engine.transfer_loop`` — and the
restatement tests/animatediff_ref.py against the reference's own B = 3 forward of golden g22 (tests/golden/make_golden_animatediff_pipeline.py).
Nothing here touches the GPU; the loops themselves are tests/test_gpu_animatediff_pipeline.py's."""
import inspect
import os
import subprocess
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SURFACE = {
    "backbones.animatediff.pipelines.pipeline_animation": ("univst_amd.backbones.animatediff.pipelines.pipeline_animation",
                                                           ["AnimationPipeline", "AnimationPipelineOutput", "register_time", "latent_adain"]),
    "backbones.animatediff.utils.util": ("univst_amd.backbones.animatediff.utils.util", ["load_weights", "save_videos_grid"]),
}


@pytest.mark.parametrize("ref_path", sorted(SURFACE))
def test_reference_import_paths_resolve_to_the_native_package(ref_path):
    import importlib
    prod_path, names = SURFACE[ref_path]
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    shim, prod = importlib.import_module(ref_path), importlib.import_module(prod_path)
    assert os.path.abspath(shim.__file__).startswith(ROOT), f"{ref_path} resolved outside this repository: {shim.__file__}"
    for n in names:
        assert getattr(shim, n) is getattr(prod, n), f"{ref_path}.{n} is not the native implementation's"
    from univst_amd.src import util
    if ref_path.endswith("utils.util"):
        assert shim.save_videos_grid is util.save_videos_grid


def test_the_rest_of_the_utils_and_pipelines_packages_resolves_to_the_checkout_behind(tmp_path):
    """the shim packages extend their __path__: with a checkout behind this repository on the path, backbones.animatediff.utils.convert_from_ckpt
    (which this repository does not carry) is the checkout's, while util stays this repository's, and so does pipeline_animation unless the checkout has one"""
    d = tmp_path / "backbones" / "animatediff" / "utils"
    d.mkdir(parents=True)
    (d / "convert_from_ckpt.py").write_text("WHO = 'checkout'\n")
    (d / "util.py").write_text("WHO = 'checkout'\n")
    code = ("import backbones.animatediff.utils.convert_from_ckpt as c, backbones.animatediff.utils.util as u, "
            "backbones.animatediff.pipelines.pipeline_animation as p; print(c.WHO, c.__file__); print(u.__file__); print(p.__file__)")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path),
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + str(tmp_path)), timeout=120)
    assert out.returncode == 0, out.stderr[-600:]
    c, u, p = out.stdout.strip().splitlines()
    assert c.startswith("checkout ") and c.split(" ", 1)[1].startswith(str(tmp_path))
    assert u.startswith(ROOT) and p.startswith(ROOT)
    # a checkout that has its own pipelines/pipeline_animation.py keeps it (tests/test_motion_abi.py pins that since before this repository had one)
    (tmp_path / "backbones" / "animatediff" / "pipelines").mkdir()
    (tmp_path / "backbones" / "animatediff" / "pipelines" / "pipeline_animation.py").write_text("WHO = 'checkout'\n")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path),
                         env=dict(os.environ, PYTHONPATH=ROOT + os.pathsep + str(tmp_path)), timeout=120)
    assert out.returncode == 0, out.stderr[-600:]
    c, u, p = out.stdout.strip().splitlines()
    assert u.startswith(ROOT) and p.startswith(str(tmp_path))


FLAGS = {"run_content_inversion_animatediff": ["--pretrained_model_path", "--motion_module_path", "--content_path", "--output_path", "--weight_dtype",
                                               "--num_frames", "--height", "--width", "--time_steps", "--ft_indices", "--ft_timesteps", "--is_opt", "--seed"],
         "run_style_inversion_animatediff": ["--pretrained_model_path", "--motion_module_path", "--style_path", "--output_path", "--weight_dtype",
                                             "--num_frames", "--height", "--width", "--time_steps", "--is_opt", "--seed"],
         "run_video_style_transfer_animatediff": ["--pretrained_model_path", "--motion_module_path", "--content_inv_path", "--style_inv_path", "--mask_path",
                                                  "--output_path", "--weight_dtype", "--time_steps", "--seed"]}


@pytest.mark.parametrize("script", sorted(FLAGS))
def test_cli_scripts_keep_the_reference_flags(script):
    """src/animatediff/run_*_animatediff.py --help works without a GPU and lists the reference's flags (their argparse blocks) and defaults"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "src", "animatediff", script + ".py"), "--help"], capture_output=True, text=True, cwd=ROOT,
                         env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    assert out.returncode == 0, out.stderr[-400:]
    for flag in FLAGS[script]:
        assert flag in out.stdout, f"{script}: flag {flag} missing from --help"
    import importlib
    a = importlib.import_module(f"univst_amd.src.animatediff.{script}").parser().parse_args([])
    assert a.motion_module_path == "ckpts/mm_sd_v15_v2.ckpt" and a.time_steps == 50 and a.seed == 33 and a.weight_dtype == torch.float16
    assert "/animatediff/" in getattr(a, "content_inv_path", "x/animatediff/") and a.output_path.startswith("results/")
    if script == "run_content_inversion_animatediff":
        assert (a.ft_indices, a.ft_timesteps, a.num_frames, a.is_opt) == (2, 301, 16, False)


def test_inference_config_constants_and_the_yaml_in_the_working_directory(tmp_path, monkeypatch):
    from univst_amd.src.animatediff import _common
    monkeypatch.chdir(tmp_path)
    unet_kw, sched_kw = _common.inference_config()
    assert sched_kw == {"beta_start": 0.00085, "beta_end": 0.012, "beta_schedule": "linear", "steps_offset": 1, "clip_sample": False}
    assert unet_kw["use_inflated_groupnorm"] and unet_kw["use_motion_module"] and unet_kw["motion_module_mid_block"] and unet_kw["motion_module_type"] == "Vanilla"
    assert list(unet_kw["motion_module_resolutions"]) == [1, 2, 4, 8] and unet_kw["motion_module_kwargs"]["num_attention_heads"] == 8
    unet_kw["motion_module_kwargs"]["num_attention_heads"] = 1
    assert _common.UNET_ADDITIONAL_KWARGS["motion_module_kwargs"]["num_attention_heads"] == 8, "callers get copies"
    (tmp_path / "backbones" / "animatediff").mkdir(parents=True)
    (tmp_path / "backbones" / "animatediff" / "animatediff-v2.yaml").write_text(
        "unet_additional_kwargs:\n  use_motion_module: false\nnoise_scheduler_kwargs:\n  beta_start: 0.001\n  beta_schedule: \"linear\"\n")
    assert _common.inference_config() == ({"use_motion_module": False}, {"beta_start": 0.001, "beta_schedule": "linear"})


# ---------------------------------------------------------------------- scheduler
def test_linear_beta_table_and_final_alpha():
    from univst_amd.schedulers import DDIMScheduler
    s = DDIMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="linear", steps_offset=1, clip_sample=False, set_alpha_to_one=True)
    k = torch.arange(1000, dtype=torch.float64)
    betas = 0.00085 + (0.012 - 0.00085) * k / 999
    assert s.betas.dtype == torch.float32 and (s.betas.double() - betas).abs().max() < 1e-9
    assert (s.alphas_cumprod.double() - torch.cumprod(1 - betas, 0)).abs().max() < 1e-5
    assert float(s.final_alpha_cumprod) == 1.0 and s.config.beta_schedule == "linear" and s.config.set_alpha_to_one is True
    s.set_timesteps(50)
    assert s.timesteps.tolist() == [20 * i + 1 for i in reversed(range(50))]
    x, e = torch.randn(2, 3, dtype=torch.float64), torch.randn(2, 3, dtype=torch.float64)
    out = s.step(e, 1, x)         # the last step: prev_t < 0, final alpha 1 -> the step returns x0
    assert torch.allclose(out.prev_sample, out.pred_original_sample)
    assert float(DDIMScheduler(beta_schedule="linear").final_alpha_cumprod) != 1.0, "set_alpha_to_one stays False by default"


def test_default_scheduler_is_unchanged():
    from univst_amd.schedulers import DDIMScheduler
    s = DDIMScheduler()
    want = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2
    assert torch.equal(s.betas, want) and s.config.beta_schedule == "scaled_linear" and s.config.set_alpha_to_one is False
    assert torch.equal(s.final_alpha_cumprod, s.alphas_cumprod[0])
    for bad in (dict(beta_schedule="squaredcos_cap_v2"), dict(prediction_type="v_prediction"), dict(timestep_spacing="trailing"), dict(clip_sample=True)):
        with pytest.raises(NotImplementedError):
            DDIMScheduler(**bad)


def test_transfer_loop_keeps_its_defaults():
    from univst_amd import engine
    p = inspect.signature(engine.transfer_loop).parameters
    for name, default in (("adain_from_inclusive", False), ("register_time_fn", None), ("pnp_window_closed", None)):
        assert p[name].kind is inspect.Parameter.KEYWORD_ONLY and p[name].default is default
    from univst_amd.backbones.animatediff.pipelines import pipeline_animation as pa
    assert [pa._window_closed(i, 0.5) for i in (24, 25, 26)] == [False, True, True]


# ---------------------------------------------------------------------- load_weights
class _UNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.motion_modules = torch.nn.ModuleList([torch.nn.Linear(2, 2, bias=False)])
        self.conv = torch.nn.Linear(2, 2, bias=False)


def test_load_weights_filter(tmp_path):
    from univst_amd.backbones.animatediff.utils.util import load_weights
    sig = inspect.signature(load_weights)
    assert list(sig.parameters) == ["animation_pipeline", "motion_module_path", "motion_module_lora_configs", "adapter_lora_path", "adapter_lora_scale",
                                    "dreambooth_model_path", "lora_model_path", "lora_alpha", "device", "dtype"]
    pipe = types.SimpleNamespace(unet=_UNet())
    conv = pipe.unet.conv.weight.detach().clone()
    sd = {"motion_modules.0.weight": torch.full((2, 2), 3.0), "motion_modules.0.pos_encoder.pe": torch.zeros(1, 24, 2),
          "conv.weight": torch.full((2, 2), 5.0), "animatediff_config": torch.zeros(1)}
    for wrapped, path in ((True, tmp_path / "a.ckpt"), (False, tmp_path / "b.ckpt")):
        torch.save({"state_dict": sd} if wrapped else sd, path)
        pipe.unet.motion_modules[0].weight.data.zero_()
        assert load_weights(pipe, motion_module_path=str(path)) is pipe
        assert (pipe.unet.motion_modules[0].weight == 3.0).all() and torch.equal(pipe.unet.conv.weight, conv), "only motion_modules. names are loaded"
    torch.save({"motion_modules.7.weight": torch.zeros(2, 2)}, tmp_path / "c.ckpt")
    with pytest.raises(AssertionError):
        load_weights(pipe, motion_module_path=str(tmp_path / "c.ckpt"))
    assert load_weights(pipe) is pipe          # no path: nothing loaded, as the reference


def test_load_weights_refusals_and_no_download(tmp_path, monkeypatch):
    from univst_amd.backbones.animatediff.utils.util import load_weights
    pipe = types.SimpleNamespace(unet=_UNet())
    for kw, names in ((dict(dreambooth_model_path="x.safetensors"), "convert_from_ckpt"), (dict(lora_model_path="x.safetensors"), "convert_lora"),
                      (dict(adapter_lora_path="x.ckpt"), "load_diffusers_lora"), (dict(motion_module_lora_configs=[{"path": "x", "alpha": 1.0}]), "load_diffusers_lora")):
        with pytest.raises(NotImplementedError, match=names):
            load_weights(pipe, **kw)
    monkeypatch.setitem(sys.modules, "huggingface_hub", None)          # any attempt to import the hub client would raise ImportError instead
    missing = tmp_path / "ckpts" / "mm_sd_v15_v2.ckpt"
    with pytest.raises(FileNotFoundError, match="mm_sd_v15_v2.ckpt"):
        load_weights(pipe, motion_module_path=str(missing))
    assert not missing.parent.exists(), "nothing is created or fetched for a missing file"


# ---------------------------------------------------------------------- pipeline
def _pipe(**kw):
    from univst_amd.backbones.animatediff.pipelines.pipeline_animation import AnimationPipeline
    from univst_amd.schedulers import DDIMScheduler
    vae = types.SimpleNamespace(config=types.SimpleNamespace(block_out_channels=(1, 2, 3, 4), scaling_factor=0.18215))
    return AnimationPipeline(vae=vae, text_encoder=None, tokenizer=None, unet=types.SimpleNamespace(device=torch.device("cpu")),
                             scheduler=DDIMScheduler(beta_schedule="linear", set_alpha_to_one=True), **kw)


def test_pipeline_input_checks_have_the_reference_messages():
    pipe = _pipe()
    assert pipe.vae_scale_factor == 8 and pipe.controlnet is None
    with pytest.raises(ValueError, match="`prompt` has to be of type `str` or `list` but is <class 'int'>"):
        pipe.check_inputs(3, 64, 64, 1)
    with pytest.raises(ValueError, match="`height` and `width` have to be divisible by 8 but are 60 and 64."):
        pipe.check_inputs("", 60, 64, 1)
    with pytest.raises(ValueError, match="`callback_steps` has to be a positive integer but is 0 of type <class 'int'>."):
        pipe.check_inputs("", 64, 64, 0)
    pipe.check_inputs([""], 64, 64, 1)
    with pytest.raises(ValueError, match=r"Unexpected latents shape, got torch.Size\(\[1, 4, 3, 8, 8\]\), expected \(1, 4, 2, 8, 8\)"):
        pipe.prepare_latents(1, 4, 2, 64, 64, torch.float32, torch.device("cpu"), None, torch.zeros(1, 4, 3, 8, 8))
    with pytest.raises(ValueError, match="You have passed a list of generators of length 1, but requested an effective batch size of 2"):
        pipe.prepare_latents(2, 4, 2, 64, 64, torch.float32, torch.device("cpu"), [torch.Generator()])
    z = pipe.prepare_latents(1, 4, 2, 64, 64, torch.float32, torch.device("cpu"), torch.Generator().manual_seed(1))
    assert z.shape == (1, 4, 2, 8, 8) and torch.equal(z, torch.randn(1, 4, 2, 8, 8, generator=torch.Generator().manual_seed(1)))
    assert pipe.prepare_extra_step_kwargs("g", 0.0) == {"eta": 0.0, "generator": "g"}


def test_pipeline_refuses_what_is_not_built():
    from univst_amd.backbones.animatediff.pipelines.pipeline_animation import AnimationPipeline
    assert list(inspect.signature(AnimationPipeline.__init__).parameters) == ["self", "vae", "text_encoder", "tokenizer", "unet", "scheduler", "controlnet"]
    with pytest.raises(NotImplementedError, match="SparseControlNet"):
        _pipe(controlnet=object())
    pipe = _pipe()
    for kw, what in ((dict(eta=0.5), "eta"), (dict(smoother="pixel"), "smoother"), (dict(shard=object()), "shard")):
        with pytest.raises(NotImplementedError, match=what):
            pipe.video_style_transfer("", latents=torch.zeros(1, 4, 2, 8, 8), **kw)
    with pytest.raises(NotImplementedError, match="eta"):
        pipe.reconstruction("", 2, 64, 64, eta=0.1)


def test_decode_latents_regroups_by_the_clips_own_frame_count():
    pipe = _pipe()
    pipe.vae = torch.nn.Module()
    pipe.vae.p = torch.nn.Parameter(torch.zeros(1))
    pipe.vae.config = types.SimpleNamespace(scaling_factor=0.5)
    pipe.vae.forward = lambda x, num_frames=1: x
    pipe.vae.decode = lambda z, num_frames=1: types.SimpleNamespace(sample=z[:, :3].repeat_interleave(2, -1).repeat_interleave(2, -2))
    z = torch.arange(2 * 4 * 3 * 2 * 2, dtype=torch.float32).view(2, 4, 3, 2, 2) / 100
    out = pipe.decode_latents(z)
    assert out.shape == (2, 3, 4, 4, 3)
    assert torch.allclose(torch.from_numpy(out[1, 2, 0, 0]), (z[1, :3, 2, 0, 0] / 0.5 / 2 + 0.5).clamp(0, 1))


# ---------------------------------------------------------------------- the restatement against the reference's forward of g22
def test_restatement_equals_the_reference_forward_of_g22():
    """one B = 3, F = 2 forward of the golden's configuration (the widths of the GPU tests' TINY): the reference's eps is stored as float16, so the
    fp64 restatement must sit within half an fp16 ulp of it"""
    import animatediff_ref as R
    g = torch.load(os.path.join(ROOT, "tests", "golden", "g22_animatediff_pipeline_tap.pt"))
    cfg = torch.load(os.path.join(ROOT, "tests", "golden", "g22_animatediff_pipeline.pt"))["cfg"]
    with torch.no_grad():
        mine = R.unet_forward(R.random_state_dict(cfg, seed=21), cfg, g["sample"].double(), g["timestep"], g["text"].double(), dtype=torch.float64)
    want = g["eps"].double()
    assert (mine - want).abs().max() <= 2.0 ** -11 * want.abs().max() + 1e-6
    for i, shape in enumerate(((2, 4, 4, 320), (2, 8, 8, 320), (2, 16, 16, 160), (2, 16, 16, 160))):
        assert tuple(g[f"feat{i}"].shape) == shape and g[f"feat{i}"].dtype == torch.float16
