"""GPU: the AnimateDiff backbone end to end on the native UNet3D — ``AnimationPipeline`` (univst_amd/backbones/animatediff/pipelines/
pipeline_animation.py) over ``engine.transfer_loop`` with this backbone's rules, the inversion tools with the feature tap, ``reconstruction``, and
the C entry ``univst_unet_forward_tap`` — against golden g22: the reference's OWN pipeline, inversion and UNet code run in float64
(tests/golden/make_golden_animatediff_pipeline.py, figures in tests/golden/REPORT_animatediff_pipeline.txt).

The golden's configuration is the widths of tests/test_gpu_animatediff.py's TINY (160 / 160 / 320 / 320, 4 heads: head dims 40 and 80, the smallest
the frame-axis attention has), weights ``animatediff_ref.random_state_dict(cfg, seed=21)``; tests/animatediff_ref.py's G21_CFG has head dims 16 / 32,
for which no native handle can be built.

Bars: the project's 40 dB PSNR on every latent of a 50-step loop (peak = range of the golden), as tests/test_gpu_unet.py's
test_transfer_loop_vs_reference_golden; relative RMS < 1e-2 on dumped features (golden G12's rule; the restatement has no feature output to take
a 2 x e_ref yardstick from); 60 dB / 1e-2 of the output scale between the full run and ``skip_dead_branches``, as the SD test."""
import ctypes as C
import math
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import animatediff_ref as R  # noqa: E402
from oracle import pipeline_ref, unet_ref, synth_inputs as si  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEEP_T = (0, 24, 25, 39, 40, 41, 45, 46, 49)
KEEP_K = (1, 3, 4, 12, 13, 14, 50)
KEEP_R = (0, 10, 25, 49)
_CACHE = {}


def gold(name=""):
    key = "g22" + name
    if key not in _CACHE:
        _CACHE[key] = torch.load(os.path.join(GOLD, f"g22_animatediff_pipeline{name}.pt"))
    return _CACHE[key]


def cfg():
    return gold()["cfg"]


def weights():
    if "sd" not in _CACHE:
        _CACHE["sd"] = R.random_state_dict(cfg(), seed=gold()["seed"])
    return _CACHE["sd"]


def mirror():
    if "unet" not in _CACHE:
        from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
        m = UNet3DConditionModel(**R.reference_kwargs(cfg()))
        m.load_state_dict(weights(), strict=True)
        _CACHE["unet"] = m.half().cuda().eval()
    return _CACHE["unet"]


def unregister(m):
    from univst_amd.backbones.animatediff.pnp_utils import PNP_LAYERS
    for r, bs in PNP_LAYERS.items():
        for b in bs:
            m.up_blocks[r].attentions[b].transformer_blocks[0].attn1.__dict__.pop("_univst_native_pnp", None)


class Tok:
    model_max_length = 77

    def __call__(self, prompt, **kw):
        n = len(prompt) if isinstance(prompt, list) else 1
        return types.SimpleNamespace(input_ids=torch.zeros(n, 77, dtype=torch.long), attention_mask=None)


class Enc(torch.nn.Module):
    config = types.SimpleNamespace()

    def forward(self, ids, attention_mask=None):
        return (si.text_embedding(cfg()["cross_attention_dim"]).half().cuda().expand(ids.shape[0], -1, -1),)


def pipeline():
    """the objects of src/animatediff/_common.build_pipeline with stand-ins for CLIP and no VAE: the pipeline's scheduler has the four yaml keys and
    set_alpha_to_one=True"""
    from univst_amd.backbones.animatediff.pipelines.pipeline_animation import AnimationPipeline
    from univst_amd.schedulers import DDIMScheduler
    from univst_amd.src.animatediff._common import NOISE_SCHEDULER_KWARGS
    m = mirror()
    unregister(m)
    return AnimationPipeline(vae=None, text_encoder=Enc(), tokenizer=Tok(), unet=m, scheduler=DDIMScheduler(set_alpha_to_one=True, **NOISE_SCHEDULER_KWARGS))


def psnr(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    mse = (got - ref).pow(2).mean().item()
    peak = (ref.max() - ref.min()).item()
    return float("inf") if mse == 0 else 10 * math.log10(peak * peak / mse)


def rel_rms(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    return ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("tag", ["nomask", "mask"])
def test_transfer_loop_vs_reference_golden(tag):
    """the reference's own 50-step three-branch AnimationPipeline.video_style_transfer (F = 16, linear betas, final alpha 1) vs the mirror: PSNR >= 40 dB
    after steps 0, 24, 25 (the PnP window is exclusive at the top), 39, 40, 41 (latent AdaIN from step 40 ON: inclusive), 45, 46 (masking ends), 49"""
    from univst_amd.backbones.animatediff import pnp_utils
    pipe = pipeline()
    F_, h, w = 16, 16, 16
    ci = [si.content_latent(k, F_, h, w) for k in range(51)]
    sy = [si.style_latent(k, F_, h, w) for k in range(51)]
    masks = torch.from_numpy(pipeline_ref.mask_from_png_values(si.disc_masks(F_, h * 8, w * 8)))[None] if tag == "mask" else None
    lat0 = ci[50].half().cuda()          # run_video_style_transfer_animatediff.py starts from the content inversion's last latent as it is
    pnp_utils.register_spatial_attention_pnp(pipe)
    got = {}
    try:
        out = pipe.video_style_transfer("", latents=lat0, num_inference_steps=50, content_inv_latents=ci, style_inv_latents=sy, masks=masks,
                                        output_type="latent", callback=lambda i, t, l: got.__setitem__(i, l.clone()) if i in KEEP_T else None).images
        out2 = pipe.video_style_transfer("", latents=lat0, num_inference_steps=50, content_inv_latents=ci, style_inv_latents=sy, masks=masks,
                                         output_type="latent", skip_dead_branches=True).images
    finally:
        unregister(pipe.unet)
    g = gold(f"_transfer_{tag}")
    ps = {i: psnr(got[i], g[f"i{i}"]) for i in KEEP_T}
    peaks = {i: g[f"i{i}"].float().abs().max().item() for i in KEEP_T}
    print(f"transfer {tag}: PSNR per step {', '.join(f'{i}: {p:.1f}' for i, p in ps.items())}; max|golden| {', '.join(f'{i}: {p:.1f}' for i, p in peaks.items())}")
    assert all(torch.isfinite(got[i].float()).all() for i in KEEP_T)
    for i in KEEP_T:
        assert ps[i] >= 40.0, (i, ps[i])
    assert torch.equal(out, got[49])
    # dead-branch skipping (from step 25 on: the window is exclusive at the top) must not change the result
    p2, d2 = psnr(out2, out), (out.float() - out2.float()).abs().max().item() / out.float().abs().max().item()
    print(f"transfer {tag}: skip_dead_branches vs full: {p2:.1f} dB, max diff {d2:.2e} of the output scale")
    assert p2 >= 60.0 and d2 <= 1e-2


@pytest.mark.parametrize("tag,easy", [("ddim_loop", False), ("ddim_loop_plus", True)])
def test_inversion_vs_reference_golden(tmp_path, tag, easy):
    """the reference's own ddim_loop / ddim_loop_plus on its AnimateDiff UNet (F = 4, 50 steps, the SD-v1.5 scaled_linear inversion scheduler, feature
    file of up_blocks[2] at t = 301) vs the native ddim_inversion entry point with the same arguments"""
    from univst_amd.inversion_tools import ddim_inversion as inv
    from univst_amd.schedulers import DDIMScheduler
    g = gold(f"_inversion_{tag}")
    pipe = pipeline()
    z0 = 0.7 * si.content_latent(0, 4, 16, 16)
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    traj = inv.ddim_inversion(pipe, sched, z0.half().cuda(), 50, "", str(tmp_path), ft_indices=[2], ft_timesteps=[301], ft_path=str(tmp_path), is_opt=easy)
    assert len(traj) == 51
    ps = {k: psnr(traj[k], g[f"k{k}"]) for k in KEEP_K}
    print(f"{tag}: PSNR per k {', '.join(f'{k}: {p:.1f}' for k, p in ps.items())}")
    for k in KEEP_K:
        assert torch.isfinite(traj[k].float()).all() and ps[k] >= 40.0, (k, ps[k])
    for k in range(51):
        assert torch.equal(torch.load(tmp_path / f"ddim_latents_{k}.pt"), traj[k]), k
    assert sorted(p.name for p in tmp_path.glob("inversion_feature_map_*")) == ["inversion_feature_map_2_block_301_step.pt"], "one hit: t = 301 only"
    feat = torch.load(tmp_path / "inversion_feature_map_2_block_301_step.pt")
    assert tuple(feat.shape) == tuple(g["feat"].shape) == (4, 16, 16, cfg()["block_out_channels"][1]) and feat.dtype == torch.float16
    assert torch.equal(feat, pipe.unet.last_feature_map)
    rms = rel_rms(feat, g["feat"])
    print(f"{tag}: feature file relative RMS {rms:.2e}")
    assert rms < 1e-2


@pytest.mark.parametrize("tag,gs", [("gs1", 1.0), ("gs7p5", 7.5)])
def test_reconstruction_vs_reference_golden(tag, gs):
    g = gold()[f"reconstruction_{tag}"]
    pipe = pipeline()
    zT = si.content_latent(50, 16, 16, 16)
    got = {}
    out = pipe.reconstruction("", video_length=16, height=128, width=128, latents=zT.half().cuda(), guidance_scale=gs, output_type="latent",
                              callback=lambda i, t, l: got.__setitem__(i, l.clone()) if i in KEEP_R else None).images
    ps = {i: psnr(got[i], g[f"i{i}"]) for i in KEEP_R}
    print(f"reconstruction {tag}: PSNR per step {', '.join(f'{i}: {p:.1f}' for i, p in ps.items())}")
    for i in KEEP_R:
        assert torch.isfinite(got[i].float()).all() and ps[i] >= 40.0, (i, ps[i])
    assert torch.equal(out, got[49])


# ---------------------------------------------------------------------- the C entry
def raw_handle():
    """the C ABI without the mirror (as tests/test_gpu_animatediff.py's): the same tensors under the same names"""
    from univst_amd import _native
    c, lib = cfg(), _native.load()
    hd = c["attention_head_dim"]
    uc = _native.UnetCfg(4, 4, (C.c_int * 4)(*c["block_out_channels"]), c["layers_per_block"], c["cross_attention_dim"],
                         (C.c_int * 4)(*((hd,) * 4 if isinstance(hd, int) else hd)), c["norm_num_groups"], c["norm_eps"], 1, 0.0)
    mask = sum(1 << i for i in range(4) if c["motion_levels"][i])
    ad = _native.AnimateDiffCfg(int(c["use_inflated_groupnorm"]), mask, int(c["motion_mid_block"]),
                                _native.MotionCfg(0, c["motion_heads"], c["motion_blocks"], c["motion_attn"], 32, c["max_len"], 1, 1e-6, 1e-5))
    h = C.c_void_p()
    _native.check(lib.univst_unet_create_animatediff(C.byref(uc), C.byref(ad), C.byref(h)), "create")
    for k, v in weights().items():
        t = v.cuda().contiguous()
        _native.check(lib.univst_unet_load_tensor(h, k.encode(), t.data_ptr(), 1, (C.c_int64 * t.dim())(*t.shape), t.dim(), _native.stream_ptr()), k)
        torch.cuda.synchronize()
    _native.check(lib.univst_unet_finalize(h, _native.stream_ptr()), "finalize")
    return h


def test_tap_entry_on_a_raw_handle():
    """univst_unet_forward_tap on an AnimateDiff handle, B = 3, F = 2: eps is bit-equal to univst_unet_forward's, the features of every block are the
    reference's dump of branch 0, the refusals come before any launch, and the old entry still refuses a feat_out on this kind of handle"""
    from univst_amd import _native
    lib, g = _native.load(), gold("_tap")
    x, txt, t = g["sample"].cuda().contiguous(), g["text"].cuda().contiguous(), float(g["timestep"])
    B, _, F_, H, W = x.shape
    h = raw_handle()
    try:
        eps0 = torch.empty_like(x)
        args = lambda e: (h, x.data_ptr(), t, txt.data_ptr(), B, F_, H, W, txt.shape[1], None, e.data_ptr())      # noqa: E731
        _native.check(lib.univst_unet_forward(*args(eps0), None, -1, _native.stream_ptr()), "forward")
        assert torch.isfinite(eps0.float()).all() and psnr(eps0, g["eps"]) >= 40.0
        for idx in range(4):
            want = g[f"feat{idx}"]
            feat, eps = torch.zeros(want.shape, device="cuda", dtype=torch.float16), torch.zeros_like(x)
            _native.check(lib.univst_unet_forward_tap(*args(eps), feat.data_ptr(), idx, _native.stream_ptr()), f"forward_tap {idx}")
            rms = rel_rms(feat, want)
            print(f"tap ft_index {idx}: shape {tuple(feat.shape)}, relative RMS {rms:.2e}, max|want| {want.float().abs().max().item():.1f}")
            assert torch.equal(eps, eps0), idx
            assert torch.isfinite(feat.float()).all() and rms < 1e-2, (idx, rms)
        keep = torch.full_like(x, 7.0)
        feat = torch.zeros(g["feat3"].shape, device="cuda", dtype=torch.float16)
        for bad, word in ((4, "ft_index"), (-1, "ft_index")):
            assert lib.univst_unet_forward_tap(*args(keep), feat.data_ptr(), bad, _native.stream_ptr()) == -1 and word in lib.univst_last_error().decode()
        assert lib.univst_unet_forward_tap(*args(keep), None, 2, _native.stream_ptr()) == -1 and "feat_out" in lib.univst_last_error().decode()
        assert lib.univst_unet_forward(*args(keep), feat.data_ptr(), 2, _native.stream_ptr()) == -1 and "feat_out" in lib.univst_last_error().decode()
        torch.cuda.synchronize()
        assert (keep == 7.0).all() and (feat == 0).all(), "a refusal comes before any launch"
    finally:
        lib.univst_unet_destroy(h)


def test_tap_entry_equals_the_old_entry_on_an_sd_handle():
    """an SD-kind handle takes the tap through both entries: the same features and the same eps, bit for bit"""
    from univst_amd import _native
    from univst_amd.backbones.video_diffusion_sd.models.unet_3d_condition import UNetPseudo3DConditionModel
    lib, c = _native.load(), unet_ref.TINY_CONFIG
    unet = UNetPseudo3DConditionModel(block_out_channels=c["block_out_channels"], cross_attention_dim=c["cross_attention_dim"],
                                      attention_head_dim=c["attention_head_dim"], norm_num_groups=c["norm_num_groups"])
    unet.load_state_dict(unet_ref.synth_state_dict(c, seed=33, trivial_temporal=True))
    unet = unet.half().cuda()
    unet._sync_native()
    x = si.content_latent(50, 4, 16, 16).half().cuda()
    txt = si.text_embedding(c["cross_attention_dim"]).half().cuda().contiguous()
    boc = list(reversed(c["block_out_channels"]))
    for idx in range(4):
        lvl = min(idx + 1, 3)
        out = []
        for fn in (lib.univst_unet_forward, lib.univst_unet_forward_tap):
            eps, feat = torch.zeros_like(x), torch.zeros(4, 2 << lvl, 2 << lvl, boc[idx], device="cuda", dtype=torch.float16)
            _native.check(fn(unet._native_handle, x.data_ptr(), 301.0, txt.data_ptr(), 1, 4, 16, 16, 77, None, eps.data_ptr(), feat.data_ptr(), idx,
                             _native.stream_ptr()), f"sd handle, ft_index {idx}")
            out.append((eps, feat))
        assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), idx
        assert out[0][1].float().abs().max() > 0 and torch.isfinite(out[0][1].float()).all()


# ---------------------------------------------------------------------- one chain through files
def test_end_to_end_chain_through_files(tmp_path):
    """scripts/start_animatediff.sh with tiny models and the on-disk bus between the stages: content inversion (Easy-Inv, the feature tap at t = 301) ->
    mask propagation on the dumped feature FILE (--backbone animatediff) -> style inversion -> localized three-branch transfer from the three folders.
    The result is finite and equals the in-memory call on the same tensors bit for bit."""
    from PIL import Image
    from univst_amd.backbones.animatediff import pnp_utils
    from univst_amd.inversion_tools import ddim_inversion as inv
    from univst_amd.src import mask_propagation as mp
    from univst_amd.src.util import load_ddim_latents_at_t, load_mask
    from univst_amd.schedulers import DDIMScheduler
    pipe = pipeline()
    F_, h, w = 16, 16, 16
    cdir, sdir, fdir, mdir = (tmp_path / n for n in ("c", "s", "f", "m"))
    for d in (cdir, sdir, fdir):
        d.mkdir()
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    inv.ddim_inversion(pipe, sched, (0.8 * si.content_latent(0, F_, h, w)).half().cuda(), 50, "", str(cdir), ft_indices=[2], ft_timesteps=[301],
                       ft_path=str(fdir), is_opt=True)
    feat_file = fdir / "inversion_feature_map_2_block_301_step.pt"
    feats = torch.load(feat_file)
    assert tuple(feats.shape) == (F_, h, w, cfg()["block_out_channels"][1]) and feats.dtype == torch.float16 and torch.isfinite(feats.float()).all()
    Image.fromarray(si.soft_first_mask()).save(tmp_path / "first.png")
    args = mp.build_parser().parse_args(["--feature_path", str(feat_file), "--mask_path", str(tmp_path / "first.png"), "--backbone", "animatediff",
                                         "--output_path", str(mdir)])
    torch.manual_seed(33)
    masks = mp.video_mask_propogation(args)
    mask_dir = mdir / "animatediff" / "first"
    m01 = load_mask(str(mask_dir), n_frames=F_)
    assert len(masks) == F_ and m01.shape == (1, F_, 128, 128) and set(m01.unique().tolist()) <= {0, 1} and 0 < m01.float().mean() < 1
    inv.ddim_inversion(pipe, sched, (0.8 * si.style_latent(0, F_, h, w)).half().cuda(), 50, "", str(sdir), is_opt=False)
    assert all((cdir / f"ddim_latents_{k}.pt").exists() and (sdir / f"ddim_latents_{k}.pt").exists() for k in range(51))
    lat0 = load_ddim_latents_at_t(50, str(cdir)).cuda()
    pnp_utils.register_spatial_attention_pnp(pipe)
    try:
        out = pipe.video_style_transfer("", latents=lat0, num_inference_steps=50, content_inv_path=str(cdir), style_inv_path=str(sdir),
                                        mask_path=str(mask_dir), output_type="latent").images
        ci = [load_ddim_latents_at_t(k, str(cdir)) for k in range(51)]
        sy = [load_ddim_latents_at_t(k, str(sdir)) for k in range(51)]
        mem = pipe.video_style_transfer("", latents=lat0, num_inference_steps=50, content_inv_latents=ci, style_inv_latents=sy, masks=m01,
                                        output_type="latent").images
    finally:
        unregister(pipe.unet)
    assert out.shape == (1, 4, F_, h, w) and out.dtype == torch.float16 and torch.isfinite(out.float()).all()
    assert torch.equal(out, mem)
    assert not np.array_equal(out.float().cpu().numpy(), lat0.float().cpu().numpy())
