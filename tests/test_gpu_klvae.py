"""GPU parity of the native plain AutoencoderKL (csrc/vae.hip through univst_klvae_* / univst_amd.vae.NativeAutoencoderKL: the SD3 / SD3.5 VAE) against
the fp32 restatement tests/klvae_ref.py run with torch ops on the device on the same fp16-valued random-init weights.

PARITY UNPINNED: the network is diffusers' AutoencoderKL (third-party, absent here); both sides restate its published definition, and
test_native_klvae_against_the_diffusers_class is the test that would pin it where diffusers can be imported.  Bars: the temporal VAE's own
(tests/test_gpu_vae.py) — max error < 2e-2 of the output scale, relative RMS < 5e-3; the plain network is a subset of that one's layers.  Next to every
pair of errors the same two figures of the restatement run in torch fp16 on the device go to parity_klvae.json.  Where that file goes is the caller's choice, $UNIVST_PARITY_DIR (default: parity_out/ in the repository root, kept out
of git): the directory a job runner collects results from belongs to the machine the suite runs on, and this repository's new files name no such
machine or tool.  The figures of the run recorded for this network are kept in profiles/klvae_parity.json."""
import json
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import klvae_ref as R  # noqa: E402

MAX_BAR, RMS_BAR = 2e-2, 5e-3
SMALL = dict(R.SD3_VAE_CONFIG, block_out_channels=(64, 128, 128, 128))
SD3 = dict(R.SD3_VAE_CONFIG)
V15 = dict(SMALL, latent_channels=4, use_quant_conv=True, use_post_quant_conv=True, scaling_factor=0.18215, shift_factor=0.0)      # SD-v1.5's image VAE's shape
BIG_LAT = 128         # the 1024 x 1024 case (test_decode_1024_once)


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def _err(got, ref):
    got, ref = got.float(), ref.float()
    return (got - ref).abs().max().item() / ref.abs().max().item(), ((got - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


def _record(name, **vals):
    out_dir = os.environ.get("UNIVST_PARITY_DIR") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "parity_out")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "parity_klvae.json")
    data = json.load(open(path)) if os.path.exists(path) else {}
    data[name] = vals
    json.dump(data, open(path, "w"), indent=1, sort_keys=True)


def _restated(fn, sd, x, cfg, dtype=torch.float32):
    """the restatement on the device in `dtype` (convolutions as im2col + matmul: torch's fp32 convolution is slow on this ROCm build)"""
    try:
        R.CONV_VIA_MATMUL = True
        with torch.no_grad():
            return fn({k: t.to(dtype) for k, t in sd.items()}, x.to(dtype), cfg)
    finally:
        R.CONV_VIA_MATMUL = False


def _hold(name, got, sd, x, cfg, fn, **extra):
    """print, record and assert the errors of `got` against the fp32 restatement, with the torch-fp16 run's own errors beside them"""
    ref = _restated(fn, sd, x, cfg)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    mx, rms = _err(got, ref)
    hmx, hrms = _err(_restated(fn, sd, x, cfg, torch.float16), ref)
    print(f"{name}: native max {mx:.3e} rms {rms:.3e} | torch fp16 max {hmx:.3e} rms {hrms:.3e}")
    _record(name, native_max=mx, native_rms=rms, torch_fp16_max=hmx, torch_fp16_rms=hrms, **extra)
    assert torch.isfinite(got.float()).all()
    assert mx < MAX_BAR and rms < RMS_BAR, (name, mx, rms)
    return ref


def _z(cfg, n, h, w, seed=1):
    return torch.randn(n, cfg["latent_channels"], h, w, generator=torch.Generator().manual_seed(seed)).half().cuda()


def _img(n, H, W, seed=2):
    return (torch.rand(n, 3, H, W, generator=torch.Generator().manual_seed(seed)) * 2 - 1).half().cuda()


_HANDLES = {}


def _handle(cfg_name, seed=3, **kw):
    """one handle (and state dict) per (config, seed, budgets) for the whole module"""
    from univst_amd import synth, vae
    key = (cfg_name, seed, tuple(sorted(kw.items())))
    if key not in _HANDLES:
        cfg = {"SMALL": SMALL, "SD3": SD3, "V15": V15}[cfg_name]
        sd = synth.klvae_state_dict(cfg, seed=seed)
        _HANDLES[key] = (vae.NativeAutoencoderKL(sd, cfg, **kw), sd, cfg)
    return _HANDLES[key]


CASES = [("SMALL", 3, 8, 8), ("SMALL", 2, 8, 24), ("SD3", 2, 16, 16), ("V15", 2, 8, 8)]


@pytest.mark.parametrize("cfg_name,n,h,w", CASES)
def test_decode_matches_restated_definition(nat, cfg_name, n, h, w):
    v, sd, cfg = _handle(cfg_name)
    z = _z(cfg, n, h, w)
    got = v.decode(z).sample
    assert got.shape == (n, 3, 8 * h, 8 * w) and got.dtype == torch.float16
    _hold(f"decode_{cfg_name}_{n}x{h}x{w}", got, sd, z, cfg, R.decode)
    assert v.query("attn_chunks") == 1 and v.query("passes") == 1
    assert v.query("weight_bytes") > 0 and v.query("arena_bytes") >= v.query("arena_high_water") > 0      # the read-outs every handle answers
    assert v.decode(z, return_dict=False)[0].equal(got)


@pytest.mark.parametrize("cfg_name,n,h,w", CASES)
def test_encode_moments_and_sampling(nat, cfg_name, n, h, w):
    v, sd, cfg = _handle(cfg_name)
    x = _img(n, 8 * h, 8 * w)
    dist = v.encode(x).latent_dist
    assert dist.parameters.shape == (n, 2 * cfg["latent_channels"], h, w)
    _hold(f"encode_{cfg_name}_{n}x{h}x{w}", dist.parameters, sd, x, cfg, R.encode_moments)
    # DiagonalGaussianDistribution.sample(): mean + exp(0.5 * clamp(logvar)) * randn, consuming torch's device RNG once
    torch.manual_seed(11)
    s = dist.sample()
    torch.manual_seed(11)
    noise = torch.randn(dist.mean.shape, device="cuda", dtype=torch.float16)
    assert torch.equal(s, dist.mean + torch.exp(0.5 * dist.logvar.clamp(-30, 20)) * noise)


@pytest.mark.parametrize("h,w,budget,last", [(16, 16, 128 * 256 * 2, 128),       # N = 256: two whole chunks of 128 query rows
                                             (8, 24, 128 * 192 * 2, 64)])         # N = 192: one chunk of 128 rows and a ragged one of 64
def test_chunked_attention(nat, h, w, budget, last):
    v, sd, cfg = _handle("SMALL", attn_score_bytes=budget)
    whole, _, _ = _handle("SMALL")
    assert (h * w - last) % 128 == 0 and budget // (2 * h * w) == 128
    z, x = _z(cfg, 2, h, w), _img(2, 8 * h, 8 * w)
    got = v.decode(z).sample
    assert v.query("attn_chunks") == 2
    d_dec = (got.float() - whole.decode(z).sample.float()).abs().max().item()
    assert whole.query("attn_chunks") == 1
    _hold(f"chunked_decode_{h}x{w}", got, sd, z, cfg, R.decode, max_abs_diff_from_unchunked=d_dec)
    mom = v.encode(x).latent_dist.parameters
    assert v.query("attn_chunks") == 2
    d_enc = (mom.float() - whole.encode(x).latent_dist.parameters.float()).abs().max().item()
    _hold(f"chunked_encode_{h}x{w}", mom, sd, x, cfg, R.encode_moments, max_abs_diff_from_unchunked=d_enc)


def test_encoder_is_the_temporal_vae_encoder_bit_for_bit(nat):
    """the native twin of tests/test_klvae_ref.py::test_encoder_equals_the_temporal_vae_encoder: a NativeTemporalVAE and a NativeAutoencoderKL
    (use_quant_conv) with the same encoder.* and quant_conv.* tensors give the same moments, bit for bit — both handles run one encoder.  SMALL's
    widths, 2 images of 64 x 64 pixels: an 8 x 8 latent, 64 attention tokens, one chunk."""
    from univst_amd import synth, vae
    tcfg = dict(synth.SVD_VAE_CONFIG, block_out_channels=SMALL["block_out_channels"])
    tsd = synth.vae_state_dict(tcfg, seed=13)
    shared = {k: t for k, t in tsd.items() if k.startswith(("encoder.", "quant_conv."))}
    ksd = {**synth.klvae_state_dict(V15, seed=14), **shared}
    assert len(shared) > 0 and all(k in ksd and ksd[k].shape == t.shape for k, t in shared.items())
    assert set(k for k in ksd if k.startswith(("encoder.", "quant_conv."))) == set(shared)
    t, k = vae.NativeTemporalVAE(tsd, tcfg), vae.NativeAutoencoderKL(ksd, V15)
    x = _img(2, 64, 64, seed=8)
    want, got = t.encode(x).latent_dist.parameters, k.encode(x).latent_dist.parameters
    assert k.query("attn_chunks") == 1 and k.query("passes") == 1
    assert got.shape == want.shape == (2, 8, 8, 8) and torch.isfinite(got.float()).all() and got.float().abs().max().item() > 0
    assert torch.equal(got, want)


def test_passes_over_images(nat):
    """3 images under a pass_bytes that holds 2: two groups, the last one ragged; the budget is read from a handle that ran 2 images (its arena is sized
    from the group), so the test does not restate the library's formula"""
    whole, sd, cfg = _handle("SMALL")
    z, x = _z(cfg, 3, 8, 8), _img(3, 64, 64)
    from univst_amd import vae
    probe = vae.NativeAutoencoderKL(sd, cfg)
    probe.decode(z[:2])
    need2 = int(probe.query("arena_bytes"))
    v = vae.NativeAutoencoderKL(sd, cfg, pass_bytes=need2)
    got = v.decode(z).sample
    assert v.query("passes") == 2 and int(v.query("arena_bytes")) == need2 and v.query("arena_high_water") <= need2
    _hold("passes_decode", got, sd, z, cfg, R.decode)
    mom = v.encode(x).latent_dist.parameters
    assert v.query("passes") == 2
    _hold("passes_encode", mom, sd, x, cfg, R.encode_moments)
    # at the default budget the same input is one pass (equality with it is not required: kernel selection may depend on the row count)
    d_dec = (got.float() - whole.decode(z).sample.float()).abs().max().item()
    assert whole.query("passes") == 1
    d_enc = (mom.float() - whole.encode(x).latent_dist.parameters.float()).abs().max().item()
    assert whole.query("passes") == 1
    _record("passes_vs_one_pass", max_abs_diff_decode=d_dec, max_abs_diff_encode=d_enc)
    one = vae.NativeAutoencoderKL(sd, cfg, pass_bytes=1)            # a group is never smaller than one image
    assert _err(one.decode(z).sample, got)[0] < MAX_BAR and one.query("passes") == 3


def test_attention_scores_beyond_the_fp16_range_stay_finite(nat):
    """to_q / to_k of the decoder's mid block scaled by 400, as tests/test_gpu_vae.py does, on a chunked handle: the softmax clamps the fp16-saturated
    scores on load, so the decode stays finite"""
    from univst_amd import synth, vae
    sd = synth.klvae_state_dict(SMALL, seed=5)
    for k in ("to_q", "to_k"):
        sd[f"decoder.mid_block.attentions.0.{k}.weight"] = sd[f"decoder.mid_block.attentions.0.{k}.weight"] * 400.0
    v = vae.NativeAutoencoderKL(sd, SMALL, attn_score_bytes=128 * 256 * 2)
    z = (torch.randn(2, 16, 16, 16, generator=torch.Generator().manual_seed(2)) * 3).half().cuda()
    got = v.decode(z).sample
    assert v.query("attn_chunks") == 2 and torch.isfinite(got.float()).all()


def test_decode_1024_once(nat):
    """SD3 widths, one image of 1024 x 1024 (128 x 128 latents: 16 384 tokens, a 512 MB score matrix unchunked) at the default budgets: four chunks of
    4096 query rows, against the fp32 restatement on the device"""
    v, sd, cfg = _handle("SD3")
    z = _z(cfg, 1, BIG_LAT, BIG_LAT, seed=6)
    v.decode(z)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = v.decode(z).sample
    torch.cuda.synchronize()
    t_nat = time.perf_counter() - t0
    assert v.query("attn_chunks") == {128: 4, 96: 2}[BIG_LAT] and v.query("passes") == 1
    t0 = time.perf_counter()
    ref = _restated(R.decode, sd, z, cfg)
    torch.cuda.synchronize()
    t_ref = time.perf_counter() - t0
    mx, rms = _err(got, ref)
    print(f"decode {8 * BIG_LAT}^2: max {mx:.3e} rms {rms:.3e} native {t_nat:.3f} s oracle {t_ref:.3f} s arena {v.query('arena_high_water') / 2**20:.0f} MiB")
    _record(f"decode_SD3_1x{BIG_LAT}x{BIG_LAT}", native_max=mx, native_rms=rms, arena_high_water=v.query("arena_high_water"), native_s=t_nat,
            fp32_oracle_on_device_s=t_ref)
    assert mx < MAX_BAR and rms < RMS_BAR, (mx, rms)


def test_behind_the_sd3_call_sites(nat):
    """CustomStableDiffusion3Pipeline._decode and inversion_tools/flow_inversion._img_latents with NativeAutoencoderKL in place of the stock module:
    the shift and scale are applied by the call sites, values against the restated definition"""
    import types
    from univst_amd import synth, vae
    from univst_amd.backbones.video_diffusion_sd3.pipelines.custom_pipeline import CustomStableDiffusion3Pipeline as P
    from univst_amd.inversion_tools import flow_inversion
    sd = synth.klvae_state_dict(SMALL, seed=9)
    L = SMALL["latent_channels"]
    sd["encoder.conv_out.weight"][L:] = 0              # the log-variance head pinned to its clamp (-30): std = exp(-15)
    sd["encoder.conv_out.bias"][L:] = -40.0
    v = vae.NativeAutoencoderKL(sd, SMALL)
    scale, shift = v.config.scaling_factor, v.config.shift_factor
    assert (scale, shift) == (1.5305, 0.0609) and next(v.parameters()).dtype == torch.float16
    pipe = P(transformer=types.SimpleNamespace(), scheduler=None, vae=v)
    lat = (scale * torch.randn(2, L, 8, 8, generator=torch.Generator().manual_seed(4))).half().cuda()
    img = pipe._decode(lat, "np")
    assert img.shape == (2, 64, 64, 3)
    ref = _restated(R.decode, sd, lat.float() / scale + shift, SMALL)
    ref8 = ((ref / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1) * 255).round().cpu()
    assert (torch.from_numpy((img * 255).round()) - ref8).abs().max().item() <= 2          # uint8 levels
    unshifted = _restated(R.decode, sd, lat.float() / scale, SMALL)
    e_nat, e_un = _err(pipe._decode(lat, "pt"), ref)[0], _err(unshifted, ref)[0]
    assert e_nat < MAX_BAR and e_un > 3 * e_nat, (e_nat, e_un)          # the shift matters and is applied
    x = _img(2, 64, 64, seed=5)
    torch.manual_seed(0)
    zl = flow_inversion._img_latents(types.SimpleNamespace(vae=v), x)
    mean = v.encode(x).latent_dist.mean
    assert zl.shape == (2, L, 8, 8) and zl.dtype == torch.float16
    # sample = mean: std = exp(-15); what is left is the fp16 rounding of the call site's two operations
    assert (zl.float() - (mean.float() - shift) * scale).abs().max().item() <= 2 * 2.0 ** -11 * scale * (mean.abs().max().item() + shift)
    torch.manual_seed(0)
    assert torch.equal(zl, (v.encode(x).latent_dist.sample() - shift) * scale)                 # one randn of the device RNG, as the stock class
    mean_ref = _restated(R.encode_moments, sd, x, SMALL)[:, :L]
    mx, rms = _err(zl, (mean_ref - shift) * scale)
    print(f"_img_latents: max {mx:.3e} rms {rms:.3e}")
    assert mx < MAX_BAR and rms < RMS_BAR, (mx, rms)


def test_store_behaviour(nat, tmp_path):
    from safetensors.torch import save_file
    from univst_amd import vae
    v, sd, cfg = _handle("SMALL", seed=17)
    z, x = _z(cfg, 2, 8, 8), _img(2, 64, 64)
    d16, e16 = v.decode(z).sample, v.encode(x).latent_dist.parameters
    # the same fp16-valued weights uploaded as fp32 tensors (converted on the device by the store's one convert kernel): bit-identical
    assert all(t.dtype == torch.float16 for t in sd.values())
    v32 = vae.NativeAutoencoderKL({k: t.float() for k, t in sd.items()}, cfg)
    assert torch.equal(v32.decode(z).sample, d16) and torch.equal(v32.encode(x).latent_dist.parameters, e16) and d16.float().abs().max().item() > 0
    # a missing tensor is named
    k1 = "decoder.up_blocks.1.resnets.2.norm2.bias"
    bad = vae.NativeAutoencoderKL({k: t for k, t in sd.items() if k != k1}, cfg)
    with pytest.raises(RuntimeError, match="was never loaded") as e:
        bad.decode(z)
    assert f"'{k1}'" in str(e.value)
    assert torch.equal(bad.encode(x).latent_dist.parameters, e16)          # the encoder does not read it
    # old attention names as 1x1 convs load as the new ones
    ren = {"to_q": "query", "to_k": "key", "to_v": "value", "to_out.0": "proj_attn"}
    old = {}
    for k, t in sd.items():
        for a, b in ren.items():
            if f".attentions.0.{a}." in k:
                k, t = k.replace(f".{a}.", f".{b}."), (t[:, :, None, None] if k.endswith(".weight") else t)
        old[k] = t
    assert torch.equal(vae.NativeAutoencoderKL(old, cfg).decode(z).sample, d16)
    # from_pretrained: <dir>/vae/config.json + diffusion_pytorch_model.safetensors, no diffusers import, same outputs
    d = tmp_path / "sd3" / "vae"
    d.mkdir(parents=True)
    json.dump({"_class_name": "AutoencoderKL", "_diffusers_version": "0.29.0", "block_out_channels": list(cfg["block_out_channels"]),
               "down_block_types": ["DownEncoderBlock2D"] * 4, "up_block_types": ["UpDecoderBlock2D"] * 4, "force_upcast": True, "in_channels": 3,
               "latent_channels": 16, "layers_per_block": 2, "norm_num_groups": 32, "out_channels": 3, "sample_size": 1024, "scaling_factor": 1.5305,
               "shift_factor": 0.0609, "use_quant_conv": False, "use_post_quant_conv": False, "mid_block_add_attention": True}, open(d / "config.json", "w"))
    save_file({k: t.cpu().contiguous() for k, t in sd.items()}, str(d / "diffusion_pytorch_model.safetensors"))
    had = "diffusers" in sys.modules
    vp = vae.NativeAutoencoderKL.from_pretrained(str(tmp_path / "sd3"), subfolder="vae")
    assert ("diffusers" in sys.modules) == had, "from_pretrained must not import diffusers"
    assert vp.config.scaling_factor == 1.5305 and vp.config.shift_factor == 0.0609 and vp.config.block_out_channels == tuple(cfg["block_out_channels"])
    assert torch.equal(vp.decode(z).sample, d16) and torch.equal(vp.encode(x).latent_dist.parameters, e16)


def test_shape_preconditions_fail_with_named_errors(nat):
    from univst_amd import synth, vae
    v, sd, cfg = _handle("SMALL")
    with pytest.raises(RuntimeError, match="GPU only"):
        v.decode(torch.zeros(1, 16, 8, 8))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        v.decode(torch.zeros(1, 16, 3, 3).half().cuda())                 # 9 tokens
    with pytest.raises(RuntimeError, match="latents have 4 channels"):
        v.decode(torch.zeros(1, 4, 8, 8).half().cuda())
    with pytest.raises(RuntimeError, match="images have 4 channels"):
        v.encode(torch.zeros(1, 4, 64, 64).half().cuda())
    with pytest.raises(RuntimeError, match="multiples of 8"):
        v.encode(torch.zeros(1, 3, 60, 64).half().cuda())
    with pytest.raises(RuntimeError, match="multiple of 8"):
        v.encode(torch.zeros(1, 3, 24, 24).half().cuda())                # 3 x 3 tokens
    with pytest.raises(RuntimeError, match="block_out_channels"):
        vae.NativeAutoencoderKL({}, dict(SMALL, block_out_channels=(64, 128, 128, 100)))
    with pytest.raises(RuntimeError, match="latent_channels=6"):
        vae.NativeAutoencoderKL({}, dict(SMALL, latent_channels=6))
    with pytest.raises(RuntimeError, match="unknown quantity"):
        v.query("nothing")


def test_native_klvae_against_the_diffusers_class(nat):
    """the native graph against the THIRD-PARTY class itself (not the repo's own restatement): a random-init diffusers.AutoencoderKL at SMALL widths, its
    state dict through NativeAutoencoderKL.from_module, decode and encode mean compared.  Skipped where diffusers is not importable: parity stays
    unpinned until this has run once somewhere."""
    diffusers = pytest.importorskip("diffusers")
    from univst_amd import vae
    torch.manual_seed(0)
    stock = diffusers.AutoencoderKL(in_channels=3, out_channels=3, latent_channels=16, block_out_channels=SMALL["block_out_channels"], layers_per_block=2,
                                    down_block_types=("DownEncoderBlock2D",) * 4, up_block_types=("UpDecoderBlock2D",) * 4, norm_num_groups=32,
                                    use_quant_conv=False, use_post_quant_conv=False, sample_size=64).half().cuda().eval()
    v = vae.NativeAutoencoderKL.from_module(stock)
    z, x = _z(SMALL, 2, 8, 8), _img(2, 64, 64)
    with torch.no_grad():
        stock = stock.float()
        mx, rms = _err(v.decode(z).sample, stock.decode(z.float()).sample)
        assert mx < MAX_BAR and rms < RMS_BAR, ("decode", mx, rms)
        mx, rms = _err(v.encode(x).latent_dist.mean, stock.encode(x.float()).latent_dist.mean)
        assert mx < MAX_BAR and rms < RMS_BAR, ("encode", mx, rms)
