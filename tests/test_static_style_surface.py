"""No GPU: the public surface of the static style branch — the new keyword and its default, the CLI flags, the two shapes of style
inversion files, and the C-ABI entries in the header and the binding."""
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keyword_and_default():
    from univst_amd import engine
    from univst_amd.backbones.video_diffusion_sd.pipelines.stable_diffusion import SpatioTemporalStableDiffusionPipeline
    from univst_amd.backbones.video_diffusion_sd.models.unet_3d_condition import UNetPseudo3DConditionModel
    p = inspect.signature(engine.transfer_loop).parameters["static_style"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False and p.annotation is bool
    p = inspect.signature(SpatioTemporalStableDiffusionPipeline.video_style_transfer).parameters["static_style"]
    assert p.default is False
    assert list(inspect.signature(UNetPseudo3DConditionModel.style_bank).parameters)[:4] == ["self", "frame", "timestep", "text"]
    assert list(inspect.signature(UNetPseudo3DConditionModel.forward_static_style).parameters) == ["self", "sample2", "timestep", "text2", "bank"]


def test_cli_flags():
    from univst_amd.src.sd import run_style_inversion_sd as inv, run_video_style_transfer_sd as tr
    for mod in (inv, tr):
        assert mod.parser().parse_args([]).static_style is False
        assert mod.parser().parse_args(["--static_style"]).static_style is True
    sh = open(os.path.join(ROOT, "scripts", "start_sd.sh")).read()
    assert '"${STATIC_STYLE:-0}" = "1"' in sh and sh.count("$STATIC") >= 2


@pytest.mark.parametrize("frames", [1, 5])
def test_both_latent_file_shapes_are_accepted(tmp_path, frames):
    """ddim_latents_k.pt as [1,4,F,h,w] (the image repeated) or [1,4,1,h,w] (--static_style inversion): the static loop takes one frame of either,
    the three-branch loop F frames of either; anything else is refused by shape"""
    from univst_amd import engine
    from univst_amd.src.util import load_ddim_latents_at_t
    F = 5
    z = torch.randn(1, 4, 1, 8, 8).expand(-1, -1, frames, -1, -1).contiguous()
    torch.save(z, tmp_path / "ddim_latents_7.pt")
    t = load_ddim_latents_at_t(7, str(tmp_path))
    assert tuple(t.shape) == (1, 4, frames, 8, 8)
    one = engine.style_inv_frames(t, F, True)
    assert tuple(one.shape) == (1, 4, 1, 8, 8) and one.is_contiguous() and torch.equal(one, z[:, :, :1])
    full = engine.style_inv_frames(t, F, False)
    assert tuple(full.shape) == (1, 4, F, 8, 8) and all(torch.equal(full[:, :, f], z[:, :, 0]) for f in range(F))
    with pytest.raises(ValueError, match="style inversion latent"):
        engine.style_inv_frames(torch.zeros(1, 4, 3, 8, 8), F, True)


def test_entries_are_declared_and_bound():
    from univst_amd import _native
    hdr = open(os.path.join(ROOT, "include", "univst.h")).read()
    for name in ("univst_unet_style_bank_bytes", "univst_unet_style_bank", "univst_unet_forward_static_style", "univst_attention_adain_shift_static"):
        assert name + "(" in hdr and name in _native.SIGNATURES
    assert "#define UNIVST_ABI_VERSION 3" in hdr
    lib = _native.load()
    assert lib.univst_unet_style_bank_bytes(None, 16, 16) == -1        # a null handle is an argument error, not a crash
