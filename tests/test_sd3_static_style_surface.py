"""No GPU: the public surface of the SD3 static style branch and of the dead-branch skip — the keywords and their defaults, the CLI flags, the
start script's switches, the two shapes of style inversion entries, and the two C-ABI entries in the header and the binding."""
import inspect
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keywords_and_defaults():
    from univst_amd import _native
    from univst_amd.backbones.video_diffusion_sd3 import pnp_utils
    from univst_amd.backbones.video_diffusion_sd3.models.transformer_3D_model import CustomSD3Transformer2DModel
    from univst_amd.backbones.video_diffusion_sd3.pipelines.custom_pipeline import CustomStableDiffusion3Pipeline
    sig = inspect.signature(CustomStableDiffusion3Pipeline.video_style_transfer).parameters
    assert sig["static_style"].default is False and sig["skip_dead_branches"].default is False
    assert list(inspect.signature(CustomSD3Transformer2DModel.style_bank).parameters) == ["self", "frame", "timestep", "enc1", "pooled1", "idx", "bank"]
    assert inspect.signature(CustomSD3Transformer2DModel.style_bank).parameters["bank"].default is None
    assert list(inspect.signature(CustomSD3Transformer2DModel.forward_static_style).parameters) == ["self", "sample2", "timestep", "enc2", "pooled2",
                                                                                                    "idx", "bank"]
    for proc in (pnp_utils.CrossFrameProcessor, pnp_utils.AttentionShiftProcessor):
        p = inspect.signature(proc.__call__).parameters["static_style"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    sig = inspect.signature(_native.sd3_joint_attention).parameters
    assert sig["style_kv"].default is None and sig["static_role"].default is None
    assert callable(_native.sd3_adain_shift_static_)
    bank = pnp_utils.StaticStyleBank()
    assert bank.mode == "write" and bank.buffers() == [] and bank.nbytes() == 0


def test_window_is_read_from_the_registered_processors():
    from types import SimpleNamespace
    from univst_amd.backbones.video_diffusion_sd3 import pnp_utils as pu
    tr = SimpleNamespace(attn_processors={"a": pu.AttentionShiftProcessor(0.0, 0.6), "b": pu.AttentionShiftProcessor(0.0, 0.6)})
    w = pu.shift_window(tr)
    assert w == (0.0, 0.6)
    assert [i for i in range(50) if not pu.window_open(w, i)] == list(range(31, 50))          # 19 of 50 steps are outside
    assert pu.window_open((0.3, 0.6), 15) and not pu.window_open((0.3, 0.6), 14)             # eta1 * 50 in double: step 15 is inside
    assert pu.shift_window(SimpleNamespace(attn_processors={"a": pu.CrossFrameProcessor()})) is None and not pu.window_open(None, 10)
    tr.attn_processors["b"] = pu.AttentionShiftProcessor(0.0, 0.5)
    with pytest.raises(ValueError, match="disagree"):
        pu.shift_window(tr)


def test_cli_flags_and_script():
    from univst_amd.src.sd3 import run_style_inversion_sd3 as inv, run_video_style_transfer_sd3 as tr
    for mod in (inv, tr):
        assert mod.parser().parse_args([]).static_style is False
        assert mod.parser().parse_args(["--static_style"]).static_style is True
    assert tr.parser().parse_args([]).skip_dead_branches is False
    assert tr.parser().parse_args(["--skip_dead_branches"]).skip_dead_branches is True
    sh = open(os.path.join(ROOT, "scripts", "start_sd3.sh")).read()
    assert '"${STATIC_STYLE:-0}" = "1"' in sh and sh.count("$STATIC") >= 2
    lines = [ln for ln in sh.splitlines() if "$STATIC" in ln]
    assert any("run_style_inversion_sd3.py" in ln for ln in lines), "the one-frame inversion"
    assert any("--output_path results/stylizations" in ln for ln in lines), "the transfer"


@pytest.mark.parametrize("frames", [1, 5])
def test_both_latent_shapes_are_accepted_and_a_third_is_refused(frames):
    """a style inversion entry as [F, 16, h, w] (the image repeated; frame 0 is taken) or [1, 16, h, w] (--static_style inversion)"""
    from univst_amd.backbones.video_diffusion_sd3.pipelines.custom_pipeline import static_style_frame
    F = 5
    z = torch.randn(frames, 16, 6, 6)
    one = static_style_frame(z, F, (16, 6, 6))
    assert tuple(one.shape) == (1, 16, 6, 6) and torch.equal(one, z[:1])
    with pytest.raises(ValueError, match=r"got \(3, 16, 6, 6\)"):
        static_style_frame(torch.zeros(3, 16, 6, 6), F, (16, 6, 6))
    with pytest.raises(ValueError, match="static_style"):
        static_style_frame(torch.zeros(frames, 16, 6, 8), F, (16, 6, 6))
    with pytest.raises(ValueError, match="static_style"):
        static_style_frame(torch.zeros(16, 6, 6), F, (16, 6, 6))


def test_entries_are_declared_and_bound():
    import ctypes as C
    from univst_amd import _native
    hdr = open(os.path.join(ROOT, "include", "univst.h")).read()
    for name in ("univst_sd3_adain_shift_static", "univst_sd3_joint_attention_static"):
        assert name + "(" in hdr and name in _native.SIGNATURES
    assert "#define UNIVST_ABI_VERSION 3" in hdr
    lib = _native.load()
    assert lib.univst_abi_version() == 3
    # the mx entry's arguments without comm, then style_kv, ld_style, role
    mx, st = _native.SIGNATURES["univst_sd3_joint_attention_mx"][1], _native.SIGNATURES["univst_sd3_joint_attention_static"][1]
    assert st == mx[:16] + mx[17:] + [C.c_void_p, C.c_int64, C.c_int]
    # refused on the host before anything touches a device: null pointers are argument errors, not crashes
    assert lib.univst_sd3_adain_shift_static(None, 120, None, 80, 2, 5, 40, 5, 0.8, 0.5, 2.0, None, None) != 0
    with pytest.raises(RuntimeError, match="qkv2"):
        _native.check(lib.univst_sd3_adain_shift_static(None, 120, None, 80, 2, 5, 40, 5, 0.8, 0.5, 2.0, None, None), "sd3_adain_shift_static")
    with pytest.raises(RuntimeError, match="role=2"):
        _native.check(lib.univst_sd3_joint_attention_static(None, None, None, 2, 16, 0, 64, 1, 64, 1, 0, 0.0, 1e-6, None, None, None, None, None, None, 0, 2),
                      "sd3_joint_attention_static")
