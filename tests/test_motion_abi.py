"""CPU: the host side of the motion-module handle (univst_motion_create refuses a bad config before any GPU call and names the field) and the
constructor of the mirror (univst_amd/backbones/animatediff/models/motion_module.py), whose parameter names and shapes are the reference's: checked
against the key list of golden g20."""
import ctypes as C
import os

import pytest
import torch

from univst_amd import _native

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g20_motion_module.pt")


def create(**over):
    cfg = dict(channels=320, num_heads=8, num_blocks=1, attn_per_block=2, norm_groups=32, max_len=24, position_encoding=1, gn_eps=1e-6, ln_eps=1e-5)
    cfg.update(over)
    lib = _native.load()
    h = C.c_void_p()
    rc = lib.univst_motion_create(C.byref(_native.MotionCfg(*[cfg[k] for k, _ in _native.MotionCfg._fields_])), C.byref(h))
    err = lib.univst_last_error().decode()
    if rc == 0:
        assert h.value
        assert lib.univst_motion_destroy(h) == 0
    return rc, err


@pytest.mark.parametrize("over,field", [(dict(channels=512), "num_heads"),          # head dim 64
                                        (dict(channels=320, norm_groups=48), "norm_groups"),
                                        (dict(max_len=33), "max_len"),
                                        (dict(max_len=0), "max_len")])
def test_create_refuses_a_bad_config_and_names_the_field(over, field):
    rc, err = create(**over)
    assert rc == -1 and field in err, (rc, err)


@pytest.mark.parametrize("channels", [320, 640, 1280])
def test_create_accepts_the_real_widths(channels):
    rc, err = create(channels=channels)
    assert rc == 0, err


def test_query_and_forward_refuse_a_null_handle():
    lib = _native.load()
    out = C.c_double()
    assert lib.univst_motion_query(None, b"arena_high_water", C.byref(out)) == -1
    assert lib.univst_motion_forward(None, None, None, 1, 1, 1, None) == -1


def test_mirror_keeps_the_reference_names_and_shapes():
    from univst_amd.backbones.animatediff.models.motion_module import VanillaTemporalModule, get_motion_module
    want = {k: tuple(v.shape) for k, v in torch.load(GOLD)["state_dict"].items()}
    m = VanillaTemporalModule(in_channels=64, num_attention_heads=4, temporal_position_encoding=True, temporal_position_encoding_max_len=24,
                              zero_initialize=False)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    m.load_state_dict({k: v.float() for k, v in torch.load(GOLD)["state_dict"].items()}, strict=True)
    assert tuple(m.temporal_transformer.transformer_blocks[0].attention_blocks[1].pos_encoder.pe.shape) == (1, 24, 64)
    z = get_motion_module(320, "Vanilla", dict(num_attention_heads=8, num_transformer_block=1, attention_block_types=["Temporal_Self", "Temporal_Self"],
                                               temporal_position_encoding=True, temporal_attention_dim_div=1, zero_initialize=True))
    assert len(z.temporal_transformer.transformer_blocks) == 1
    assert z.temporal_transformer.proj_out.weight.abs().max() == 0 and z.temporal_transformer.proj_out.bias.abs().max() == 0
    assert z.temporal_transformer.proj_in.weight.abs().max() > 0


def test_mirror_says_what_is_unsupported():
    from univst_amd.backbones.animatediff.models.motion_module import VanillaTemporalModule, get_motion_module
    with pytest.raises(NotImplementedError, match="Temporal_Cross"):
        VanillaTemporalModule(320, attention_block_types=("Temporal_Self", "Temporal_Cross"))
    with pytest.raises(NotImplementedError, match="temporal_attention_dim_div"):
        VanillaTemporalModule(320, temporal_attention_dim_div=2)
    with pytest.raises(ValueError, match="Vanilla"):
        get_motion_module(320, "Other", {})
    m = VanillaTemporalModule(320, num_transformer_block=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 320, 2, 2, 2), None, None)


def test_reference_import_path_resolves_to_the_mirror():
    import importlib
    shim = importlib.import_module("backbones.animatediff.models.motion_module")
    prod = importlib.import_module("univst_amd.backbones.animatediff.models.motion_module")
    for n in ("get_motion_module", "VanillaTemporalModule"):
        assert getattr(shim, n) is getattr(prod, n)


def test_the_rest_of_the_animatediff_package_still_resolves_behind_the_shim(tmp_path):
    """INTEGRATION.md level 1: this repository goes on the path BEFORE a UniVST checkout, whose backbones/ directories are namespace portions.  The two
    __init__.py shims extend their __path__, so a module this repository does not provide (models/unet.py, pipelines/...) is still found there."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    other = tmp_path / "checkout" / "backbones" / "animatediff"
    (other / "models").mkdir(parents=True)
    (other / "pipelines").mkdir()
    (other / "models" / "unet_blocks.py").write_text("WHERE = 'checkout'\n")
    (other / "models" / "motion_module.py").write_text("WHERE = 'checkout'\n")
    (other / "pipelines" / "pipeline_animation.py").write_text("WHERE = 'checkout'\n")
    code = ("import backbones.animatediff.models.unet_blocks as u, backbones.animatediff.pipelines.pipeline_animation as p, "
            "backbones.animatediff.models.motion_module as m; print(u.WHERE, p.WHERE, m.__file__)")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=str(tmp_path),
                         env=dict(os.environ, PYTHONPATH=os.pathsep.join([root, str(tmp_path / "checkout")])), timeout=120)
    assert out.returncode == 0, out.stderr[-600:]
    u, p, m = out.stdout.split()
    assert (u, p) == ("checkout", "checkout") and os.path.abspath(m).startswith(root)


def test_temporal_attention_refuses_on_the_host_before_any_launch():
    """the launcher's argument checks are plain host code in front of the launch, so they answer without a GPU; each message names its argument.
    N * heads beyond 2^24 would not fit the grid's x dimension (B * F * N < 2^31 alone allows it at F = 1)."""
    lib = _native.load()
    buf = (C.c_char * 4096)()
    a = (C.addressof(buf) + 255) & ~255
    for kw, word in ((dict(F=0), "F=0"), (dict(F=33), "F=33"), (dict(d=64), "head_dim=64"), (dict(ldx=964), "ldx=964"), (dict(ldo=322), "ldo=322"),
                     (dict(F=1, N=(1 << 21) + 1), "N * heads"), (dict(B=3, F=32, N=1 << 25), "B * F * N"), (dict(B=70000), "B=70000")):
        v = dict(B=1, F=8, N=4, heads=8, d=40, ldx=960, ldo=320)
        v.update(kw)
        rc = lib.univst_temporal_attention(a, v["ldx"], None, v["B"], v["F"], v["N"], v["heads"], v["d"], a + 2048, v["ldo"], None)
        err = lib.univst_last_error().decode()
        assert rc == -1 and word in err, (kw, rc, err)


def test_mirror_copies_and_pickles_without_its_handle():
    import copy
    import pickle
    from univst_amd.backbones.animatediff.models.motion_module import VanillaTemporalModule
    m = VanillaTemporalModule(320, num_transformer_block=1, temporal_position_encoding=True, zero_initialize=False)
    m._native, m._native_fp = C.c_void_p(1), 7          # what a forward leaves: an object that cannot be copied
    for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
        assert twin._native is None and twin._native_fp is None
        assert all(torch.equal(v, twin.state_dict()[k]) for k, v in m.state_dict().items())
    m._native = None
