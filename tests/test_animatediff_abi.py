"""CPU: the host side of the AnimateDiff UNet handle (univst_unet_create_animatediff refuses a bad config before any GPU call and names the
argument; the handle refuses a communicator and motion_fold = 1) and of its Python mirror (loading, copies, shims)."""
import ctypes as C
import json
import os
import sys

import pytest
import torch

from univst_amd import _native

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import animatediff_ref as R  # noqa: E402

UNSUPPORTED = -3


def create(boc=(320, 640, 1280, 1280), heads=8, mask=15, mid=1, inflated=1, keep=False, **motion):
    mc = dict(channels=0, num_heads=8, num_blocks=1, attn_per_block=2, norm_groups=32, max_len=24, position_encoding=1, gn_eps=1e-6, ln_eps=1e-5)
    mc.update(motion)
    lib = _native.load()
    cfg = _native.UnetCfg(4, 4, (C.c_int * 4)(*boc), 2, 768, (C.c_int * 4)(*([heads] * 4)), 32, 1e-5, 1, 0.0)
    ad = _native.AnimateDiffCfg(inflated, mask, mid, _native.MotionCfg(*[mc[k] for k, _ in _native.MotionCfg._fields_]))
    h = C.c_void_p()
    rc = lib.univst_unet_create_animatediff(C.byref(cfg), C.byref(ad), C.byref(h))
    err = lib.univst_last_error().decode()
    if rc == 0 and not keep:
        assert h.value and lib.univst_unet_destroy(h) == 0
    return (rc, err, h) if keep else (rc, err)


def test_exports_exist():
    lib = _native.load()
    assert hasattr(lib, "univst_unet_create_animatediff") and "univst_unet_create_animatediff" in _native.SIGNATURES
    assert lib.univst_abi_version() == 3, "an added entry point leaves the ABI version alone"
    assert [n for n, _ in _native.AnimateDiffCfg._fields_] == ["inflated_groupnorm", "motion_levels_mask", "motion_mid_block", "motion"]
    assert C.sizeof(_native.AnimateDiffCfg) == 3 * 4 + C.sizeof(_native.MotionCfg)


def test_create_accepts_the_v2_configuration():
    assert create()[0] == 0
    assert create(mask=0, mid=0, num_heads=7)[0] == 0, "no motion module: the motion config is not looked at"
    assert create(boc=(160, 160, 320, 320), heads=4, num_heads=4)[0] == 0


@pytest.mark.parametrize("kw,words", [(dict(num_heads=5), ("block_out_channels[0]=320", "num_heads")),            # head dim 64
                                      (dict(boc=(320, 640, 1280, 2560)), ("block_out_channels[3]=2560", "num_heads")),   # head dim 320 at the deepest level
                                      (dict(mask=1, mid=1, boc=(320, 512, 512, 2560)), ("block_out_channels[3]=2560",)),   # the mid block alone reaches level 3
                                      (dict(norm_groups=48), ("norm_groups",)),
                                      (dict(max_len=33), ("max_len",)),
                                      (dict(mask=16), ("motion_levels_mask",)),
                                      (dict(inflated=2), ("inflated_groupnorm",))])
def test_create_refuses_a_bad_config_and_names_the_argument(kw, words):
    rc, err = create(**kw)
    assert rc == -1 and all(w in err for w in words), (rc, err)


def test_create_ignores_levels_without_modules():
    assert create(mask=1, mid=0, boc=(320, 512, 512, 512))[0] == 0, "only level 0 has modules: the other widths need no motion head dim"


def test_handle_refuses_what_it_cannot_do():
    rc, err, h = create(keep=True)
    assert rc == 0, err
    lib = _native.load()
    try:
        assert lib.univst_unet_set_comm(h, 0, 1, None, 0, _native.ALLREDUCE_FN(), _native.KVEXCHANGE_FN(), None) == UNSUPPORTED
        assert "every frame on one rank" in lib.univst_last_error().decode()
        assert lib.univst_unet_set_comm_native(h, C.c_void_p(8)) == UNSUPPORTED
        assert lib.univst_unet_set_option(h, b"motion_fold", 0) == 0
        assert lib.univst_unet_set_option(h, b"motion_fold", 1) == UNSUPPORTED and "not built" in lib.univst_last_error().decode()
        assert lib.univst_unet_set_option(h, b"motion_fold", 2) == -1
        shape = (C.c_int64 * 1)(320)
        assert lib.univst_unet_load_tensor(h, b"down_blocks.0.motion_modules.2.temporal_transformer.norm.weight", None, 0, shape, 1, None) == -1
        assert "motion_modules.2" in lib.univst_last_error().decode(), "layers_per_block = 2: a down block has modules 0 and 1"
        out = C.c_double(-1)
        assert lib.univst_unet_query(h, b"arena_high_water", C.byref(out)) == 0 and out.value == 0
    finally:
        lib.univst_unet_destroy(h)
    h2 = C.c_void_p()
    cfg = _native.UnetCfg(4, 4, (C.c_int * 4)(320, 640, 1280, 1280), 2, 768, (C.c_int * 4)(8, 8, 8, 8), 32, 1e-5, 1, 0.0)
    assert lib.univst_unet_create(C.byref(cfg), C.byref(h2)) == 0
    try:
        assert lib.univst_unet_set_option(h2, b"motion_fold", 0) == -1, "the SD handle has no such option"
    finally:
        lib.univst_unet_destroy(h2)


def tiny_kwargs():
    return R.reference_kwargs(R.G21_CFG)


def test_from_pretrained_2d_and_a_motion_checkpoint(tmp_path):
    """from_pretrained_2d over a local config.json + weights leaves the motion modules at their initialisation (proj_out zero with zero_initialize);
    load_state_dict(strict=False) of a motion checkpoint — what utils/util.py load_weights does — then fills them and nothing else"""
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel, WEIGHTS_NAME
    cfg = R.G21_CFG
    sd = R.random_state_dict(cfg, seed=5)
    two_d = {k: v for k, v in sd.items() if ".motion_modules." not in k}
    sub = tmp_path / "sd" / "unet"
    sub.mkdir(parents=True)
    kw = tiny_kwargs()
    conf = {k: (list(v) if isinstance(v, tuple) else v) for k, v in kw.items() if not k.startswith(("motion", "use_", "unet_use"))}
    conf.update(_class_name="UNet2DConditionModel", mid_block_type="UNetMidBlock2DCrossAttn", down_block_types=["CrossAttnDownBlock2D"] * 3 + ["DownBlock2D"],
                up_block_types=["UpBlock2D"] + ["CrossAttnUpBlock2D"] * 3)
    (sub / "config.json").write_text(json.dumps(conf))
    torch.save(two_d, str(sub / WEIGHTS_NAME))
    extra = {k: v for k, v in kw.items() if k.startswith(("motion", "use_", "unet_use"))}
    extra["motion_module_kwargs"] = dict(extra["motion_module_kwargs"], zero_initialize=True)
    m = UNet3DConditionModel.from_pretrained_2d(str(tmp_path / "sd"), subfolder="unet", unet_additional_kwargs=extra)
    got = m.state_dict()
    assert set(got) == set(sd)
    assert all(torch.equal(got[k], v) for k, v in two_d.items())
    po = [k for k in got if ".motion_modules." in k and ".proj_out." in k]
    assert len(po) == 42 and all(got[k].abs().max() == 0 for k in po)
    motion = {k: v for k, v in sd.items() if ".motion_modules." in k}
    motion["down_blocks.0.motion_modules.0.temporal_transformer.transformer_blocks.0.attention_blocks.0.pos_encoder.pe"] = torch.zeros(1, 24, 32)
    missing, unexpected = m.load_state_dict(motion, strict=False)
    assert set(missing) == set(two_d) and unexpected == [next(k for k in motion if k.endswith("pos_encoder.pe"))]
    assert all(torch.equal(m.state_dict()[k], v) for k, v in sd.items()) and m._native_dirty
    with pytest.raises(RuntimeError, match="config.json"):
        UNet3DConditionModel.from_pretrained_2d(str(tmp_path / "nowhere"), unet_additional_kwargs=extra)


def test_mirror_says_what_is_unsupported():
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    kw = tiny_kwargs()
    for over, word in ((dict(unet_use_cross_frame_attention=True), "cross_frame"), (dict(motion_module_decoder_only=True), "decoder_only"),
                       (dict(use_linear_projection=True), "use_linear_projection")):
        with pytest.raises(NotImplementedError, match=word):
            UNet3DConditionModel(**dict(kw, **over))
    m = UNet3DConditionModel(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 4, 2, 16, 16), 1, torch.zeros(1, 6, 16))


def test_mirror_copies_and_pickles_without_its_handle():
    import copy
    import pickle
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    m = UNet3DConditionModel(**tiny_kwargs())
    m._native_handle, m._native_dirty, m._native_fp = C.c_void_p(1), False, 7          # what a forward leaves: an object that cannot be copied
    try:
        for twin in (copy.deepcopy(m), pickle.loads(pickle.dumps(m))):
            assert twin._native_handle is None and twin._native_dirty and twin._native_fp is None
            assert all(torch.equal(v, twin.state_dict()[k]) for k, v in m.state_dict().items())
    finally:
        m._native_handle = None


def test_pnp_registration_is_read_back():
    import types
    from univst_amd.backbones.animatediff import pnp_utils
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    m = UNet3DConditionModel(**tiny_kwargs())
    assert m._pnp_state() is None
    pipe = types.SimpleNamespace(unet=m)
    pnp_utils.register_spatial_attention_pnp(pipe, eta1=0.0, eta2=0.5)
    with pytest.raises(RuntimeError, match="register_time"):
        m._pnp_state()
    pnp_utils.register_time(pipe, 24)
    p = m._pnp_state()
    assert (p.registered, p.idx, p.eta1, p.eta2) == (1, 24, 0.0, 0.5) and abs(p.alpha - 0.8) < 1e-6 and p.gamma == 2.0
    assert m.up_blocks[1].attentions[1].transformer_blocks[0].attn2.idx == 24 and not hasattr(m.up_blocks[1].attentions[0].transformer_blocks[0].attn1, "idx")


def test_reference_import_paths_resolve_to_the_mirror():
    import importlib
    for mod, names in (("backbones.animatediff.models.unet", ("UNet3DConditionModel", "InflatedConv3d", "InflatedGroupNorm")),
                       ("backbones.animatediff.pnp_utils", ("register_time", "register_spatial_attention_pnp", "attention_adain", "latent_adain"))):
        shim, prod = importlib.import_module(mod), importlib.import_module("univst_amd." + mod)
        for n in names:
            assert getattr(shim, n) is getattr(prod, n)
