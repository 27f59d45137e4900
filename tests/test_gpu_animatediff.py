"""GPU: the native AnimateDiff UNet3D (csrc/unet.hip behind univst_unet_create_animatediff, through the mirror
univst_amd/backbones/animatediff/models/unet.py) against the restatement tests/animatediff_ref.py, which tests/test_animatediff_ref.py holds to the
reference's own classes (golden g21).

Yardstick of every whole-UNet comparison (tests/test_gpu_motion.py::test_module_against_fp64_restatement): the reference runs this UNet in torch fp16
on this GPU, i.e. the restatement in fp16, whose distance to the fp64 restatement is e_ref; the native graph must be finite and within 2 x e_ref in
the maximum norm.  Both figures are printed.

The tiny configuration: block_out_channels (160, 160, 320, 320) with 4 heads for the spatial and the motion attention alike, i.e. head dims 40 and 80,
the smallest the frame-axis kernel has; 16x16 latents give N = 256 / 64 / 16 / 4 tokens per frame, the last of which leaves the `% 16` statistics
route of the GroupNorms.

motion_fold = 1 is not built, so its 0-vs-1 case is absent; the run-to-run determinism of the unfolded chain is checked."""
import ctypes as C
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import animatediff_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

TINY = R.make_cfg(block_out_channels=(160, 160, 320, 320), cross_attention_dim=32, attention_head_dim=4, norm_num_groups=32, motion_heads=4, max_len=24)
CFGS = {
    "tiny": TINY,
    "gn5d": dict(TINY, use_inflated_groupnorm=False),
    "nomid": dict(TINY, motion_mid_block=False),
    "nomotion": dict(TINY, motion_levels=(False,) * 4, motion_mid_block=False),
    # a level at an SD-v1.5 width: C = 320 with 8 heads (head dim 40), motion modules at that level only; the other levels are narrow (their widths
    # have no motion head dim at 8 heads, and need none).  At (1, 4, 32, 32) — 4 096 rows — the level still runs on the small-problem kernels; at
    # (3, 4, 64, 64) — 49 152 rows, 4 096 tokens per frame — it runs on the kernels of a full-size step (test_full_size_level_...)
    "sd_level": R.make_cfg(block_out_channels=(320, 160, 160, 160), cross_attention_dim=32, attention_head_dim=(8, 4, 4, 4), norm_num_groups=32,
                           motion_levels=(True, False, False, False), motion_mid_block=False, motion_heads=8, max_len=24),
}
TEXT_LEN = 77
_MODELS, _SDS, _REFS = {}, {}, {}


def weights(name, zero_motion=False):
    key = (name, zero_motion)
    if key not in _SDS:
        _SDS[key] = R.random_state_dict(CFGS[name], seed=21, zero_motion=zero_motion)
    return _SDS[key]


def mirror(name, sd=None):
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    m = UNet3DConditionModel(**R.reference_kwargs(CFGS[name]))
    m.load_state_dict(weights(name) if sd is None else sd, strict=True)
    return m.half().cuda().eval()


def model(name):
    if name not in _MODELS:
        _MODELS[name] = mirror(name)
    return _MODELS[name]


def inputs(B, F, H, W, D=32):
    g = torch.Generator().manual_seed(B * 1000 + F * 100 + H + W)
    return torch.randn(B, 4, F, H, W, generator=g).half().cuda(), torch.randn(B, TEXT_LEN, D, generator=g).half().cuda()


def refs(name, shape, idx=None):
    """the fp64 and fp16 restatement outputs of one case, computed once"""
    key = (name, shape, idx)
    if key not in _REFS:
        x, txt = inputs(*shape)
        pnp = None if idx is None else dict(idx=idx, eta1=0.0, eta2=0.5)
        with torch.no_grad():
            _REFS[key] = tuple(R.unet_forward(weights(name), CFGS[name], x, 481, txt, pnp=pnp, dtype=dt) for dt in (torch.float64, torch.float16))
    return _REFS[key]


def register(m, idx):
    from univst_amd.backbones.animatediff import pnp_utils
    pipe = types.SimpleNamespace(unet=m)
    pnp_utils.register_spatial_attention_pnp(pipe, eta1=0.0, eta2=0.5)
    pnp_utils.register_time(pipe, idx)


def unregister(m):
    from univst_amd.backbones.animatediff.pnp_utils import PNP_LAYERS
    for r, bs in PNP_LAYERS.items():
        for b in bs:
            m.up_blocks[r].attentions[b].transformer_blocks[0].attn1.__dict__.pop("_univst_native_pnp", None)


def within_bound(tag, got, r64, r16):
    e_nat, e_ref = (got.double() - r64).abs().max().item(), (r16.double() - r64).abs().max().item()
    print(f"{tag}: e_native {e_nat:.3e}, e_ref (torch fp16) {e_ref:.3e}, ratio {e_nat / e_ref:.2f}, max|want| {r64.abs().max().item():.2f}")
    assert got.shape == r64.shape and got.dtype == torch.float16 and torch.isfinite(got).all()
    assert e_nat <= 2 * e_ref, (tag, e_nat, e_ref)


@pytest.mark.parametrize("name,shape", [("tiny", (1, 3, 16, 16)),          # the stock forward
                                        ("tiny", (1, 2, 16, 24)),          # non-square
                                        ("tiny", (1, 17, 16, 16)),         # F > 16: the two-tile instantiation of the frame-axis attention
                                        ("gn5d", (1, 3, 16, 16)),          # inflated_groupnorm = 0: statistics over all frames of a branch
                                        ("nomid", (1, 3, 16, 16)),         # motion_mid_block = 0
                                        ("sd_level", (1, 4, 32, 32))])     # C = 320, 8 heads, N = 1024, F = 4
def test_forward_against_fp64_restatement(name, shape):
    x, txt = inputs(*shape)
    got = model(name)(x, 481, txt).sample
    within_bound(f"{name} {shape}", got, *refs(name, shape))
    if name == "tiny" and shape == (1, 3, 16, 16):
        assert model(name).native_query("motion_active") == 21
        zero = R.unet_forward(weights("tiny", zero_motion=True), TINY, x, 481, txt, dtype=torch.float64)
        assert (zero - refs(name, shape)[0]).abs().max() > 50 * (refs(name, shape)[1].double() - refs(name, shape)[0]).abs().max(), "the modules matter at this seed"


@pytest.mark.parametrize("idx", [0, 24])
def test_pnp_inside_the_window(idx):
    """B = 3 (content, style, stylised), alpha 0.8 and gamma 2.0 as this backbone's pnp_utils has them; only branch 2 differs from the stock forward"""
    shape = (3, 2, 16, 16)
    x, txt = inputs(*shape)
    m = model("tiny")
    unregister(m)
    stock = m(x, 481, txt).sample
    register(m, idx)
    try:
        got = m(x, 481, txt).sample
    finally:
        unregister(m)
    within_bound(f"pnp idx {idx}", got, *refs("tiny", shape, idx))
    assert torch.equal(got[:2], stock[:2]) and not torch.equal(got[2], stock[2])
    r64, s64 = refs("tiny", shape, idx)[0], refs("tiny", shape)[0]
    assert (r64 - s64).abs().max() > 50 * (refs("tiny", shape)[1].double() - s64).abs().max(), "the shift matters at this seed"


def test_pnp_window_is_exclusive_at_the_top():
    """idx 25 = eta2 * 50: the registered forward equals the unregistered one bit for bit (the SD path's window would still shift here)"""
    x, txt = inputs(3, 2, 16, 16)
    m = model("tiny")
    unregister(m)
    stock = m(x, 481, txt).sample
    register(m, 25)
    try:
        got = m(x, 481, txt).sample
    finally:
        unregister(m)
    assert torch.equal(got, stock)


def test_zero_proj_out_is_skipped_exactly():
    """motion_levels_mask = 0 / motion_mid_block = 0 equals the same weights with every proj_out zero, bit for bit: the identity skip"""
    x, txt = inputs(1, 3, 16, 16)
    zero = weights("tiny", zero_motion=True)
    with_modules = mirror("tiny", zero)
    without = mirror("nomotion", {k: v for k, v in zero.items() if ".motion_modules." not in k})
    a, b = with_modules(x, 481, txt).sample, without(x, 481, txt).sample
    assert with_modules.native_query("motion_active") == 0
    assert torch.equal(a, b)
    assert not torch.equal(a, model("tiny")(x, 481, txt).sample)


def test_motion_checkpoint_loaded_after_the_2d_weights_changes_the_output():
    """from_pretrained_2d leaves zero-initialised modules: the UNet equals the per-frame 2-D UNet; load_state_dict(strict=False) of the motion keys
    (utils/util.py load_weights) rebuilds the handle and then equals the fully loaded model"""
    from univst_amd.backbones.animatediff.models.unet import UNet3DConditionModel
    x, txt = inputs(1, 3, 16, 16)
    kw = R.reference_kwargs(TINY)
    kw["motion_module_kwargs"] = dict(kw["motion_module_kwargs"], zero_initialize=True)
    sd = weights("tiny")
    m = UNet3DConditionModel(**kw)
    m.load_state_dict({k: v for k, v in sd.items() if ".motion_modules." not in k}, strict=False)
    m = m.half().cuda()
    two_d = mirror("nomotion", {k: v for k, v in sd.items() if ".motion_modules." not in k})
    before = m(x, 481, txt).sample
    assert torch.equal(before, two_d(x, 481, txt).sample)
    missing, unexpected = m.load_state_dict({k: v for k, v in sd.items() if ".motion_modules." in k}, strict=False)
    assert not unexpected and all(".motion_modules." not in k for k in missing)
    after = m(x, 481, txt).sample
    assert not torch.equal(after, before) and torch.equal(after, model("tiny")(x, 481, txt).sample)


def raw_handle(name):
    """the C ABI without the mirror: the same tensors under the same names"""
    from univst_amd import _native
    cfg, lib = CFGS[name], _native.load()
    hd = cfg["attention_head_dim"]
    uc = _native.UnetCfg(4, 4, (C.c_int * 4)(*cfg["block_out_channels"]), cfg["layers_per_block"], cfg["cross_attention_dim"],
                         (C.c_int * 4)(*((hd,) * 4 if isinstance(hd, int) else hd)), cfg["norm_num_groups"], cfg["norm_eps"], 1, 0.0)
    mask = sum(1 << i for i in range(4) if cfg["motion_levels"][i])
    ad = _native.AnimateDiffCfg(int(cfg["use_inflated_groupnorm"]), mask, int(cfg["motion_mid_block"]),
                                _native.MotionCfg(0, cfg["motion_heads"], cfg["motion_blocks"], cfg["motion_attn"], 32, cfg["max_len"], 1, 1e-6, 1e-5))
    h = C.c_void_p()
    _native.check(lib.univst_unet_create_animatediff(C.byref(uc), C.byref(ad), C.byref(h)), "create")
    for k, v in weights(name).items():
        t = v.cuda().contiguous()
        _native.check(lib.univst_unet_load_tensor(h, k.encode(), t.data_ptr(), 1, (C.c_int64 * t.dim())(*t.shape), t.dim(), _native.stream_ptr()), k)
        torch.cuda.synchronize()
    _native.check(lib.univst_unet_finalize(h, _native.stream_ptr()), "finalize")
    return h


def test_mirror_equals_the_handle_and_the_handle_refuses():
    from univst_amd import _native
    lib = _native.load()
    x, txt = inputs(1, 3, 16, 16)
    h = raw_handle("tiny")
    try:
        eps = torch.empty_like(x)
        fwd = lambda xx, F, feat=None: lib.univst_unet_forward(h, xx.data_ptr(), 481.0, txt.data_ptr(), 1, F, 16, 16, TEXT_LEN, None, eps.data_ptr(), feat, -1,  # noqa: E731
                                                               _native.stream_ptr())
        _native.check(fwd(x, 3), "forward")
        assert torch.equal(eps, model("tiny")(x, 481, txt).sample)
        keep = eps.clone()
        feat = torch.zeros(64, device="cuda", dtype=torch.float16)
        assert fwd(x, 3, feat.data_ptr()) == -1 and "feat_out" in lib.univst_last_error().decode()
        x33 = torch.zeros(1, 4, 33, 16, 16, device="cuda", dtype=torch.float16)
        assert fwd(x33, 33) == -1 and "F=33" in lib.univst_last_error().decode()
        x25 = torch.zeros(1, 4, 25, 16, 16, device="cuda", dtype=torch.float16)
        assert fwd(x25, 25) == -1 and "max_len" in lib.univst_last_error().decode()
        ws = torch.zeros(1 << 18, device="cuda", dtype=torch.uint8)
        assert lib.univst_unet_set_comm(h, 0, 2, ws.data_ptr(), ws.numel(), _native.ALLREDUCE_FN(lambda *a: 0), _native.KVEXCHANGE_FN(lambda *a: 0), None) == -3
        torch.cuda.synchronize()
        assert torch.equal(eps, keep) and (feat == 0).all(), "a refusal comes before any launch"
    finally:
        lib.univst_unet_destroy(h)


def test_second_forward_is_deterministic_and_allocates_nothing():
    """the motion chains run on the UNet's arena: a second forward at the same size leaves the slab and its high-water mark alone and returns the
    same bits (the unfolded chain has no atomics in its reductions)"""
    x, txt = inputs(1, 3, 16, 16)
    m = model("tiny")
    a = m(x, 481, txt).sample
    hw, size = m.native_query("arena_high_water"), m.native_query("arena_bytes")
    b = m(x, 481, txt).sample
    assert torch.equal(a, b)
    assert hw > 0 and m.native_query("arena_high_water") == hw and m.native_query("arena_bytes") == size
    assert m.native_query("weight_bytes") > 0 and size >= hw      # the read-outs every handle answers
    with pytest.raises(RuntimeError, match="not built"):
        m.set_native_option("motion_fold", 1)
    assert "motion_fold" not in getattr(m, "_native_options", {}), "a refused value is not recorded: the next rebuild would raise on it"
    m.set_native_option("motion_fold", 0)
    assert m._native_options == {"motion_fold": 0} and torch.equal(m(x, 481, txt).sample, a)
    m._native_options.clear()


def test_forward_refuses_what_the_reference_does_not_take():
    x, txt = inputs(1, 3, 16, 16)
    m = model("tiny")
    with pytest.raises(TypeError, match="down_block_additional_residuals"):
        m(x, 481, txt, down_block_additional_residuals=[x])
    with pytest.raises(NotImplementedError, match="per-sample timesteps"):
        m(torch.cat([x, x]), torch.tensor([481, 480]), torch.cat([txt, txt]))
    x2, txt2 = torch.cat([x, x]), torch.cat([txt, txt])
    assert torch.equal(m(x2, torch.tensor([481, 481]), txt2).sample, m(x2, 481, txt2).sample), "equal per-sample values are the one timestep"


def plan(kind, *args):
    from univst_amd import _native
    buf = C.create_string_buffer(4096)
    fn = getattr(_native.load(), f"univst_debug_{kind}_plan")
    assert fn(*args, buf, 4096) == 0, _native.load().univst_last_error().decode()
    return buf.value.decode()


def test_full_size_level_inside_the_pnp_window():
    """The kernels a full-size step runs, against the restatement: C = 320 with 8 heads at 64x64 latents, B = 3, F = 4 — 49 152 rows (192 tiles of
    256 rows: the 256x320 GEMM path with its GroupNorm-statistics epilogue, the LDS-patch convs, kcat_fold without a temporal bias), 4 096 tokens per
    frame (the software-pipelined d = 40 self-attention with ONE key source and no count / weight tables), per-frame resnet GroupNorms fed by
    producer statistics over two concat sources, the motion chains on those GEMMs over the UNet's workspace, and the AdaIN shift in front of the
    attention.  The host-side plans say which kernels the shapes of this level take; the bound is the file's."""
    from univst_amd import _native
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    rows = 3 * 4 * 4096
    assert plan("attention", 12, 8, 4096, 4096, 1, 40, 1, 0, 0).startswith("attn_pp40_kernel<0,1,true,0> ")
    for N, K, geglu in ((320, 320, 0), (960, 320, 0), (320, 1280, 0)):          # proj_in / to_out / proj_out, q|k|v, ff.net.2: the spatial block's and the module's
        assert plan("gemm", ncu, 0, rows, N, K, geglu, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0).startswith("gemm_big_kernel<"), (N, K)
    gn = (C.c_int * 16)()
    assert _native.load().univst_debug_groupnorm_plan(320, 320, rows, 4096, 32, 0, 1, 1, gn) == 0 and gn[0] == 2, "per-frame norm1 over [x | skip]: producer statistics"
    shape = (3, 4, 64, 64)
    x, txt = inputs(*shape)
    m = model("sd_level")
    U = R.U
    U.SDPA_MAX_BATCH, keep = 1, U.SDPA_MAX_BATCH          # (an fp64 SDPA over all 12 frames at once would hold 13 GB of scores)
    try:
        r64, r16 = refs("sd_level", shape, 10)
    finally:
        U.SDPA_MAX_BATCH = keep
    register(m, 10)
    try:
        got = m(x, 481, txt).sample
    finally:
        unregister(m)
    within_bound("sd_level (3, 4, 64, 64) pnp idx 10", got, r64, r16)
    stock = m(x, 481, txt).sample
    assert torch.equal(got[:2], stock[:2]) and not torch.equal(got[2], stock[2])
