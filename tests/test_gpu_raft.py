"""GPU: the native RAFT-large (univst_amd/flow.py, csrc/raft.hip) against the fp32 restatement of torchvision's definition (tests/raft_ref.py):
every stage on seeded inputs, then the whole estimator with random weights whose flow head is scaled so that the 1/8-resolution flow is 1 - 4 px
(lookups leave the centre and cross the volume border; checked on the restatement below), then the call sites."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raft_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
EPS32, EPS16 = 2.0 ** -24, 2.0 ** -11          # unit roundoffs
SHAPES = [(128, 128), (136, 200)]


@pytest.fixture(scope="module")
def sd():
    return R.random_state_dict(0, 1.0, 6.0)


@pytest.fixture(scope="module")
def ref32(sd):
    m = R.RAFT().eval()
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def ref16(sd):
    m = R.RAFT(round_fp16=True).eval()
    m.load_state_dict(sd, strict=True)
    return m


@pytest.fixture(scope="module")
def native(sd):
    from univst_amd.flow import NativeRAFT
    return NativeRAFT.from_state_dict(sd)


_E2E = {}


def e2e(shape, ref32, ref16):
    """restatement results of one shape, computed once: images, fp32 flow, D_ref, low-resolution flow range"""
    if shape not in _E2E:
        a, b = R.make_images(*shape)
        f32 = ref32(R.preprocess(a), R.preprocess(b))[-1][0].permute(1, 2, 0).contiguous()
        lo = ref32.last_lowres_flow.norm(dim=1)
        f16 = ref16(R.preprocess(a), R.preprocess(b))[-1][0].permute(1, 2, 0)
        _E2E[shape] = dict(a=a, b=b, f32=f32, d_ref=(f32 - f16).norm(dim=-1).max().item(), lo=(lo.min().item(), lo.max().item()))
    return _E2E[shape]


def nhwc(t):        # [1, C, h, w] -> [h*w, C]
    return t[0].permute(1, 2, 0).reshape(-1, t.shape[1])


# ------------------------------------------------------------------------------------------------------------ stages
@pytest.mark.parametrize("fh,fw", [(16, 16), (17, 25), (24, 32)])
def test_correlation_pyramid(fh, fw):
    """fp32 work: bound = 2 x (256 eps32 max|a| max|b|) / 16 — the accumulation-order bound of a 256-term fp32 dot product, scaled like the volume"""
    from univst_amd import flow
    g = torch.Generator().manual_seed(fh * 100 + fw)
    f1, f2 = torch.randn(fh * fw, 256, generator=g).half(), torch.randn(fh * fw, 256, generator=g).half()
    _, lv = flow.corr_pyramid(f1.cuda(), f2.cuda(), fh, fw)
    to4 = lambda f: f.float().t().reshape(1, 256, fh, fw)
    want = R.build_pyramid(to4(f1), to4(f2))
    tol = 2 * 256 * EPS32 * f1.float().abs().max().item() * f2.float().abs().max().item() / 16
    for l in range(4):
        assert tuple(lv[l].shape) == (fh * fw, fh >> l, fw >> l)
        err = (lv[l].cpu() - want[l][:, 0]).abs().max().item()
        print(f"corr level {l} {fh}x{fw}: max err {err:.3e} (tol {tol:.3e})")
        assert err <= tol


def _lookup_coords(fh, fw, seed):
    g = torch.Generator().manual_seed(seed)
    c = R.make_coords_grid(1, fh, fw)[0].permute(1, 2, 0).reshape(-1, 2).clone()        # exact integers
    n = c.shape[0]
    k = n // 8
    c[k:2 * k] += torch.rand(k, 2, generator=g) * 6 - 3                                 # fractional flows of a few px
    c[2 * k:3 * k, 0] = fw - 1                                                          # last column
    c[3 * k:4 * k, 1] = fh - 1                                                          # last row
    c[4 * k:4 * k + 8] = torch.tensor([[-6.5, 3.0], [fw + 5.25, 3.0], [3.0, -7.75], [3.0, fh + 4.5], [-9.0, -9.0], [fw + 8.0, fh + 8.0], [-40.0, 2.0], [2.0, 90.0]])
    c[5 * k:6 * k] = -torch.rand(k, 2, generator=g) * 3                                 # negative fractions
    c[6 * k:7 * k] = torch.rand(k, 2, generator=g) * torch.tensor([fw + 10.0, fh + 10.0]) - 5
    return c


@pytest.mark.parametrize("fh,fw", [(16, 16), (17, 25), (24, 32)])
def test_pyramid_lookup(fh, fw):
    """held on the NATIVE pyramid (identical inputs).  Bound: 8 eps32 M for the bilinear arithmetic (3 products and 3 sums of values <= M) plus the
    restatement's own coordinate error: torchvision maps x -> 2x/(w-1) - 1 and grid_sample maps it back, 4 roundings at magnitude X = max(|x| + 4, h, w),
    i.e. 4 eps32 X px in x and in y, each moving a bilinear sample by at most 2 M per px."""
    from univst_amd import flow
    g = torch.Generator().manual_seed(7)
    f1, f2 = torch.randn(fh * fw, 256, generator=g).half(), torch.randn(fh * fw, 256, generator=g).half()
    buf, lv = flow.corr_pyramid(f1.cuda(), f2.cuda(), fh, fw)
    c = _lookup_coords(fh, fw, 11)
    o32, o16 = flow.corr_lookup(buf, c.cuda(), fh, fw, want_f16=True)
    want = nhwc(R.index_pyramid([v.cpu()[:, None] for v in lv], c.reshape(1, fh, fw, 2).permute(0, 3, 1, 2)))
    M = lv[0].abs().max().item()
    X = max(c.abs().max().item() + 4, fh, fw)
    tol = 8 * EPS32 * M + 2 * (2 * M) * (4 * EPS32 * X)
    err = (o32.cpu() - want).abs().max().item()
    print(f"lookup {fh}x{fw}: max err {err:.3e} (tol {tol:.3e}, max |corr| {M:.2f})")
    assert err <= tol
    assert (want.abs().sum(dim=1) == 0).any() and (want[:, 324 - 81:].abs().sum(dim=1) > 0).any()
    assert torch.equal(o16[:, :324], o32.half()) and o16[:, 324:].abs().max().item() == 0


@pytest.mark.parametrize("fh,fw", [(16, 16), (17, 25)])
def test_convex_upsample(fh, fw):
    """fp32 softmax rounding: weights carry ~4 eps32 (exp of a rounded difference, the 9-term sum, the division), 9 terms -> 16 eps32 x max|8 flow|"""
    from univst_amd import flow
    g = torch.Generator().manual_seed(5)
    fl = torch.randn(fh, fw, 2, generator=g) * 3
    mask = (torch.randn(fh * fw, 576, generator=g) * 4).half()
    got = flow.convex_upsample(fl.cuda(), mask.cuda(), fh, fw).cpu()
    want = R.upsample_flow(fl.permute(2, 0, 1)[None], 0.25 * mask.float().t().reshape(1, 576, fh, fw))[0].permute(1, 2, 0)
    tol = 16 * EPS32 * 8 * fl.abs().max().item()
    err = (got - want).abs().max().item()
    print(f"upsample {fh}x{fw}: max err {err:.3e} (tol {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("fh,fw", [(16, 16), (17, 25)])
def test_gru_step(native, ref16, fh, fw):
    """against the round_fp16 restatement.  Both round every conv output to fp16; where the fp32 accumulation order differs a pre-activation may land
    on the neighbouring fp16 value.  With P the largest pre-activation of the block's six convs in the restatement, neighbouring fp16 values are
    u = 2^(floor(log2 max(P, 1)) - 10) apart.  r feeds q, so a ConvGRU carries at most two such flips through gates of slope <= 1 with |h| <= 1, and the
    block has two ConvGRUs: 4 u."""
    import math
    g = torch.Generator().manual_seed(fh)
    n = fh * fw
    hid = torch.tanh(torch.randn(n, 128, generator=g))
    ctx, mot = torch.rand(n, 128, generator=g).half(), torch.randn(n, 128, generator=g).half()
    got = native.gru(hid.cuda(), ctx.cuda(), mot.cuda(), fh, fw).cpu()
    to4 = lambda t: t.float().t().reshape(1, 128, fh, fw)
    rb, pre = ref16.update_block.recurrent_block, []
    hooks = [m.register_forward_hook(lambda _m, _i, o: pre.append(o.abs().max().item())) for m in rb.modules() if isinstance(m, R.Conv)]
    with torch.no_grad():
        want = nhwc(R.gru(rb, to4(hid), to4(ctx), to4(mot)))
    for h in hooks:
        h.remove()
    assert len(pre) == 6
    tol = 4 * 2.0 ** (math.floor(math.log2(max(max(pre), 1.0))) - 10)
    err = (got - want).abs().max().item()
    print(f"gru {fh}x{fw}: max err {err:.3e} (tol {tol:.3e}, largest pre-activation {max(pre):.3f})")
    assert err <= tol


@pytest.mark.parametrize("shape", SHAPES)
def test_encoders(native, ref32, ref16, shape):
    """against the round_fp16 restatement: 15 convs in sequence (+ the BatchNorm fold's rounding of w * scale in the context encoder), each output rounded
    to fp16 (unit roundoff 2^-11) on possibly the neighbouring value -> 32 x 2^-11 of the largest activation"""
    d = e2e(shape, ref32, ref16)
    fmap, hid, ctx = native.encode(d["a"].cuda(), d["b"].cuda())
    with torch.no_grad():
        f1, f2, h, c = ref16.encode(R.preprocess(d["a"]), R.preprocess(d["b"]))
    for name, got, want in (("fmap1", fmap[0], f1), ("fmap2", fmap[1], f2), ("hidden", hid, h), ("context", ctx, c)):
        want = nhwc(want)
        err, tol = (got.float().cpu() - want).abs().max().item(), 32 * EPS16 * max(1.0, want.abs().max().item())
        print(f"encoder {shape} {name}: max err {err:.3e} (tol {tol:.3e}, max |ref| {want.abs().max().item():.2f})")
        assert err <= tol


def test_pair_images_do_not_share_instance_norm_statistics(native):
    a, b = R.make_images(128, 128, seed=1)
    c = R.make_images(128, 128, seed=2)[1]
    f_ab = native.encode(a.cuda(), b.cuda())[0]
    f_ac = native.encode(a.cuda(), c.cuda())[0]
    assert torch.equal(f_ab[0], f_ac[0]) and not torch.equal(f_ab[1], f_ac[1])


# ------------------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("shape", SHAPES)
def test_end_to_end_flow(native, ref32, ref16, shape):
    """native vs the fp32 restatement within 3 D_ref + 0.02 px, D_ref = max endpoint difference between the restatement in fp32 and with round_fp16
    on the same weights and images.  Measured on MI355X: 128 x 128 D_ref 0.0076 px, native error 0.0082 px; 136 x 200 D_ref 0.0106 px, native error
    0.0106 px (also in DESIGN.md, kernel table)."""
    d = e2e(shape, ref32, ref16)
    assert 0.5 <= d["lo"][0] and d["lo"][1] <= 8.0, d["lo"]         # the 1/8-resolution flow range the weights were scaled for
    got = native(d["a"].cuda(), d["b"].cuda())
    assert got.dtype == torch.float32 and tuple(got.shape) == (*shape, 2)
    err = (got.cpu() - d["f32"]).norm(dim=-1).max().item()
    print(f"end to end {shape}: D_ref {d['d_ref']:.4e} px, native error {err:.4e} px, bound {3 * d['d_ref'] + 0.02:.4e} px, low-res |flow| {d['lo']}")
    assert err <= 3 * d["d_ref"] + 0.02


def test_second_call_at_a_size_allocates_nothing(native):
    a, b = (t.cuda() for t in R.make_images(128, 128))
    out = native(a, b)
    torch.cuda.synchronize()
    del out
    t0, free0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
    out = native(b, a)
    torch.cuda.synchronize()
    del out
    assert torch.cuda.memory_allocated() == t0
    assert free0 - torch.cuda.mem_get_info()[0] < (1 << 20)       # the workspace of this size is a few MB: a re-allocation would show


# ------------------------------------------------------------------------------------------------------------ call sites
def _ref_flow_fn(ref32):
    def fn(x, y):
        return ref32(R.preprocess(x.cpu()), R.preprocess(y.cpu()))[-1][0].permute(1, 2, 0).contiguous().cuda()
    return fn


def _assert_frames_agree(got, want, src, bound):
    """a flow difference of `bound` px moves a bilinear sample by at most bound x (largest step between neighbouring pixels) in x and in y; + 1 for
    the truncation to uint8.  Pixels whose occlusion test sits within `bound` of its threshold may flip between the warped and the key frame: <= 1 %."""
    s = src.float()
    G = max((s[:, 1:] - s[:, :-1]).abs().max().item(), (s[1:] - s[:-1]).abs().max().item())
    diff = (got.float() - want.float()).abs()
    frac = (diff > 1 + 2 * bound * G).float().mean().item()
    print(f"call site: max diff {diff.max().item():.0f} levels, {100 * frac:.3f} % beyond {1 + 2 * bound * G:.1f}")
    assert frac <= 0.01


def test_get_warp_with_the_native_flow_fn(sd, native, ref32, ref16):
    from univst_amd.src.cal_optica_flow import get_warp, make_native_flow_fn
    d = e2e((128, 128), ref32, ref16)
    fn = make_native_flow_fn(sd)
    a, b = d["a"].cuda(), d["b"].cuda()
    bound = 3 * d["d_ref"] + 0.02
    assert (fn(a, b).cpu() - d["f32"]).norm(dim=-1).max().item() <= bound
    got, want = get_warp(a, b, flow_fn=fn), get_warp(a, b, flow_fn=_ref_flow_fn(ref32))
    assert got.dtype == torch.uint8 and got.shape == a.shape
    _assert_frames_agree(got.cpu(), want.cpu(), d["b"], bound)


def test_sliding_window_smooth_with_the_native_flow_fn(native, ref32, ref16):
    """4 frames of 128 x 128, window radius 1 (12 flows per pass: the restatement runs them on the CPU)"""
    from univst_amd.src.cal_optica_flow import sliding_window_smooth
    d = e2e((128, 128), ref32, ref16)
    frames = [d["a"], d["b"], R.make_images(128, 128, seed=0, shift=(5, 1))[1], R.make_images(128, 128, seed=0, shift=(6, 3))[1]]
    clip = torch.stack(frames).permute(3, 0, 1, 2)[None].contiguous().cuda()          # [1, 3, F, H, W]
    got = sliding_window_smooth(clip, native, r=1)
    want = sliding_window_smooth(clip, _ref_flow_fn(ref32), r=1)
    assert got.shape == clip.shape and got.dtype == torch.uint8
    for f in range(4):
        _assert_frames_agree(got[0, :, f].permute(1, 2, 0).cpu(), want[0, :, f].permute(1, 2, 0).cpu(), frames[f], 3 * d["d_ref"] + 0.02)


def test_raft_ckpt_flag_parses():
    from univst_amd.src.sd.run_video_style_transfer_sd import parser
    assert parser().parse_args([]).raft_ckpt == ""
    assert parser().parse_args(["--smoother", "pixel", "--raft_ckpt", "/w/raft_large.pth"]).raft_ckpt == "/w/raft_large.pth"


def test_from_file_reads_pth_and_safetensors(sd, native, tmp_path):
    from univst_amd.flow import NativeRAFT
    a, b = (t.cuda() for t in R.make_images(128, 128))
    want = native(a, b)
    torch.save(sd, tmp_path / "raft.pth")
    assert torch.equal(NativeRAFT.from_file(str(tmp_path / "raft.pth"))(a, b), want)
    st = pytest.importorskip("safetensors.torch")
    st.save_file({k: v.contiguous() for k, v in sd.items()}, str(tmp_path / "raft.safetensors"))
    assert torch.equal(NativeRAFT.from_file(str(tmp_path / "raft.safetensors"))(a, b), want)


def test_native_raft_fails_loudly(native):
    a = torch.zeros(128, 128, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="runs on the GPU only"):
        native(a, a)
    with pytest.raises(ValueError, match=r"input image H and W should be divisible by 8, but got 132 \(h\) and 128 \(w\)"):
        native(torch.zeros(132, 128, 3, dtype=torch.uint8).cuda(), torch.zeros(132, 128, 3, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError, match="Feature maps are too small"):
        native(torch.zeros(120, 128, 3, dtype=torch.uint8).cuda(), torch.zeros(120, 128, 3, dtype=torch.uint8).cuda())
    from univst_amd.flow import NativeRAFT
    with pytest.raises(RuntimeError, match="was never loaded"):
        NativeRAFT.from_state_dict({})(a.cuda(), a.cuda())
