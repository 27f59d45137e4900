"""GPU: the native AnimateDiff motion module (univst_amd/motion.py, csrc/motion.hip) against the restatement tests/motion_ref.py (held to the
reference by tests/test_motion_ref.py): the frame-axis attention operator against an fp64 softmax with a derived bound, exact-data checks of its lane
maps, memory that must never reach an output, its refusals; the whole module against the fp64 restatement with the torch-fp16 restatement's own
error as the yardstick, the 5-D call, the mirror and the arena."""
import os
import sys
import types

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import motion_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu
EPS16 = 2.0 ** -11          # unit roundoff of fp16
HEADS = 8


# ------------------------------------------------------------------------------------------------------------ the attention operator
def make_qkv(rows, heads, d, seed):
    """the recipe of tests/test_gpu_clip.py::make_qkv at head dim d: q | k | v rows [rows, 3*heads*d] fp16; q carries the folded scale, so the scores
    ARE q.k: sigma_q sigma_k sqrt(d) = 3"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(rows, 3, heads * d, generator=g)
    qkv[:, :2] *= (3.0 / d ** 0.5) ** 0.5
    return qkv.reshape(rows, 3 * heads * d).half()


def add_pe(qkv, pe, B, F, N):
    """what the kernel adds as it loads a row of frame f: pe[f], the sum rounded to fp16 once (the fp32 sum of two fp16 numbers that are within 2^13 of
    each other is exact, and a smaller one cannot reach a tie)"""
    return (qkv.view(B, F, N, -1).float() + pe.view(1, F, 1, -1).float()).half().view(B * F * N, -1)


def attention_ref64(qkv, B, F, N, heads, d):
    """fp64 softmax attention over the F frames of each (b, n, head) on the same fp16 inputs -> (o [B*F*N, heads*d], vmax = max_f |v[f, c]|, scores)"""
    x = qkv.double().view(B, F, N, 3, heads, d).permute(3, 0, 2, 4, 1, 5)      # [3][B][N][heads][F][d]
    q, k, v = x[0], x[1], x[2]
    sc = q @ k.transpose(-1, -2)
    o = torch.softmax(sc, dim=-1) @ v
    back = lambda t: t.permute(0, 3, 1, 2, 4).reshape(B * F * N, heads * d)      # noqa: E731
    return back(o), back(v.abs().amax(dim=3, keepdim=True).expand_as(v)), sc


def check_against_fp64(qkv_rows, pe, B, F, N, d, got, tag):
    eff = add_pe(qkv_rows, pe, B, F, N) if pe is not None else qkv_rows
    want, vmax, sc = attention_ref64(eff, B, F, N, HEADS, d)
    frac = ((got.double() - want).abs() / (4 * EPS16 * vmax).clamp(min=1e-30)).max().item()
    std = f", score std {sc.std().item():.2f}" if F > 1 else ""
    print(f"{tag}: worst |o - o64| / bound = {frac:.3f}{std}")
    assert torch.isfinite(got).all() and frac <= 1.0


@pytest.mark.parametrize("with_pe", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("N", [5, 70])
@pytest.mark.parametrize("F", [1, 2, 8, 15, 16, 17, 24, 32])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_attention_operator(d, F, N, B, with_pe):
    """every output element is a convex combination of the F value rows, so |o - o64| <= 4 x 2^-11 x max_f |v_f| elementwise: one unit roundoff each
    for the fp16 rounding of P, the fp16 rounding of the output and the exp2 / fp32 accumulation error, and one spare (the bound of
    tests/test_gpu_clip.py::test_attention_operator); v is taken after the position add and its rounding"""
    from univst_amd import _native
    qkv = make_qkv(B * F * N, HEADS, d, seed=d * 1000 + F * 10 + N + B).cuda()
    pe = (0.5 * torch.randn(F, 3 * HEADS * d, generator=torch.Generator().manual_seed(F))).half().cuda() if with_pe else None
    got = _native.temporal_attention(qkv, B, F, N, HEADS, d, pe_qkv=pe)
    check_against_fp64(qkv, pe, B, F, N, d, got, f"d={d} F={F} N={N} B={B} pe={int(with_pe)}")


def test_attention_operator_with_leading_dimensions():
    """ldx > 3C and ldo > C: the pad columns are neither read nor written"""
    from univst_amd import _native
    d, B, F, N = 80, 2, 17, 9
    Cw = HEADS * d
    qkv = make_qkv(B * F * N, HEADS, d, seed=3).cuda()
    wide = torch.full((B * F * N, 3 * Cw + 24), float("nan"), device="cuda", dtype=torch.float16)
    wide[:, :3 * Cw] = qkv
    out = torch.full((B * F * N, Cw + 12), -7.0, device="cuda", dtype=torch.float16)
    _native.temporal_attention(wide[:, :3 * Cw], B, F, N, HEADS, d, out=out[:, :Cw])
    assert (out[:, Cw:] == -7.0).all()
    check_against_fp64(qkv, None, B, F, N, d, out[:, :Cw], "ldx = 3C + 24, ldo = C + 12")


def test_attention_operator_on_a_grid_of_many_rounds():
    """d = 40, B = 1, F = 8, N = 4096: 32 768 (pixel, head) problems, at most 8 to a block, so the launch has several times more blocks than the
    device can hold at once (a fault of an earlier kernel of this library showed on such grids only)"""
    from univst_amd import _native
    d, B, F, N = 40, 1, 8, 4096
    assert N * HEADS // 8 > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    qkv = make_qkv(B * F * N, HEADS, d, seed=11).cuda()
    got = _native.temporal_attention(qkv, B, F, N, HEADS, d)
    check_against_fp64(qkv, None, B, F, N, d, got, "d=40 F=8 N=4096")


@pytest.mark.parametrize("F", [16, 32])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_exact_data_orientation(d, F):
    """integer data on which every step is exact.  (a) identical key rows: q.k is the same for all keys, the softmax is uniform and the output is the
    exact mean over the frames of v[f][c] = f + 32 (c mod 7) (asymmetric in frame and column).  (b) one-hot rows: q_f = 16 e_{p(f)}, k_f' = 16 e_f'
    with p(f) = 3f + 1 mod F (a permutation that is not its own inverse): the score is 256 on key p(f) and 0 elsewhere, exp underflows to an exact 0
    and the output of query f is the row v[p(f)] — a swap of the query and key roles, or a wrong key order in either product, moves rows."""
    from univst_amd import _native
    B, N, Cw = 2, 3, HEADS * d
    c = torch.arange(Cw)
    f = torch.arange(F)
    v = (f[:, None] + 32 * (c[None, :] % 7)).float()                                   # [F, C]
    v = v[None, :, None, :] + torch.tensor([0.0, 1.0])[:, None, None, None] + 2 * torch.arange(N)[None, None, :, None]      # [B, F, N, C]: every (b, n) differs
    g = torch.Generator().manual_seed(d + F)
    # (a)
    q = torch.randint(-2, 3, (B, F, N, Cw), generator=g).float()
    k = torch.randint(-2, 3, (B, 1, N, Cw), generator=g).float().expand(B, F, N, Cw)
    qkv = torch.cat([q, k, v], dim=-1).reshape(B * F * N, 3 * Cw).half().cuda()
    got = _native.temporal_attention(qkv, B, F, N, HEADS, d).view(B, F, N, Cw)
    want = v.mean(dim=1, keepdim=True).expand(B, F, N, Cw).half().cuda()
    assert torch.equal(want.float().cpu(), v.mean(dim=1, keepdim=True).expand(B, F, N, Cw)), "the mean must be representable"
    assert torch.equal(got, want)
    # (b)
    p = (3 * f + 1) % F
    hot = torch.zeros(F, d)
    hot[f, f] = 16.0
    k = hot.repeat(1, HEADS)[None, :, None, :].expand(B, F, N, Cw)
    q = hot[p].repeat(1, HEADS)[None, :, None, :].expand(B, F, N, Cw)
    qkv = torch.cat([q, k, v], dim=-1).reshape(B * F * N, 3 * Cw).half().cuda()
    got = _native.temporal_attention(qkv, B, F, N, HEADS, d).view(B, F, N, Cw)
    assert torch.equal(got, v[:, p].half().cuda())


@pytest.mark.parametrize("F", [15, 17])
@pytest.mark.parametrize("d", [40, 80, 160])
def test_memory_outside_the_rows_never_leaks(d, F):
    """a tail of rows behind row B F N and the pad columns of ldx > 3C, filled with zeros and then with NaN: the output is bit-identical and finite
    (the padding keys F .. 15 / 31 of the kernel's tile and the padding columns of the contraction are made in registers, never read)"""
    from univst_amd import _native
    B, N, Cw = 2, 5, HEADS * d
    rows = B * F * N
    qkv = make_qkv(rows, HEADS, d, seed=F).cuda()
    pe = (0.5 * torch.randn(F, 3 * Cw, generator=torch.Generator().manual_seed(1))).half().cuda()
    outs = []
    for fill in (0.0, float("nan")):
        buf = torch.full((rows + 40 * N, 3 * Cw + 8), fill, device="cuda", dtype=torch.float16)
        buf[:rows, :3 * Cw] = qkv
        outs.append(_native.temporal_attention(buf[:, :3 * Cw], B, F, N, HEADS, d, pe_qkv=pe)[:rows])
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16))


def test_attention_refuses_bad_arguments():
    from univst_amd import _native
    d, N = 40, 4
    Cw = HEADS * d
    buf = torch.zeros(33 * N, 3 * Cw + 4, device="cuda", dtype=torch.float16)
    out = torch.full((33 * N, Cw), -7.0, device="cuda", dtype=torch.float16)
    qkv = buf[:, :3 * Cw].contiguous()
    for F, dd, src, word in ((0, d, qkv, "F=0"), (33, d, qkv, "F=33"), (8, 64, torch.zeros(33 * N, 3 * HEADS * 64, device="cuda", dtype=torch.float16), "head_dim=64"),
                             (8, d, buf[:, :3 * Cw], "ldx=")):
        with pytest.raises(RuntimeError, match=word):
            _native.temporal_attention(src, 1, F, N, HEADS, dd, out=out if dd == d else None)
    torch.cuda.synchronize()
    assert (out == -7.0).all(), "a refusal comes before any launch"


# ------------------------------------------------------------------------------------------------------------ the module
SHAPES = {"F16_4x4": (2, 16, 4, 4), "F7_3x5": (2, 7, 3, 5)}
_CASES = {}


def case(Cw):
    """per width: seeded weights (non-zero proj_out), the native module, and per shape the input with its fp64 / fp16 restatement outputs (computed once)"""
    if Cw not in _CASES:
        from univst_amd.motion import NativeMotionModule
        cfg = R.Cfg(channels=Cw, num_heads=HEADS, num_blocks=1, attn_per_block=2, max_len=24)
        sd = R.random_state_dict(cfg, seed=Cw)
        conf = dict(num_attention_heads=HEADS, num_transformer_block=1, temporal_position_encoding=True, temporal_position_encoding_max_len=24)
        c = types.SimpleNamespace(cfg=cfg, sd=sd, conf=conf, mod=NativeMotionModule(sd, config=conf), x={}, ref64={}, ref16={})
        for name, (B, F, H, W) in SHAPES.items():
            x = torch.randn(B, Cw, F, H, W, generator=torch.Generator().manual_seed(F)).half().cuda()
            with torch.no_grad():
                c.x[name], c.ref64[name], c.ref16[name] = x, R.forward(sd, cfg, x, torch.float64), R.forward(sd, cfg, x, torch.float16)
        _CASES[Cw] = c
    return _CASES[Cw]


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("Cw", [320, 640, 1280])
def test_module_against_fp64_restatement(Cw, shape):
    """yardstick (that of tests/test_gpu_clip.py::test_encoder_against_fp64_restatement): the reference runs this module in torch fp16 on this GPU,
    i.e. the restatement in fp16, whose distance to the fp64 restatement is e_ref.  The native module must be finite and within 2 x e_ref in the
    maximum norm (the factor covers a different but equally valid accumulation order and the projected position rows)."""
    c = case(Cw)
    got = c.mod(c.x[shape])
    r64, r16 = c.ref64[shape], c.ref16[shape]
    assert got.shape == r64.shape and got.dtype == torch.float16
    e_nat, e_ref = (got.double() - r64).abs().max().item(), (r16.double() - r64).abs().max().item()
    print(f"C={Cw} {shape}: e_native {e_nat:.3e}, e_ref (torch fp16) {e_ref:.3e}, ratio {e_nat / e_ref:.2f}, max|want| {r64.abs().max().item():.2f}, "
          f"max|want - x| {(r64 - c.x[shape].double()).abs().max().item():.2f}")
    assert torch.isfinite(got).all() and e_nat <= 2 * e_ref


def test_five_d_call_equals_forward_rows():
    c = case(320)
    x = c.x["F7_3x5"]
    B, Cw, F, H, W = x.shape
    rows = x.permute(0, 2, 3, 4, 1).reshape(B * F * H * W, Cw).contiguous()
    y_rows = c.mod.forward_rows(rows, B, F, H * W)
    assert y_rows.shape == rows.shape
    assert torch.equal(c.mod(x, None, encoder_hidden_states=None), y_rows.view(B, F, H, W, Cw).permute(0, 4, 1, 2, 3))


def test_mirror_equals_the_native_module():
    """the reference's import path: a state dict loaded strict=True, .half().cuda(), called as the UNet calls it"""
    from backbones.animatediff.models.motion_module import VanillaTemporalModule
    c = case(320)
    m = VanillaTemporalModule(in_channels=320, num_attention_heads=HEADS, num_transformer_block=1, temporal_position_encoding=True,
                              temporal_position_encoding_max_len=24, zero_initialize=False)
    m.load_state_dict(c.sd, strict=True)
    m = m.half().cuda()
    x = c.x["F16_4x4"]
    y = m(x, None, encoder_hidden_states=None)
    assert torch.equal(y, c.mod(x))
    handle = m._native
    assert m(x, None, None) is not None and m._native is handle, "unchanged parameters keep the handle"
    with torch.no_grad():
        m.temporal_transformer.proj_out.weight.mul_(0.5)
    y2 = m(x, None, None)
    assert m._native is not handle and not torch.equal(y2, y), "edited parameters rebuild the handle"


def test_zero_initialised_mirror_returns_its_input():
    from backbones.animatediff.models.motion_module import VanillaTemporalModule
    m = VanillaTemporalModule(in_channels=640, num_attention_heads=HEADS, num_transformer_block=1, temporal_position_encoding=True,
                              zero_initialize=True).half().cuda()
    x = case(640).x["F7_3x5"]
    assert torch.equal(m(x, None, None), x)


def test_arena_is_sized_once_per_shape():
    c = case(320)
    xa, xb = c.x["F16_4x4"], c.x["F7_3x5"]
    ya = c.mod(xa)
    hw = c.mod.query("arena_high_water")
    assert hw > 0 and c.mod.query("weight_bytes") > 2 * 12 * 320 * 320
    assert torch.equal(c.mod(xa), ya) and c.mod.query("arena_high_water") == hw
    c.mod(xb)
    assert torch.equal(c.mod(xa), ya)


def test_finalize_names_a_tensor_whose_shape_the_config_does_not_give():
    """ff.net.2.weight [C, 4C] given as [C, 2C] at C = 320: finalize names the key and says what is wrong with it"""
    from univst_amd.motion import NativeMotionModule
    c = case(320)
    sd = dict(c.sd)
    key = "temporal_transformer.transformer_blocks.0.ff.net.2.weight"
    assert tuple(sd[key].shape) == (320, 1280)
    sd[key] = sd[key][:, :640].contiguous()
    with pytest.raises(RuntimeError, match="which the config does not give") as e:
        NativeMotionModule(sd, config=c.conf)
    assert key in str(e.value)


def test_shared_readouts():
    """the read-outs every handle answers: the weights are counted and the slab holds the high-water mark"""
    c = case(320)
    c.mod(c.x["F7_3x5"])
    assert c.mod.query("weight_bytes") > 0 and c.mod.query("arena_bytes") >= c.mod.query("arena_high_water") > 0


def test_more_frames_than_the_position_table_are_refused():
    from univst_amd import _native
    c = case(320)
    x = torch.zeros(1, 320, 25, 2, 2, device="cuda", dtype=torch.float16)
    with pytest.raises(ValueError, match="temporal_position_encoding_max_len"):
        c.mod(x)
    rows = torch.zeros(25 * 4, 320, device="cuda", dtype=torch.float16)
    rc = _native.load().univst_motion_forward(c.mod._h, _native.ptr(rows), _native.ptr(torch.empty_like(rows)), 1, 25, 4, _native.stream_ptr())
    assert rc == -1 and "max_len" in _native.load().univst_last_error().decode()
    with pytest.raises(TypeError, match="fp16"):
        c.mod(x.float())
    with pytest.raises(RuntimeError, match="GPU only"):
        c.mod(x.cpu())


def test_without_position_encoding_the_table_length_does_not_bound_the_frames():
    """temporal_position_encoding off: no pe[:, :F] add exists, so F = 25 > max_len = 24 runs (the reference accepts it too); same yardstick as the
    module test; F = 33 is beyond the attention kernel"""
    from univst_amd.motion import NativeMotionModule
    cfg = R.Cfg(channels=320, num_heads=HEADS, num_blocks=1, attn_per_block=2, max_len=24, position_encoding=False)
    sd = R.random_state_dict(cfg, seed=5)
    mod = NativeMotionModule(sd, config=dict(num_attention_heads=HEADS, num_transformer_block=1, temporal_position_encoding=False,
                                             temporal_position_encoding_max_len=24))
    x = torch.randn(1, 320, 25, 2, 3, generator=torch.Generator().manual_seed(25)).half().cuda()
    with torch.no_grad():
        r64, r16 = R.forward(sd, cfg, x, torch.float64), R.forward(sd, cfg, x, torch.float16)
    got = mod(x)
    e_nat, e_ref = (got.double() - r64).abs().max().item(), (r16.double() - r64).abs().max().item()
    print(f"no position encoding, F=25: e_native {e_nat:.3e}, e_ref (torch fp16) {e_ref:.3e}, ratio {e_nat / e_ref:.2f}")
    assert torch.isfinite(got).all() and e_nat <= 2 * e_ref
    with pytest.raises(ValueError, match="at most 32"):
        mod(torch.zeros(1, 320, 33, 2, 2, device="cuda", dtype=torch.float16))
