"""GPU: the static style branch of the SD3 / SD3.5 path and the dead-branch skip.

The style input is ONE image.  F identical style frames give every frame the key set [own image keys x 3 ++ own text keys] — the joint attention at
B = 1, clip_length = 1 — and the stylised branch reads nothing of the style branch but its post-norm K | V image rows.  So every comparison below is
against the THREE-branch computation with the style frame repeated F times: the float64 shift (oracle/adain_ref.sd3_shift_ref), the fp32 joint
attention and MM-DiT restatements (oracle/sd3_ref) and the reference-pinned transfer loop (sd3_ref.sd3_transfer_loop).

Bounds are those of the three-branch tests, unchanged: ac.shift_bound per element for the shift (the static kernel runs the same row arithmetic on the
same statistics: colstats over the N style rows, once instead of F times); 4e-3 / 1e-3 (max / rms of the output scale) for the op, 1e-2 / 4e-3 for the
model against fp32, 6e-3 / 1.5e-3 where only summation orders differ, 6e-3 / 2e-3 for the 50-step loops and 5e-3 / 2e-3 for a ten-step inversion
(tests/test_gpu_sd3.py, tests/test_gpu_adain.py).  Every test prints its figures (pytest -s) before it asserts."""
import ctypes as C
import types
from functools import lru_cache

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import adain_cases as ac  # noqa: E402
from oracle import adain_ref as ar  # noqa: E402
from oracle import sd3_ref  # noqa: E402


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def errs(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    e = got - ref
    return e.abs().max().item() / ref.abs().max().item(), (e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


raw = lambda t: t.view(torch.int16)          # noqa: E731  (bit comparison: NaN pads compare equal to themselves)


# ------------------------------------------------------------------------------------------------ a. the shift against float64
STATIC_SHIFT_CASES = ["s1_smallest", "s2_two_stats_blocks", "s3_d8_idle_lanes", "s5_ragged_rows_partial_cols", "sv_mean800"]
LD_PAD, LD_STYLE_PAD, TAIL_ROWS = 24, 16, 40


@lru_cache(maxsize=2)
def _static_case(name):
    """the three-branch case with its style branch overwritten by frame 0 repeated F times, the float64 reference of THAT buffer, and the
    static entry's operands: the two-branch buffer [content | stylised] and the one-frame bank [N, 2C]"""
    b = ac.build_shift(name)
    c = b.case
    FN = c.F * c.N
    qkv = b.qkv.clone()
    qkv[FN:2 * FN] = qkv[FN:FN + c.N].repeat(c.F, 1)
    ref = ar.sd3_shift_ref(qkv, c.F, c.N, c.C, c.heads, ac.SD3_ALPHA, ac.BETA, ac.SD3_GAMMA)
    b3 = types.SimpleNamespace(case=c, qkv=qkv, ref=ref, sd3=True)
    two = torch.cat([qkv[:FN], qkv[2 * FN:]]).contiguous()
    bank = qkv[FN:FN + c.N, c.C:].contiguous()
    return b3, two, bank, ac.shift_bound(b3)


@pytest.mark.parametrize("name", STATIC_SHIFT_CASES)
def test_static_shift_case_against_float64(nat, name):
    """dense and with padded strides (ld = 3C + 24, ld_style = 2C + 16, NaN pads and 40 NaN rows behind both buffers): every stylised element
    within the three-branch kernel's own bound of the float64 reference; content rows, bank rows, pad columns and tail rows bit-untouched; padded
    == dense, and two runs agree"""
    b3, two, bank, bound = _static_case(name)
    c = b3.case
    F, N, Cc, FN = c.F, c.N, c.C, c.F * c.N
    args = (F, N, Cc, c.heads, ac.SD3_ALPHA, ac.BETA, ac.SD3_GAMMA)
    dense, dbank = two.cuda(), bank.cuda()
    nat.sd3_adain_shift_static_(dense, dbank, *args)
    again = two.cuda()
    nat.sd3_adain_shift_static_(again, bank.cuda(), *args)
    torch.cuda.synchronize()
    assert torch.equal(dense, again), f"{name}: two runs of the same call differ"
    assert torch.equal(raw(dense[:FN].cpu()), raw(two[:FN])), f"{name}: content rows were written"
    assert torch.equal(raw(dbank.cpu()), raw(bank)), f"{name}: the bank was written"
    out = dense[FN:].cpu()
    ref = b3.ref.out[2 * FN:]
    err = (out.double() - ref).abs()
    ratio = err / bound
    worst = int(ratio.argmax())
    row, col = divmod(worst, 3 * Cc)
    msg = (f"{name}: static shift max(err / bound) Q {ratio[:, :Cc].max().item():.3f}  K|V {ratio[:, Cc:].max().item():.3f}; worst at row {row} "
           f"(frame {row // N}, token {row % N}) column {col} ({'qkv'[col // Cc]} {col % Cc}): got {out[row, col].item():.6g}, ref "
           f"{ref[row, col].item():.6g}; max err {err.max().item():.3e}")
    print(msg)
    assert torch.isfinite(out).all() and ratio.max().item() <= 1.0, msg
    # padded strides
    ld, lds = 3 * Cc + LD_PAD, 2 * Cc + LD_STYLE_PAD
    buf = torch.full((2 * FN + TAIL_ROWS, ld), float("nan"), dtype=torch.float16, device="cuda")
    sbuf = torch.full((N + TAIL_ROWS, lds), float("nan"), dtype=torch.float16, device="cuda")
    buf[:2 * FN, :3 * Cc] = two.cuda()
    sbuf[:N, :2 * Cc] = bank.cuda()
    before, sbefore = buf.clone(), sbuf.clone()
    view, sview = buf[:2 * FN, :3 * Cc], sbuf[:N, :2 * Cc]
    assert view.stride() == (ld, 1) and sview.stride() == (lds, 1)
    nat.sd3_adain_shift_static_(view, sview, *args)
    torch.cuda.synchronize()
    assert torch.equal(view, dense), f"{name}: ld = {ld}, ld_style = {lds} and the dense call differ"
    assert torch.equal(raw(buf[:2 * FN, 3 * Cc:]), raw(before[:2 * FN, 3 * Cc:])), f"{name}: pad columns of qkv2 were written"
    assert torch.equal(raw(buf[2 * FN:]), raw(before[2 * FN:])), f"{name}: rows behind qkv2 were written"
    assert torch.equal(raw(sbuf), raw(sbefore)), f"{name}: the padded bank, its pad columns or the rows behind it were written"
    with pytest.raises(ValueError, match="unit column stride"):
        nat.sd3_adain_shift_static_(buf[:2 * FN, ::2], sview, *args)


# ------------------------------------------------------------------------------------------------ b. refusals
# what differs from (F 2, N 5, C 40, heads 5, ld 120, ld_style 80, all pointers set), what the message names
_SHIFT_REFUSALS = [
    ("null_qkv2", dict(qkv2=None), "qkv2 is null"),
    ("null_style_kv", dict(style_kv=None), "style_kv is null"),
    ("null_ws", dict(ws=None), "ws is null"),
    ("n_1", dict(N=1), "N=1"),
    ("c_mod_heads", dict(heads=3), "heads=3"),
    ("c_mod_8", dict(C=36, ld=112, ld_style=72), "C=36"),
    ("ld_mod_8", dict(ld=124), "ld=124"),
    ("ld_below_3c", dict(ld=112), "ld=112"),
    ("ld_style_mod_8", dict(ld_style=84), "ld_style=84"),
    ("ld_style_below_2c", dict(ld_style=72), "ld_style=72"),
]


@pytest.mark.parametrize("tag,args,names", _SHIFT_REFUSALS, ids=[r[0] for r in _SHIFT_REFUSALS])
def test_static_shift_refuses_before_any_launch(nat, tag, args, names):
    """UNIVST_ERR_ARG, the argument named, and nothing written: the -7 filled buffers are untouched after a synchronize"""
    buf = torch.full((2 * 2 * 5 + 8, 128), -7.0, dtype=torch.float16, device="cuda")
    sty = torch.full((5 + 8, 96), -7.0, dtype=torch.float16, device="cuda")
    ws = torch.full((1 << 14,), -7.0, dtype=torch.float32, device="cuda")
    a = dict(qkv2=buf.data_ptr(), style_kv=sty.data_ptr(), ws=ws.data_ptr(), F=2, N=5, C=40, heads=5, ld=120, ld_style=80)
    a.update(args)
    rc = nat.load().univst_sd3_adain_shift_static(a["qkv2"], a["ld"], a["style_kv"], a["ld_style"], a["F"], a["N"], a["C"], a["heads"], ac.SD3_ALPHA,
                                                  ac.BETA, ac.SD3_GAMMA, a["ws"], nat.stream_ptr())
    assert rc == -1, (tag, rc)
    with pytest.raises(RuntimeError, match=names):
        nat.check(rc, "sd3_adain_shift_static")
    torch.cuda.synchronize()
    assert (buf == -7).all() and (sty == -7).all() and (ws == -7).all(), (tag, "a refused call wrote")


def _attn_params(seed=99, Cw=128, heads=2):
    g = torch.Generator().manual_seed(seed)
    P = {}
    for nm in ("to_q", "to_k", "to_v", "add_q_proj", "add_k_proj", "add_v_proj", "to_out.0", "to_add_out"):
        P[nm + ".weight"] = (torch.randn(Cw, Cw, generator=g) / Cw ** 0.5).half().float()
        P[nm + ".bias"] = (0.1 * torch.randn(Cw, generator=g)).half().float()
    for nm in ("norm_q", "norm_k", "norm_added_q", "norm_added_k"):
        P[nm + ".weight"] = (1.0 + 0.2 * torch.randn(Cw // heads, generator=g)).half().float()
    return P


# role, B, clip_length, shift, style_kv set, ld_style, what the message names
_ATTN_REFUSALS = [
    ("apply_wrong_b", 1, 5, 5, 1, True, 256, r"B=5 must be 2 \* clip_length=5"),
    ("apply_three_branch_b", 1, 9, 3, 1, True, 256, r"B=9 must be 2 \* clip_length=3"),
    ("apply_null_bank", 1, 6, 3, 1, False, 256, "style_kv is null"),
    ("bank_null_bank", 0, 1, 1, 0, False, 256, "style_kv is null"),
    ("bank_shift", 0, 1, 1, 1, True, 256, "shift=1 must be 0"),
    ("apply_ld_style_mod_8", 1, 6, 3, 1, True, 260, "ld_style=260"),
    ("bank_ld_style_below_2c", 0, 1, 1, 0, True, 248, "ld_style=248"),
    ("role_2", 2, 6, 3, 0, True, 256, "role=2"),
]


def test_static_joint_attention_refuses_one_token_shift_before_any_launch(nat):
    """N = 1 in the apply role with the shift on: refused by the entry itself, as the stand-alone shift refuses it, before the projections are enqueued"""
    p = nat.Sd3AttnParams(_attn_params(), torch.device("cuda"))
    w = nat.Sd3AttnWeights(**{k: (p[k].data_ptr() if k in p else None) for k in nat.Sd3AttnWeights._NAMES})
    hid = torch.full((6, 1, 128), -7.0, dtype=torch.float16, device="cuda")
    out, bank = torch.full_like(hid, -7.0), torch.full((1, 256), -7.0, dtype=torch.float16, device="cuda")
    rc = nat.load().univst_sd3_joint_attention_static(C.byref(w), hid.data_ptr(), None, 6, 1, 0, 128, 2, 64, 3, 1, 0.5, 1e-6, out.data_ptr(), None, None,
                                                      nat.stream_ptr(), None, bank.data_ptr(), 256, 1)
    assert rc == -1, rc
    with pytest.raises(RuntimeError, match="N=1 must be at least 2"):
        nat.check(rc, "sd3_joint_attention_static")
    torch.cuda.synchronize()
    assert (out == -7).all() and (bank == -7).all()


@pytest.mark.parametrize("tag,role,B,clip,shift,has_bank,lds,names", _ATTN_REFUSALS, ids=[r[0] for r in _ATTN_REFUSALS])
def test_static_joint_attention_refuses_before_any_launch(nat, tag, role, B, clip, shift, has_bank, lds, names):
    p = nat.Sd3AttnParams(_attn_params(), torch.device("cuda"))
    w = nat.Sd3AttnWeights(**{k: (p[k].data_ptr() if k in p else None) for k in nat.Sd3AttnWeights._NAMES})
    N, Nt, Cw = 16, 5, 128
    hid = torch.full((B, N, Cw), -7.0, dtype=torch.float16, device="cuda")
    enc = torch.full((B, Nt, Cw), -7.0, dtype=torch.float16, device="cuda")
    out_i, out_t = torch.full_like(hid, -7.0), torch.full_like(enc, -7.0)
    bank = torch.full((N, 264), -7.0, dtype=torch.float16, device="cuda")
    rc = nat.load().univst_sd3_joint_attention_static(C.byref(w), hid.data_ptr(), enc.data_ptr(), B, N, Nt, Cw, 2, 64, clip, shift, 0.5, 1e-6,
                                                      out_i.data_ptr(), out_t.data_ptr(), None, nat.stream_ptr(), None,
                                                      bank.data_ptr() if has_bank else None, lds, role)
    assert rc == -1, (tag, rc)
    with pytest.raises(RuntimeError, match=names):
        nat.check(rc, "sd3_joint_attention_static")
    torch.cuda.synchronize()
    assert (out_i == -7).all() and (out_t == -7).all() and (bank == -7).all(), (tag, "a refused call wrote")


def test_binding_refuses_a_bank_it_cannot_pass(nat):
    hid = torch.zeros(2, 16, 128, dtype=torch.float16, device="cuda")
    bank = torch.zeros(16, 256, dtype=torch.float16, device="cuda")
    with pytest.raises(ValueError, match="static_role must be"):
        nat.sd3_joint_attention({}, hid, None, 2, static_role=2)
    with pytest.raises(ValueError, match="style_kv needs static_role"):
        nat.sd3_joint_attention({}, hid, None, 2, style_kv=bank)
    with pytest.raises(ValueError, match="unit column stride"):
        nat.sd3_joint_attention({}, hid, None, 2, style_kv=bank[:, ::2], static_role=1)
    with pytest.raises(ValueError, match="cannot be combined"):
        nat.sd3_joint_attention({}, hid, None, 2, style_kv=bank, static_role=1, comm=1)


# ------------------------------------------------------------------------------------------------ c. op level
@lru_cache(maxsize=2)
def _op_case(N):
    """F = 3, Nt = 5, 2 heads x 64: the three-branch batch with the style frame (and its text tokens) repeated, and the oracle's joint attention
    of it inside (idx 10) and outside (45) the window — computed once per token count"""
    F_, Nt, heads, Cw = 3, 5, 2, 128
    P = _attn_params()
    g = torch.Generator().manual_seed(200 + N)
    hid = torch.randn(3 * F_, N, Cw, generator=g).half()
    hid[2 * F_:] = hid[2 * F_:] * 1.4 - 0.2
    hid[F_:2 * F_] = (0.3 + 1.2 * hid[F_:F_ + 1]).half().expand(F_, -1, -1)
    enc = torch.randn(3 * F_, Nt, Cw, generator=g).half()
    enc[F_:2 * F_] = enc[F_:F_ + 1].clone().expand(F_, -1, -1)
    want = {idx: sd3_ref.joint_attention(P, heads, hid.float(), enc.float(), idx=idx, shift=True, eta1=0.0, eta2=0.6, clip_length=F_)
            for idx in (10, 45)}
    res_i, res_t = torch.randn(3 * F_, N, Cw, generator=g).half(), torch.randn(3 * F_, Nt, Cw, generator=g).half()
    gate_i, gate_t = torch.randn(3 * F_, Cw, generator=g).half(), torch.randn(3 * F_, Cw, generator=g).half()
    return P, hid, enc, want, (res_i, gate_i, res_t, gate_t)


@pytest.mark.parametrize("fused", [False, True], ids=["plain", "gated_residual"])
@pytest.mark.parametrize("idx", [10, 45])
@pytest.mark.parametrize("N", [16, 67])
def test_static_joint_attention_roles_vs_oracle(nat, N, idx, fused):
    """role 0 on the one style frame, then role 1 on [content | stylised], against branches 0 and 2 of the oracle's three-branch joint attention
    (N = 16: one key tile; N = 67: two tiles with a 3-key tail, ragged 16-byte pieces per wave in the shift); plain and with the gated residual
    in the out-projections' epilogue.  The style frame's own output is the oracle's branch 1."""
    F_, heads = 3, 2
    P, hid, enc, want, (res_i, gate_i, res_t, gate_t) = _op_case(N)
    params = nat.Sd3AttnParams(P, torch.device("cuda"))
    w_img, w_txt = want[idx]
    if fused:
        w_img = res_i.float() + gate_i.float()[:, None] * w_img
        w_txt = res_t.float() + gate_t.float()[:, None] * w_txt
    pick = lambda t, rows: t[rows].cuda().contiguous()          # noqa: E731
    fuse = lambda rows: dict(res_img=pick(res_i, rows), gate_img=pick(gate_i, rows), res_txt=pick(res_t, rows),          # noqa: E731
                             gate_txt=pick(gate_t, rows)) if fused else None
    one = slice(F_, F_ + 1)
    bank = torch.full((N, 2 * 128), float("nan"), dtype=torch.float16, device="cuda")
    s_img, s_txt = nat.sd3_joint_attention(params, pick(hid, one), pick(enc, one), heads, clip_length=1, shift=False, idx=idx, fuse=fuse(one),
                                           style_kv=bank, static_role=0)
    assert torch.isfinite(bank).all(), "role 0 fills the whole bank"
    kept = bank.clone()
    two = torch.cat([torch.arange(F_), torch.arange(2 * F_, 3 * F_)])
    g_img, g_txt = nat.sd3_joint_attention(params, pick(hid, two), pick(enc, two), heads, clip_length=F_, shift=True, idx=idx, eta1=0.0, eta2=0.6,
                                           fuse=fuse(two), style_kv=bank, static_role=1)
    torch.cuda.synchronize()
    assert torch.equal(bank, kept), "role 1 only reads the bank"
    for what, got, ref in (("img", g_img, w_img[two]), ("txt", g_txt, w_txt[two]), ("style img", s_img, w_img[one]), ("style txt", s_txt, w_txt[one])):
        mx, rms = errs(got, ref)
        print(f"static joint attention N={N} idx={idx} fused={fused} {what}: max {mx:.2e} rms {rms:.2e}")
        assert mx < 4e-3 and rms < 1e-3, (what, mx, rms)
    if idx == 45:          # outside the window the bank may be absent, and the call is the ordinary entry on the two-branch batch, bit for bit
        n_img, n_txt = nat.sd3_joint_attention(params, pick(hid, two), pick(enc, two), heads, clip_length=F_, shift=True, idx=idx, eta1=0.0, eta2=0.6,
                                               fuse=fuse(two), style_kv=None, static_role=1)
        p_img, p_txt = nat.sd3_joint_attention(params, pick(hid, two), pick(enc, two), heads, clip_length=F_, shift=False, idx=idx, fuse=fuse(two))
        assert torch.equal(n_img, g_img) and torch.equal(n_txt, g_txt) and torch.equal(p_img, g_img) and torch.equal(p_txt, g_txt)


# ------------------------------------------------------------------------------------------------ d, e. model level
def _tiny_sd3(layers=2, dual=(0,), qk_norm="rms_norm", heads=2, seed=11):
    """tests/test_gpu_sd3.py::_tiny_sd3(layers=2, dual=(0,)), restated"""
    from univst_amd.backbones.video_diffusion_sd3.models.transformer_3D_model import CustomSD3Transformer2DModel
    torch.manual_seed(seed)
    m = CustomSD3Transformer2DModel(sample_size=32, patch_size=2, in_channels=16, num_layers=layers, attention_head_dim=64,
                                    num_attention_heads=heads, joint_attention_dim=64, caption_projection_dim=64 * heads, pooled_projection_dim=32,
                                    out_channels=16, pos_embed_max_size=24, dual_attention_layers=dual, qk_norm=qk_norm)
    for n, p in m.named_parameters():                       # adaLN / RMS weights away from their trivial values
        if n.endswith("norm_q.weight") or n.endswith("norm_k.weight") or "norm_added" in n:
            p.data = 1.0 + 0.2 * torch.randn_like(p)
    m = m.half()
    P = {k: v.float() for k, v in m.state_dict().items()}   # the oracle sees the fp16-rounded weights
    return m.cuda(), P


@lru_cache(maxsize=2)
def _model_case(F_):
    """the tiny MM-DiT with the shift processors registered at clip_length = F, the three-branch inputs (8 x 8 latents, 5 text tokens) with the
    style frame, its text tokens and its pooled vector repeated, and the oracle's stylised branch inside the window (idx 10) — once per F"""
    from univst_amd.backbones.video_diffusion_sd3 import pnp_utils
    m, P = _tiny_sd3()
    pnp_utils.register_spatial_attention_pnp(types.SimpleNamespace(transformer=m), eta1=0.0, eta2=0.6)
    for proc in m.attn_processors.values():
        proc.clip_length = F_
    g = torch.Generator().manual_seed(40 + F_)
    lat, enc, pooled = torch.randn(3 * F_, 16, 8, 8, generator=g).half(), torch.randn(3 * F_, 5, 64, generator=g).half(), \
        torch.randn(3 * F_, 32, generator=g).half()
    for t in (lat, enc, pooled):
        t[F_:2 * F_] = t[F_:F_ + 1].clone().expand(F_, *t.shape[1:])
    t = torch.tensor([437.0])
    want = sd3_ref.sd3_transformer(P, m.config, lat.float(), enc.float(), pooled.float(), t,
                                   attn_kw=dict(idx=10, shift=True, eta1=0.0, eta2=0.6, clip_length=F_))[2 * F_:]
    return m, lat, enc, pooled, t, want


def _three_branch(m, lat, enc, pooled, t, idx):
    return m(hidden_states=lat.cuda(), timestep=t.cuda().expand(lat.shape[0]), encoder_hidden_states=enc.cuda(), pooled_projections=pooled.cuda(),
             return_dict=False, joint_attention_kwargs={"idx": idx})[0]


def _static(m, lat, enc, pooled, t, idx, F_, bank=None, run_bank=True):
    one = slice(F_, F_ + 1)
    two = torch.cat([torch.arange(F_), torch.arange(2 * F_, 3 * F_)])
    if run_bank:
        bank = m.style_bank(lat[one].cuda(), t.cuda(), enc[one].cuda(), pooled[one].cuda(), idx, bank)
    out = m.forward_static_style(lat[two].cuda(), t.cuda().expand(2 * F_), enc[two].cuda(), pooled[two].cuda(), idx, bank)
    return out, bank


@pytest.mark.parametrize("F_", [3, 5])
def test_static_style_forward_vs_restatement_and_three_branch(nat, F_):
    """style_bank + forward_static_style against the fp32 restatement of the MM-DiT on the 3F batch with the style frame repeated (stylised
    branch), and against the native three-branch forward, from which only summation orders differ; the content branch is the three-branch one's"""
    m, lat, enc, pooled, t, want = _model_case(F_)
    m.set_qkv_dtype("fp16")
    got, bank = _static(m, lat, enc, pooled, t, 10, F_)
    assert bank is not None and len(bank.buffers()) == 3 and all(tuple(b.shape) == (16, 256) for b in bank.buffers())
    assert bank.nbytes() == 3 * 16 * 256 * 2
    mx, rms = errs(got[F_:], want)
    print(f"static style F={F_}: stylised branch vs fp32 restatement: max {mx:.2e} rms {rms:.2e}")
    assert mx < 1e-2 and rms < 4e-3, (mx, rms)
    full = _three_branch(m, lat, enc, pooled, t, 10)
    mx3, rms3 = errs(got[F_:], full[2 * F_:])
    print(f"static style F={F_}: stylised branch vs the native three-branch forward: max {mx3:.2e} rms {rms3:.2e}")
    assert mx3 < 6e-3 and rms3 < 1.5e-3, (mx3, rms3)
    mxc, rmsc = errs(got[:F_], full[:F_])
    print(f"static style F={F_}: content branch vs the native three-branch forward: max {mxc:.2e} rms {rmsc:.2e}")
    assert mxc < 6e-3 and rmsc < 1.5e-3, (mxc, rmsc)
    # the same bank object is reused: a second step writes the same buffers
    ptrs = [b.data_ptr() for b in bank.buffers()]
    _, bank2 = _static(m, lat, enc, pooled, t, 11, F_, bank=bank)
    assert bank2 is bank and [b.data_ptr() for b in bank.buffers()] == ptrs


def test_static_style_forward_mxfp8_vs_three_branch(nat):
    """set_qkv_dtype("mxfp8"): the bank call and the apply call quantise the same rows the three-branch forward quantises"""
    F_ = 3
    m, lat, enc, pooled, t, _ = _model_case(F_)
    m.set_qkv_dtype("mxfp8")
    try:
        got, _ = _static(m, lat, enc, pooled, t, 10, F_)
        full = _three_branch(m, lat, enc, pooled, t, 10)
    finally:
        m.set_qkv_dtype("fp16")
    mx, rms = errs(got[F_:], full[2 * F_:])
    print(f"static style mxfp8: stylised branch vs the native three-branch mxfp8 forward: max {mx:.2e} rms {rms:.2e}")
    assert mx < 6e-3 and rms < 1.5e-3, (mx, rms)


def test_bank_is_read_inside_the_window_and_nothing_runs_outside(nat):
    F_ = 3
    m, lat, enc, pooled, t, want = _model_case(F_)
    m.set_qkv_dtype("fp16")
    good, bank = _static(m, lat, enc, pooled, t, 10, F_)
    for b in bank.buffers():
        b.zero_()
    zeroed, _ = _static(m, lat, enc, pooled, t, 10, F_, bank=bank, run_bank=False)
    mx, rms = errs(zeroed[F_:], want)
    print(f"zeroed bank: stylised branch vs fp32 restatement: max {mx:.2e} rms {rms:.2e}")
    assert not (mx < 1e-2 and rms < 4e-3), "the stylised branch does not read the bank"
    assert torch.equal(zeroed[:F_], good[:F_]), "the content branch never reads the bank"
    # outside the window: no bank, nothing run, nothing written; the static forward is the plain two-branch forward
    for b in bank.buffers():
        b.fill_(-7.0)
    one = slice(F_, F_ + 1)
    assert m.style_bank(lat[one].cuda(), t.cuda(), enc[one].cuda(), pooled[one].cuda(), 45, bank) is None
    assert m.style_bank(lat[one].cuda(), t.cuda(), enc[one].cuda(), pooled[one].cuda(), 45) is None
    torch.cuda.synchronize()
    assert all((b == -7).all() for b in bank.buffers()), "style_bank wrote outside the window"
    two = torch.cat([torch.arange(F_), torch.arange(2 * F_, 3 * F_)])
    out, _ = _static(m, lat, enc, pooled, t, 45, F_, bank=None, run_bank=False)
    plain = _three_branch(m, lat[two], enc[two], pooled[two], t, 45)
    assert torch.equal(out, plain), "outside the window forward_static_style is the two-branch forward"
    with pytest.raises(ValueError, match="needs the bank"):
        m.forward_static_style(lat[two].cuda(), t.cuda().expand(2 * F_), enc[two].cuda(), pooled[two].cuda(), 10, None)


def test_static_style_and_frame_shard_refuse_each_other(nat):
    from univst_amd.backbones.video_diffusion_sd3 import pnp_utils
    F_ = 3
    m, lat, enc, pooled, t, _ = _model_case(F_)
    attn = m.transformer_blocks[0].attn
    attn._uv_frame_shard = types.SimpleNamespace(world=2, local=F_, comm=types.SimpleNamespace(ptr=None))
    try:
        with pytest.raises(NotImplementedError, match=r"static_style under a frame shard \(world 2\)"):
            _static(m, lat, enc, pooled, t, 10, F_, bank=pnp_utils.StaticStyleBank())
    finally:
        del attn._uv_frame_shard


# ------------------------------------------------------------------------------------------------ f. loops
ETA1, ETA2 = 0.0, 0.6


def _open(i):
    return i >= ETA1 * 50 and i <= ETA2 * 50


def _windowed_velocity(x, t, i, F_):
    """sd3_ref.toy_velocity with its cross-branch term only inside the shift window, as the MM-DiT has it: outside, the stylised branch's velocity
    does not depend on the other two.  x [3F, ...] fp32"""
    v = sd3_ref.toy_velocity(x, t, i, -1)
    if _open(i):
        v = torch.cat([v[:2 * F_], v[2 * F_:] + 0.2 * x[:F_] - 0.1 * x[F_:2 * F_]])
    return v


class _ToyStaticTransformer:
    """the test double of tests/test_gpu_sd3.py::_ToyTransformer with the static-style surface of CustomSD3Transformer2DModel: the same windowed
    velocity on whichever batch the pipeline sends"""
    config = types.SimpleNamespace(in_channels=4, patch_size=2, sample_size=6, joint_attention_dim=8)
    device = torch.device("cuda")

    def __init__(self, frames):
        from univst_amd.backbones.video_diffusion_sd3.pnp_utils import AttentionShiftProcessor
        self.frames, self.calls = frames, []
        self.attn_processors = {"transformer_blocks.0.attn.processor": AttentionShiftProcessor(ETA1, ETA2)}

    def __call__(self, hidden_states, timestep, encoder_hidden_states=None, pooled_projections=None, return_dict=False, joint_attention_kwargs=None):
        idx = (joint_attention_kwargs or {}).get("idx", 0)
        assert encoder_hidden_states.shape[0] == pooled_projections.shape[0] == timestep.shape[0] == hidden_states.shape[0]
        self.calls.append(("forward", hidden_states.shape[0], idx))
        x = hidden_states.float()
        if x.shape[0] == 3 * self.frames:
            return (_windowed_velocity(x, timestep, idx, self.frames).half(),)
        return (sd3_ref.toy_velocity(x, timestep, idx, -1).half(),)

    def style_bank(self, frame, timestep, enc1, pooled1, idx, bank=None):
        if not _open(idx):
            return None
        assert frame.shape[0] == enc1.shape[0] == pooled1.shape[0] == timestep.shape[0] == 1
        self.calls.append(("style_bank", 1, idx))
        bank = {} if bank is None else bank
        bank["style"] = frame.float()
        return bank

    def forward_static_style(self, sample2, timestep, enc2, pooled2, idx, bank):
        F_ = self.frames
        assert sample2.shape[0] == enc2.shape[0] == pooled2.shape[0] == timestep.shape[0] == 2 * F_
        self.calls.append(("forward_static_style", 2 * F_, idx))
        x = sample2.float()
        v = sd3_ref.toy_velocity(x, timestep, idx, -1)
        if _open(idx):
            v = torch.cat([v[:F_], v[F_:] + 0.2 * x[:F_] - 0.1 * bank["style"]])
        else:
            assert bank is None
        return v.half()


@lru_cache(maxsize=1)
def _loop_case():
    """the inputs of test_sd3_pipeline_loops_vs_g19 with the style frame repeated, and the reference-pinned loop over the windowed velocity,
    without and with the mask"""
    ti = sd3_ref.toy_loop_inputs()
    Fr = ti["content"][0].shape[0]
    style_rep = [s[:1].expand(Fr, -1, -1, -1).contiguous() for s in ti["style"]]
    style_one = [s[:1].contiguous() for s in ti["style"]]
    from univst_amd.backbones.video_diffusion_sd3.pnp_utils import latent_adain
    start = latent_adain(ti["content"][50].half().cuda(), style_rep[50].half().cuda())
    ts, sig = sd3_ref.flow_match_schedule(50)
    eta = sd3_ref.generate_eta_values(ts, 25, 39, 0.85, "constant")
    vf = lambda x, t, i: _windowed_velocity(x, t, i, Fr)          # noqa: E731
    want = {m: sd3_ref.sd3_transfer_loop(vf, start.float().cpu(), ti["content"][0], ti["content"], style_rep, ts, sig, eta,
                                         mask=ti["mask"] if m else None) for m in (False, True)}
    return ti, Fr, style_rep, style_one, start, want


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("static,skip", [(True, False), (False, True), (True, True)], ids=["static_style", "skip_dead_branches", "both"])
def test_sd3_transfer_loop_switches_vs_reference_loop(nat, static, skip, masked):
    from univst_amd.backbones.video_diffusion_sd3.pipelines.custom_pipeline import CustomStableDiffusion3Pipeline
    from univst_amd.schedulers import FlowMatchEulerDiscreteScheduler
    ti, Fr, style_rep, style_one, start, want = _loop_case()
    kw = dict(latents=start, img_latents=ti["content"][0], num_inference_steps=50, prompt_embeds=torch.zeros(1, 3, 8), pooled_prompt_embeds=torch.zeros(1, 8),
              eta_base=0.85, eta_trend="constant", start_step=25, end_step=39, output_type="latent", content_inv_latents=ti["content"],
              masks=ti["mask"] if masked else None, static_style=static, skip_dead_branches=skip)
    pipe = CustomStableDiffusion3Pipeline(transformer=_ToyStaticTransformer(Fr), scheduler=FlowMatchEulerDiscreteScheduler())
    out = pipe.video_style_transfer("", style_inv_latents=style_rep, **kw).images
    mx, rms = errs(out, want[masked])
    print(f"transfer loop static_style={static} skip_dead_branches={skip} mask={masked}: max {mx:.2e} rms {rms:.2e}")
    assert mx < 6e-3 and rms < 2e-3, (mx, rms)
    calls = pipe.transformer.calls
    inside = [c for c in calls if c[2] <= 30]
    outside = [c for c in calls if c[2] > 30]
    if static:
        assert [c[:2] for c in inside] == [("style_bank", 1), ("forward_static_style", 2 * Fr)] * 31          # 2F + 1 frame-forwards a step
    else:
        assert [c[:2] for c in inside] == [("forward", 3 * Fr)] * 31
    if skip:
        assert [c[:2] for c in outside] == [("forward", Fr)] * 19                                           # the stylised branch alone
    elif static:
        assert [c[:2] for c in outside] == [("forward_static_style", 2 * Fr)] * 19
    if static:          # one-frame and F-frame style latents give the same result
        pipe1 = CustomStableDiffusion3Pipeline(transformer=_ToyStaticTransformer(Fr), scheduler=FlowMatchEulerDiscreteScheduler())
        out1 = pipe1.video_style_transfer("", style_inv_latents=style_one, **kw).images
        assert torch.equal(out1, out), "one-frame and F-frame style latents differ"


def test_sd3_transfer_loop_switch_refusals(nat):
    from univst_amd.backbones.video_diffusion_sd3.pnp_utils import AttentionShiftProcessor
    from univst_amd.backbones.video_diffusion_sd3.pipelines.custom_pipeline import CustomStableDiffusion3Pipeline
    from univst_amd.schedulers import FlowMatchEulerDiscreteScheduler
    ti, Fr, style_rep, style_one, start, _ = _loop_case()
    kw = dict(latents=start, img_latents=ti["content"][0], num_inference_steps=50, prompt_embeds=torch.zeros(1, 3, 8), pooled_prompt_embeds=torch.zeros(1, 8),
              output_type="latent", content_inv_latents=ti["content"])
    pipe = CustomStableDiffusion3Pipeline(transformer=_ToyStaticTransformer(Fr), scheduler=FlowMatchEulerDiscreteScheduler())
    bad = [s[:2].contiguous() for s in ti["style"]]
    with pytest.raises(ValueError, match=r"got \(2, 4, 6, 6\)"):
        pipe.video_style_transfer("", style_inv_latents=bad, static_style=True, **kw)
    with pytest.raises(NotImplementedError, match="static_style under a frame shard"):
        pipe.video_style_transfer("", style_inv_latents=style_rep, static_style=True, shard=types.SimpleNamespace(world=2), **kw)
    pipe.transformer.attn_processors["transformer_blocks.0.attn2.processor"] = AttentionShiftProcessor(0.0, 0.5)
    for sw in (dict(static_style=True), dict(skip_dead_branches=True)):
        with pytest.raises(ValueError, match="disagree on the shift window"):
            pipe.video_style_transfer("", style_inv_latents=style_rep, **sw, **kw)


# ------------------------------------------------------------------------------------------------ g. one-frame inversion
class _Bar:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def update(self):
        pass


def test_one_frame_rf_inversion_is_frame_0_of_the_inversion_of_f_copies(nat, tmp_path):
    """what run_style_inversion_sd3.py --static_style does: the tiny MM-DiT with the CrossFrameProcessors of the inversion entry points, one style
    frame as a clip of its own (clip_length 1) against F = 4 copies of it as one clip (clip_length 4), ten steps of rf_inversion at gamma = 0 (the
    style inversion's value: the Gaussian target has weight 0, so the two runs do not depend on how many frames of noise were drawn).  Identical
    frames stay identical, and the files of the one-frame run hold [1, 16, h, w]."""
    from univst_amd.backbones.video_diffusion_sd3.pnp_utils import CrossFrameProcessor
    from univst_amd.inversion_tools import flow_inversion as fi
    from univst_amd.schedulers import FlowMatchEulerDiscreteScheduler
    m, _ = _tiny_sd3()
    m.set_attn_processor({n: CrossFrameProcessor() for n in m.attn_processors})
    g = torch.Generator().manual_seed(77)
    z1 = torch.randn(1, 16, 8, 8, generator=g).half()
    pe, pp = torch.randn(1, 5, 64, generator=g).half().cuda(), torch.randn(1, 32, generator=g).half().cuda()
    pipe = types.SimpleNamespace(device="cuda", scheduler=FlowMatchEulerDiscreteScheduler(), transformer=m,
                                 encode_prompt=lambda prompt, prompt_2, prompt_3: (pe, None, pp, None), progress_bar=lambda total=None: _Bar())
    Fc = 4

    def run(z, frames, path):
        for proc in m.attn_processors.values():
            proc.clip_length = frames
        path.mkdir()
        torch.manual_seed(1701)
        return fi.rf_inversion(pipe, z.cuda(), gamma=0.0, num_inference_steps=10, inversion_path=str(path))
    full = run(z1.expand(Fc, -1, -1, -1).contiguous(), Fc, tmp_path / "f")
    one = run(z1, 1, tmp_path / "one")
    assert tuple(one.shape) == (1, 16, 8, 8) and tuple(full.shape) == (Fc, 16, 8, 8)
    mx, rms = errs(one, full[:1])
    print(f"one-frame rf_inversion vs frame 0 of {Fc} copies: max {mx:.2e} rms {rms:.2e}")
    assert mx < 5e-3 and rms < 2e-3, (mx, rms)
    spread = errs(full[1:], full[:1].expand(Fc - 1, -1, -1, -1))
    print(f"frames 1 .. {Fc - 1} of the {Fc}-copy inversion vs its frame 0: max {spread[0]:.2e} rms {spread[1]:.2e}")
    assert spread[0] < 5e-3 and spread[1] < 2e-3, spread
    for k in (0, 5, 10):
        assert tuple(torch.load(tmp_path / "one" / f"ddim_latents_{k}.pt", weights_only=True).shape) == (1, 16, 8, 8)
        assert tuple(torch.load(tmp_path / "f" / f"ddim_latents_{k}.pt", weights_only=True).shape) == (Fc, 16, 8, 8)
