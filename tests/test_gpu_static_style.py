"""The static style branch on the GPU: the style image as ONE frame instead of F copies of it (DESIGN.md "Static style branch").

a  univst_attention_adain_shift_static against float64: oracle.adain_ref.shift_ref on the three-branch buffer whose style rows are the one frame
   repeated F times, held to oracle.adain_cases.shift_bound of that shape (the bound of the three-branch kernel: the arithmetic is the same).
b  style_bank + forward_static_style against unet_ref.unet_forward on the B = 3 batch with the style frame repeated, branch 2: the file-wide bound of
   tests/test_gpu_unet.py (max < 2e-2 max|ref|, relative rms < 5e-3); and against the native three-branch forward on the same batch: max < 5e-3
   max|ref|, the project's bound for "only summation orders differ" (sharded = unsharded).
c  another style frame in the bank moves the stylised eps by more than 5e-2 of its maximum (the oracle alone gives 0.165 on the CPU).
d  outside the window: the ordinary B = 2 forward bit for bit, no bank needed, none written.
e  transfer_loop(static_style=True) and the existing loop against the oracle's loop, PSNR >= 40 dB each; a one-frame inversion against frame 0 of
   the same inversion on three copies.
f  every refusal returns its code before a launch.

Every figure is printed (pytest -s) before it is asserted."""
import ctypes as C
import functools
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import adain_cases as ac, adain_ref as ar, pipeline_ref, unet_ref, synth_inputs as si  # noqa: E402

T = 501


# ------------------------------------------------------------------------------------------------ a: the operator
def _shift_case(F, N, C):
    """three-branch fp16 buffer [3 F N, 3C] whose style rows are one frame repeated F times (base data of oracle/adain_cases: 0.2 + 1.5 n, with
    + 48 on every K | V column of the style frame's first and last row), its float64 reference, and the bound of the three-branch kernel"""
    g = torch.Generator().manual_seed(4100 + F * 1000 + N * 10 + C)
    FN = F * N
    x = 0.2 + 1.5 * torch.randn(3 * FN, 3 * C, generator=g)
    frame = 0.2 + 1.5 * torch.randn(N, 3 * C, generator=g)
    for r in {0, N - 1}:
        frame[r, C:] += ac.SENTINEL * 1.5
    x[FN:2 * FN] = frame.repeat(F, 1)
    qkv = x.half()
    b = types.SimpleNamespace(case=ac.ShiftCase(f"static_{F}_{N}_{C}", F, N, C, 0, "normal"), qkv=qkv, sd3=False,
                              ref=ar.shift_ref(qkv, F, N, C, ac.ALPHA, ac.BETA, ac.GAMMA))
    return b, ac.shift_bound(b)


@pytest.mark.parametrize("F,N,C,pad", [(3, 37, 64, False), (2, 300, 640, False), (2, 70, 1280, False), (1, 1, 8, False), (3, 37, 64, True)])
def test_static_shift_against_float64(F, N, C, pad):
    """each width instantiation (C / 8 <= 64, <= 128, <= 256 chunks), ragged N, the smallest legal case; `pad`: ld = 3C + 24 and ld_style = 2C + 16 with
    NaN in the padding — padding, content rows and style rows come back bit-identical, and the result is that of the dense call"""
    from univst_amd import _native as nat
    b, bound = _shift_case(F, N, C)
    FN = F * N
    two = torch.cat([b.qkv[:FN], b.qkv[2 * FN:]]).cuda()
    style = b.qkv[FN:FN + N, C:].contiguous().cuda()
    raw = lambda t: t.view(torch.int16)
    if pad:
        qbuf = torch.full((2 * FN + 5, 3 * C + 24), float("nan"), dtype=torch.float16, device="cuda")
        sbuf = torch.full((N + 5, 2 * C + 16), float("nan"), dtype=torch.float16, device="cuda")
        qbuf[:2 * FN, :3 * C] = two
        sbuf[:N, :2 * C] = style
        q0, s0 = qbuf.clone(), sbuf.clone()
        qv, sv = qbuf[:2 * FN, :3 * C], sbuf[:N, :2 * C]
        assert qv.stride() == (3 * C + 24, 1) and sv.stride() == (2 * C + 16, 1)
        nat.attention_adain_shift_static_(qv, sv, F, N, C, ac.ALPHA, ac.BETA, ac.GAMMA)
        torch.cuda.synchronize()
        assert torch.equal(raw(sbuf), raw(s0)), "the style rows or their padding were written"
        assert torch.equal(raw(qbuf[:FN]), raw(q0[:FN])) and torch.equal(raw(qbuf[2 * FN:]), raw(q0[2 * FN:])), "content rows / rows behind the buffer were written"
        assert torch.equal(raw(qbuf[:, 3 * C:]), raw(q0[:, 3 * C:])), "padding columns were written"
        dense = two.clone()
        nat.attention_adain_shift_static_(dense, style, F, N, C, ac.ALPHA, ac.BETA, ac.GAMMA)
        assert torch.equal(qv, dense), "padded and dense calls differ"
        got = qv.contiguous().cpu()
    else:
        s0 = style.clone()
        nat.attention_adain_shift_static_(two, style, F, N, C, ac.ALPHA, ac.BETA, ac.GAMMA)
        torch.cuda.synchronize()
        assert torch.equal(raw(style), raw(s0)), "the style rows were written"
        got = two.cpu()
    assert torch.equal(got[:FN], b.qkv[:FN]), "content rows must be bit-untouched"
    out, ref = got[FN:], b.ref.out[2 * FN:]
    ratio = (out.double() - ref).abs() / bound
    msg = f"static shift F={F} N={N} C={C} pad={pad}: max(err / bound) Q {ratio[:, :C].max().item():.3f}  K|V {ratio[:, C:].max().item():.3f}"
    print(msg)
    assert torch.isfinite(out).all() and ratio.max().item() <= 1.0, msg


@pytest.mark.parametrize("what,kw", [("ld_style=24", dict(ld_style=24)), ("ld=112", dict(ld=112)), ("C=36", dict(C=36, ld=120, ld_style=80)),
                                     ("ld_style=84", dict(ld_style=84)), ("F=0", dict(F=0)), ("N=0", dict(N=0))])
def test_static_shift_refuses_before_any_launch(what, kw):
    """the refusals of the three-branch launcher plus ld_style < 2C, each named in the message; nothing is written"""
    from univst_amd import _native as nat
    a = dict(F=2, N=5, C=40, ld=120, ld_style=80)
    a.update(kw)
    q = torch.full((64, 256), 3.0, dtype=torch.float16, device="cuda")
    s = torch.full((64, 256), 5.0, dtype=torch.float16, device="cuda")
    ws = torch.zeros(4 * 64, dtype=torch.float32, device="cuda")
    rc = nat.load().univst_attention_adain_shift_static(q.data_ptr(), a["ld"], s.data_ptr(), a["ld_style"], a["F"], a["N"], a["C"], 0.65, 0.5, 3.0,
                                                        ws.data_ptr(), nat.stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and what in nat.load().univst_last_error().decode(), (rc, nat.load().univst_last_error())
    assert (q == 3.0).all() and (s == 5.0).all() and (ws == 0).all()


# ------------------------------------------------------------------------------------------------ b - d: the UNet
def errs(got, ref):
    got, ref = got.float().cpu(), ref.float().cpu()
    e = got - ref
    return e.abs().max().item() / ref.abs().max().item(), (e.pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()).item()


@functools.lru_cache(maxsize=None)
def model(kind):
    """-> (native UNet with PnP registered, state dict, config); one per kind for the whole file"""
    from univst_amd.backbones.video_diffusion_sd.models.unet_3d_condition import UNetPseudo3DConditionModel
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    cfg = unet_ref.TINY_SD2_CONFIG if kind == "sd2" else unet_ref.TINY_CONFIG
    sd = unet_ref.synth_state_dict(cfg, seed=33, trivial_temporal=kind != "trained")
    unet = UNetPseudo3DConditionModel(block_out_channels=cfg["block_out_channels"], cross_attention_dim=cfg["cross_attention_dim"],
                                      attention_head_dim=cfg["attention_head_dim"], norm_num_groups=cfg["norm_num_groups"],
                                      use_linear_projection=kind == "sd2")
    unet.load_state_dict(sd)
    unet = unet.half().cuda()
    pnp_utils.register_spatial_attention_pnp(types.SimpleNamespace(unet=unet))
    return unet, sd, cfg


def set_idx(unet, idx):
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    pnp_utils.register_time(types.SimpleNamespace(unet=unet), idx)


def batch(cfg, F, h, w, style_k=50):
    """(x [3,4,F,h,w] with the style frame repeated, ctx [3,77,D]) fp16 on the GPU"""
    frame = si.style_latent(style_k, 1, h, w)
    x = torch.cat([si.content_latent(50, F, h, w), frame.expand(-1, -1, F, -1, -1), si.content_latent(49, F, h, w)])
    ctx = si.text_embedding(cfg["cross_attention_dim"]).expand(3, -1, -1).contiguous()
    return x.half().cuda(), ctx.half().cuda()


def static_step(unet, x, ctx):
    """the stylised eps [1,4,F,h,w] of the static step on the three-branch inputs (x, ctx): bank call on frame 0 of branch 1, then B = 2"""
    bank = unet.style_bank(x[1:2, :, :1], T, ctx[1:2])
    assert bank is not None and bank.dtype == torch.uint8
    return unet.forward_static_style(torch.cat([x[0:1], x[2:3]]), T, torch.cat([ctx[0:1], ctx[2:3]]), bank).sample[1:2]


@functools.lru_cache(maxsize=None)
def step_results(kind, F, h, w):
    """(static, native three-branch, oracle) stylised eps at idx 5, computed once and shared"""
    unet, sd, cfg = model(kind)
    set_idx(unet, 5)
    x, ctx = batch(cfg, F, h, w)
    static = static_step(unet, x, ctx)
    three = unet(x, T, encoder_hidden_states=ctx).sample[2:3]
    with torch.no_grad():
        ref = unet_ref.unet_forward(sd, cfg, x.float().cpu(), T, ctx.float().cpu(), pnp_idx=5, exact_temporal=False)[0][2:3]
    return static, three, ref


@pytest.mark.parametrize("kind", ["sd1", "sd2"])
@pytest.mark.parametrize("F,h,w", [(3, 16, 24), (1, 16, 16), (2, 24, 8)])
def test_static_step_vs_oracle_and_three_branch(kind, F, h, w):
    static, three, ref = step_results(kind, F, h, w)
    mx, rms = errs(static, ref)
    mx3, _ = errs(static, three)
    print(f"static step {kind} F={F} {h}x{w}: vs oracle max {mx:.3e} rms {rms:.3e}; vs native three-branch max {mx3:.3e}")
    assert static.shape == (1, 4, F, h, w) and torch.isfinite(static).all()
    assert mx < 2e-2 and rms < 5e-3, (mx, rms)
    assert mx3 < 5e-3, mx3


def test_bank_is_read():
    """the bank of another style frame moves the stylised eps by more than 5e-2 of its maximum (oracle alone, on the CPU: 0.165)"""
    unet, sd, cfg = model("sd1")
    static, _, _ = step_results("sd1", 3, 16, 24)
    set_idx(unet, 5)
    x, ctx = batch(cfg, 3, 16, 24)
    other, _ = batch(cfg, 3, 16, 24, style_k=37)
    x37 = x.clone()
    x37[1] = other[1]
    moved = static_step(unet, x37, ctx)
    d = (moved.float() - static.float()).abs().max().item() / static.float().abs().max().item()
    print(f"another style frame moves the stylised eps by {d:.3f} of max")
    assert d > 5e-2, d


def test_outside_the_window_is_the_two_branch_forward():
    unet, sd, cfg = model("sd1")
    set_idx(unet, 30)
    x, ctx = batch(cfg, 3, 16, 24)
    x2, ctx2 = torch.cat([x[0:1], x[2:3]]), torch.cat([ctx[0:1], ctx[2:3]])
    plain = unet(x2, T, encoder_hidden_states=ctx2).sample
    got = unet.forward_static_style(x2, T, ctx2, None).sample
    assert torch.equal(got, plain)
    need = unet.style_bank(x[1:2, :, :1], T, ctx[1:2])
    assert need is None                                             # inactive, and nothing allocated for the caller
    set_idx(unet, 5)
    size = unet.style_bank(x[1:2, :, :1], T, ctx[1:2]).numel()
    set_idx(unet, 30)
    bank = torch.full((size,), 0xA5, dtype=torch.uint8, device="cuda")
    assert unet.style_bank(x[1:2, :, :1], T, ctx[1:2], bank=bank) is None
    torch.cuda.synchronize()
    assert (bank == 0xA5).all(), "an inactive style_bank call wrote the bank"


def test_alternating_geometries_allocate_nothing_after_the_first_step():
    """the (1, 1) bank call and the (2, F) forward alternate every step: the K/V source tables of both are uploaded once and the arena is not
    replaced after the first step; the bank's size is the documented layout"""
    from univst_amd import _native
    unet, sd, cfg = model("sd1")
    set_idx(unet, 5)
    F, h, w = 3, 16, 24
    x, ctx = batch(cfg, F, h, w)
    first = static_step(unet, x, ctx)
    q = lambda n: _native.unet_query(unet._native_handle, n)
    before = (q("idx_tables"), q("arena_bytes"))
    for _ in range(2):
        again = static_step(unet, x, ctx)
    assert (q("idx_tables"), q("arena_bytes")) == before, (before, q("idx_tables"), q("arena_bytes"))
    assert torch.equal(first, again)
    boc = cfg["block_out_channels"]
    want = sum((((h >> s) * (w >> s) * 2 * boc[s] * 2 + 255) // 256 * 256) * n for s, n in ((2, 2), (1, 3), (0, 3)))
    assert _native.load().univst_unet_style_bank_bytes(unet._native_handle, h, w) == want


# ------------------------------------------------------------------------------------------------ e: the loops
def psnr(got, ref):
    import math
    got, ref = got.float().cpu(), ref.float().cpu()
    mse = (got - ref).pow(2).mean().item()
    peak = (ref.max() - ref.min()).item()
    return float("inf") if mse == 0 else 10 * math.log10(peak * peak / mse)


def test_transfer_loop_static_style_vs_oracle_loop():
    """50 steps, F = 16, 16x16 latents (the geometry of test_transfer_loop_vs_reference_golden) on a repeated style: the static loop and the existing
    loop against the oracle's loop, PSNR >= 40 dB each; static against existing is printed, not bounded.  One-frame style latents ([1,4,1,h,w]) and
    F-frame ones give the static loop the same result bit for bit."""
    from univst_amd import engine
    from univst_amd.backbones.video_diffusion_sd import pnp_utils
    from univst_amd.schedulers import DDIMScheduler
    unet, sd, cfg = model("sd1")
    F, h, w, n = 16, 16, 16, 50
    pipe = types.SimpleNamespace(unet=unet, scheduler=DDIMScheduler())
    ci = [si.content_latent(k, F, h, w) for k in range(n + 1)]
    s1 = [si.style_latent(k, 1, h, w) for k in range(n + 1)]
    sy = [t.expand(-1, -1, F, -1, -1).contiguous() for t in s1]
    text3 = si.text_embedding(cfg["cross_attention_dim"]).expand(3, -1, -1).contiguous().half().cuda()
    lat0 = pnp_utils.latent_adain(ci[n].half().cuda(), sy[n].half().cuda())
    static = engine.transfer_loop(pipe, lat0, text3, ci, s1, None, n, static_style=True)
    static_f = engine.transfer_loop(pipe, lat0, text3, ci, sy, None, n, static_style=True)
    plain = engine.transfer_loop(pipe, lat0, text3, ci, sy, None, n)
    assert torch.equal(static, static_f)
    dsd = {k: v.cuda() for k, v in sd.items()}
    ctx = text3.float()
    osch = pipeline_ref.DDIMSchedule()
    osch.set_timesteps(n)
    with torch.no_grad():
        ref = pipeline_ref.video_style_transfer_loop(
            lambda x, t, i: unet_ref.unet_forward(dsd, cfg, x.cuda(), int(t), ctx, pnp_idx=i, exact_temporal=False)[0].cpu(),
            osch, unet_ref.latent_adain(ci[n].half().float(), sy[n].half().float()), [t.half().float() for t in ci],
            [t.half().float() for t in sy], None, n)
    ref = ref[0] if isinstance(ref, (tuple, list)) else ref
    ps, pp, sp = psnr(static, ref), psnr(plain, ref), psnr(static, plain)
    print(f"transfer loop PSNR vs oracle: static {ps:.2f} dB, existing {pp:.2f} dB; static vs existing {sp:.2f} dB")
    assert ps >= 40.0 and pp >= 40.0, (ps, pp)
    with pytest.raises(NotImplementedError, match="static_style"):
        engine.transfer_loop(pipe, lat0, text3, ci, s1, None, n, static_style=True, shard=types.SimpleNamespace(world=2, frames=F))


def test_one_frame_inversion_equals_frame_0_of_three_copies():
    from univst_amd import engine
    from univst_amd.schedulers import DDIMScheduler
    unet, sd, cfg = model("sd1")
    h, w = 16, 24
    z1 = (0.7 * si.style_latent(0, 1, h, w)).half().cuda()
    z3 = z1.expand(-1, -1, 3, -1, -1).contiguous()
    ctx = si.text_embedding(cfg["cross_attention_dim"]).half().cuda()
    pipe = types.SimpleNamespace(unet=unet)
    out = []
    for z in (z1, z3):
        sched = DDIMScheduler()
        sched.set_timesteps(50)
        out.append(engine.inversion_loop(pipe, sched, z, ctx, 5, False))
    assert len(out[0]) == 6 and tuple(out[0][5].shape) == (1, 4, 1, h, w)
    mx = max(errs(a, b[:, :, :1])[0] for a, b in zip(out[0][1:], out[1][1:]))
    print(f"one-frame inversion vs frame 0 of three copies, 5 steps: max {mx:.3e} of max|ref|")
    assert mx < 5e-3, mx


# ------------------------------------------------------------------------------------------------ f: refusals
def _raw_calls(handle, cfg, pnp, bank, bank_bytes, F=2, h=16, w=16):
    """both entries on sentinel-filled buffers -> (rc bank, rc forward, messages, buffers untouched)"""
    from univst_amd import _native
    lib = _native.load()
    D = cfg["cross_attention_dim"]
    x1, x2 = torch.zeros(1, 4, 1, h, w).half().cuda(), torch.zeros(2, 4, F, h, w).half().cuda()
    t1, t2 = torch.zeros(1, 77, D).half().cuda(), torch.zeros(2, 77, D).half().cuda()
    eps = torch.full((2, 4, F, h, w), 7.0, dtype=torch.float16, device="cuda")
    before = bank.clone() if bank is not None else None
    active = C.c_int(-7)
    pp = C.byref(pnp) if pnp is not None else None
    rb = lib.univst_unet_style_bank(handle, x1.data_ptr(), float(T), t1.data_ptr(), h, w, 77, pp, bank.data_ptr() if bank is not None else None,
                                    bank_bytes, C.byref(active), _native.stream_ptr())
    mb = lib.univst_last_error().decode()
    rf = lib.univst_unet_forward_static_style(handle, x2.data_ptr(), float(T), t2.data_ptr(), F, h, w, 77, pp,
                                              bank.data_ptr() if bank is not None else None, bank_bytes, eps.data_ptr(), _native.stream_ptr())
    mf = lib.univst_last_error().decode()
    torch.cuda.synchronize()
    clean = bool((eps == 7.0).all()) and (bank is None or torch.equal(bank, before))
    return rb, rf, mb, mf, clean


def test_refusals_return_their_code_before_any_launch():
    from univst_amd import _native
    lib = _native.load()
    ARG, UNSUPPORTED = -1, -3
    unet, sd, cfg = model("sd1")
    unet._sync_native()
    h = unet._native_handle
    size = lib.univst_unet_style_bank_bytes(h, 16, 16)
    assert size > 0 and lib.univst_unet_style_bank_bytes(h, 12, 16) == ARG
    bank = torch.full((size,), 0x5A, dtype=torch.uint8, device="cuda")
    inside = _native.PnP(1, 5, 0.0, 0.5, 0.65, 3.0)
    # the bank call without a registered PnP state; the forward is then the ordinary one (not refused): its eps is written
    for pnp in (None, _native.PnP(0, 5, 0.0, 0.5, 0.65, 3.0)):
        rb, rf, mb, _, _ = _raw_calls(h, cfg, pnp, bank, size)
        assert rb == ARG and "registered" in mb and rf == 0, (rb, rf, mb)
        assert (bank == 0x5A).all()
    # a bank that is too small, and a NULL bank with the window open
    rb, rf, mb, mf, clean = _raw_calls(h, cfg, inside, bank[:size - 256], size - 256)
    assert rb == ARG and rf == ARG and "bytes" in mb and "bytes" in mf and clean, (rb, rf, mb, mf, clean)
    rb, rf, mb, mf, clean = _raw_calls(h, cfg, inside, None, 0)
    assert rb == ARG and rf == ARG and "NULL" in mb and "NULL" in mf and clean, (rb, rf, mb, mf, clean)
    # a communicator attached (world 2 through the callback entry; detached again with world 1)
    ws = torch.zeros(1 << 18, dtype=torch.uint8, device="cuda")
    ar_fn, kv_fn = _native.ALLREDUCE_FN(lambda *a: 0), _native.KVEXCHANGE_FN(lambda *a: 0)
    assert lib.univst_unet_set_comm(h, 0, 2, ws.data_ptr(), ws.numel(), ar_fn, kv_fn, None) == 0
    try:
        rb, rf, mb, mf, clean = _raw_calls(h, cfg, inside, bank, size)
    finally:
        assert lib.univst_unet_set_comm(h, 0, 1, None, 0, _native.ALLREDUCE_FN(), _native.KVEXCHANGE_FN(), None) == 0
    assert rb == UNSUPPORTED and rf == UNSUPPORTED and "communicator" in mb and "communicator" in mf and clean, (rb, rf, mb, mf, clean)
    # trained temporal layers
    tr, _, _ = model("trained")
    tr._sync_native()
    rb, rf, mb, mf, clean = _raw_calls(tr._native_handle, cfg, inside, bank, size)
    assert rb == UNSUPPORTED and rf == UNSUPPORTED and "trained temporal" in mb and "trained temporal" in mf and clean, (rb, rf, mb, mf, clean)
    set_idx(tr, 5)
    with pytest.raises(RuntimeError, match="trained temporal"):
        tr.style_bank(torch.zeros(1, 4, 1, 16, 16).half().cuda(), T, torch.zeros(1, 77, cfg["cross_attention_dim"]).half().cuda())
    # a handle of univst_unet_create_animatediff (no weights needed: refused by its kind)
    boc = cfg["block_out_channels"]
    ucfg = _native.UnetCfg(4, 4, (C.c_int * 4)(*boc), 2, cfg["cross_attention_dim"], (C.c_int * 4)(2, 2, 2, 2), cfg["norm_num_groups"], 1e-5, 1, 0.0)
    ad = _native.AnimateDiffCfg()
    ah = C.c_void_p()
    assert lib.univst_unet_create_animatediff(C.byref(ucfg), C.byref(ad), C.byref(ah)) == 0, lib.univst_last_error()
    try:
        rb, rf, mb, mf, clean = _raw_calls(ah, cfg, inside, bank, size)
    finally:
        lib.univst_unet_destroy(ah)
    assert rb == UNSUPPORTED and rf == UNSUPPORTED and "AnimateDiff" in mb and "AnimateDiff" in mf and clean, (rb, rf, mb, mf, clean)
    # the handle is still good
    rb, rf, _, _, _ = _raw_calls(h, cfg, inside, bank, size)
    assert rb == 0 and rf == 0
