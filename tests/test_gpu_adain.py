"""GPU: every path of the AdaIN kernels — the UNet plugin's attention shift (csrc/pnp.hip: colstats_kernel, adain_shift_kernel<1 / 2 / 4>),
the SD3 plugin's (csrc/sd3.hip: sd3_group_stats_kernel, sd3_shift_kernel), the latent AdaIN in one launch and as the frame shard's
stats -> sum -> apply pair — through the C ABI, element by element against float64 (oracle/adain_ref.py), plus the elementwise helpers of
the loop.  The cases, their sentinel rows and what each is for: oracle/adain_cases.py; that they take the paths they are named for, that a
float32 emulation of the kernels meets the bounds below, and that the defects they are there to catch move the reference by more than 8
bounds: tests/test_adain_cases.py (no GPU).

The bounds follow the kernels' arithmetic.  For a K / V output element of the UNet shift, with r = 1 / sqrt(var + eps) of the stylised row,
m_s / sigma_s the style column statistics, A the row's mean |x| and K = max(C / 64, N / 32) + 16:

    T     = beta (|x - mu| r sigma_s + |m_s|) + (1 - beta) |sty|
    bound = 2^-11 |ref| + K 2^-24 (T + beta r sigma_s A + 4 beta sigma_s) + 2^-25

2^-11 |ref| + 2^-25: the store `o[e] = (half_t)(...)` rounds to the nearest fp16 (half the smallest subnormal step absolute).  K: every fp32
sum is short before a fixed-order merge — adain_shift_kernel adds at most 8 MAXCH = C / 64 elements per lane (`s += (float)x[i][e]`,
`q += dlt * dlt`) before wave_sum, colstats_kernel at most N / 32 rows per phase (`s[e] += t; q[e] += t * t`) before the merge in double
— so a sum is off by at most that count times 2^-24 of its sum of magnitudes; the + 16 holds the 6 additions of wave_sum and the fewer
than 10 roundings of `ad = (x - mu) * rstd * sp + mp`, `beta * ad + (1 - beta) * sty`, each on a term no larger than T.  K 2^-24 T: the
relative error of rstd (half that of `wave_sum(q) / C`) and of sigma_s (half that of m2) multiply |x - mu| r sigma_s <= T / beta, the one of
m_s (the pivoted sum `st / nt`, whose magnitudes are |x - pivot|, well under |m_s| + 4 sigma_s — hence the last term) its own size.
beta r sigma_s A: the error of `mu = wave_sum(s) / C`, at most K 2^-24 A, passes through r sigma_s beta.  For Q,
`gamma * (alpha * a + (1 - alpha) * b)` is 4 roundings (1 - alpha, two products and the sum, gamma) of terms <= gamma (alpha |q0| + (1 -
alpha) |q2|) <= |q0| + 3 |q2| for the alpha, gamma in use: 2^-11 |ref| + 4 * 2^-24 (|q0| + 3 |q2|) + 2^-25.

SD3 shift: the same form with K = N / 32 + 16 (sd3_shift_kernel has no row sums: both statistics come from colstats) and A = 2 mean |x| of
the (frame, head) group: mu_g is the mean of d column means, each off by the pivoted sum's K 2^-24 mean |x - pivot| <= K 2^-24 (mean |x| +
|pivot|).  The group variance is E[x^2] - mean_g^2 in double from the fp32 column statistics; the rounding of a column mean m_c enters as
N m_c^2 in the first term and through mean_g^2 in the second and cancels to first order (8e-9 relative at mean 200, std 0.25), so it
needs no rho^2 term.  The entry has no width limit (C = 2432 is SD3.5-large), so the C = 2056 refusal is the UNet entry's alone.

Latent AdaIN, out = (c - cmu) crstd sstd + smu, z = |c - cmu| r sstd, A_c / A_s the mean |content| of the channel / mean |style| of the
(channel, frame), K = max(n, 1024) / 1024 + 16 (each of the 1024 threads adds n / 1024 elements before wave_sum; 16 wave totals in double):

    one launch:   2^-11 |ref| + K 2^-24 (z + r sstd A_c + A_s) + 2^-25
    stats/apply:  the same + z ((rho_c^2 + 8) + (rho_s^2 + 8)) 2^-25

latent_adain_kernel is two-pass: crstd and sstd are off by K 2^-24 relative (on z), cmu by K 2^-24 A_c (through r sstd), smu by K 2^-24 A_s.
The pair takes the content variance as sumsq / n - mean^2 from fp32 (sum, sumsq) that cross the all-reduce: one rounding of sumsq is
(1 + rho_c^2) 2^-24 of the variance, half of it on rstd, rho_c = |cmu| / sigma_c, as in the GroupNorm bound.  latent_adain_apply_kernel takes
the style sums in one pass about the frame's first element s[0]: rho_s = |s[0] - smu| / sstd.  (It used to take raw sum(x), sum(x^2): the
emulation of that put the constant style frame of lv_const_style_frame_odd at 1.43 bounds with sstd = 2e-4 instead of 0, and nothing held
the variance of a frame with |mean| >> std.  The pivot makes a constant frame's sums exactly 0.)

Every ratio is err / bound against float64 on the same fp16 inputs, never against the kernel's own output.  Where the store dominates the
ratio sits just under 1 by construction.  max(err / bound), CPU float32 emulation | MI355X:

    UNet shift (Q, K|V)           emulation       MI355X          SD3 shift (Q, K|V)              emulation       MI355X
    g1_n2_empty_phases            0.810  0.917    0.810  0.917    s1_smallest                     0.775  0.855    0.775  0.855
    g2_ragged_rows_partial_cols   0.946  0.982    0.946  0.982    s2_two_stats_blocks             0.999  0.987    0.999  0.987
    g3_phases_of_2_and_1_rows     0.993  0.983    0.993  0.983    s3_d8_idle_lanes                0.999  0.969    0.999  0.969
    g4_one_phase_unrolled         0.998  0.984    0.998  0.984    s4_sd35_large_text              0.999  0.973    0.999  0.973
    g5_inst2_12_tail_phases       0.999  0.983    0.999  0.983    s5_ragged_rows_partial_cols     0.916  0.969    0.916  0.969
    g6_two_unrolled_nch3          0.999  0.982    0.999  0.982    sv_mean30                       0.999  0.993    0.999  0.993
    g7_inst4_c1280                0.999  0.985    0.999  0.985    sv_mean800                      0.514  0.638    0.514  0.638
    g8_width_limit                0.999  0.985    0.999  0.985    latent (one launch, worst pair) emulation       MI355X
    g9_4096_blocks                0.999  0.965    0.999  0.965    l1_hw6                          0.787  0.786    0.787  0.786
    v_mean30                      0.774  0.992    0.774  0.992    l2_odd                          0.982  0.981    0.982  0.981
    v_mean800                     0.856  0.639    0.856  0.639    l3_sd3_call_hw1056              0.992  0.992    0.992  0.991
    v_const_row                   0.999  0.987    0.999  0.987    l4_16_frames_hw64               0.984  0.983    0.984  0.983
    v_const_col                   0.999  0.987    0.999  0.987    l5_hw4096                       0.983  0.982    0.983  0.982
                                                                  lv_mean3_odd                    0.942  0.942    0.942  0.942
                                                                  lv_mean3_hw4096                 0.978  0.976    0.978  0.976
                                                                  lv_const_style_frame_odd        0.925  0.923    0.925  0.923
                                                                  lv_const_style_frame_hw4096     0.988  0.987    0.988  0.987

The non-store part of the bound is 0.5 % .. 4.6 % of the store part at the median K | V element of the UNet cases (11.9 % at N = 4096),
0.6 % .. 6.6 % for SD3 and 0.5 % .. 2.7 % for the latent cases, sentinels included (tests/test_adain_cases.py asserts <= 25 % on every case):
one fp16 rounding plus a margin that cannot hide a wrong element.

Every test prints its figures (pytest -s) before it asserts and repeats them in the assertion message."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import adain_cases as ac  # noqa: E402


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def _shift(nat, b, qkv):
    """in place on qkv (a GPU tensor or view); -> (mean, std) of the UNet entry, None for SD3"""
    c = b.case
    if b.sd3:
        nat.sd3_adain_shift_(qkv, c.F, c.N, c.C, c.heads, *ac.shift_args(b))
        return None
    _, mean, std = nat.attention_adain_shift_(qkv, c.F, c.N, c.C, *ac.shift_args(b), return_stats=True)
    return mean, std


def _run_shift(nat, b):
    qkv = b.qkv.cuda()
    stats = _shift(nat, b, qkv)
    torch.cuda.synchronize()
    return qkv.cpu(), None if stats is None else tuple(t.cpu() for t in stats)


def _check_shift(nat, name):
    b = ac.build_shift(name)
    c = b.case
    F, N, C = c.F, c.N, c.C
    FN = F * N
    want = ac.EXPECT[name]
    assert {k: b.path[k] for k in want} == want, b.path                                  # the path this case is here for
    got, stats = _run_shift(nat, b)
    again, _ = _run_shift(nat, b)
    assert got.shape == b.qkv.shape and got.dtype == torch.float16
    assert torch.equal(got, again), f"{name}: two runs of the same call differ"          # fixed reduction orders
    assert torch.equal(got[:2 * FN], b.qkv[:2 * FN]), f"{name}: content / style rows must be bit-untouched"
    out = got[2 * FN:]
    ref = b.ref.out[2 * FN:]
    err = (out.double() - ref).abs()
    ratio = err / ac.shift_bound(b)
    worst = int(ratio.argmax())
    row, col = divmod(worst, 3 * C)
    msg = (f"{name}: max(err / bound) Q {ratio[:, :C].max().item():.3f}  K|V {ratio[:, C:].max().item():.3f}; worst at row {row} (frame {row // N}, "
           f"token {row % N}) column {col} ({'qkv'[col // C]} {col % C}): got {out[row, col].item():.6g}, ref {ref[row, col].item():.6g}; "
           f"max err {err.max().item():.3e}; path {b.path}")
    print(msg)
    assert torch.isfinite(out).all(), msg
    assert ratio.max().item() <= 1.0, msg
    if stats is not None:                                                                # the style statistics the kernel used
        mean, std = (t.double() for t in stats)
        scale = b.qkv[FN:2 * FN, C:].double().abs().max().item()
        em = ((mean - b.ref.mean).abs() / scale).max().item()
        pos = b.ref.std > 0
        es = (std[pos] / b.ref.std[pos] - 1).abs().max().item()
        smsg = f"{name}: style statistics: mean off by {em:.2e} of the scale {scale:.4g}, std by {es:.2e} relative"
        print(smsg)
        assert mean.shape == b.ref.mean.shape == (F, 2 * C) and em < 1e-6 and es < 1e-4, smsg
        assert (std[~pos] == 0).all(), f"{name}: a column that is constant over N has std 0"
    return b, out


@pytest.mark.parametrize("name", list(ac.SHIFT_CASES))
def test_attention_adain_shift_case_against_float64(nat, name):
    """One case of oracle/adain_cases.SHIFT_CASES: two identical runs, finite, max(err / bound) <= 1 against float64, the returned style
    statistics, untouched content and style rows; the constant row and the constant column are within one fp16 step of their closed forms."""
    b, out = _check_shift(nat, name)
    c = b.case
    if c.values == "const_row":              # LayerNorm of zero variance: x - mu = 0, the output is beta m_s + (1 - beta) sty
        for f, r in ac.CONST_ROWS:
            want = ac.BETA * b.ref.mean[f] + (1.0 - ac.BETA) * b.ref.sty[f, r].reshape(-1)
            off = ((out[f * c.N + r, c.C:].double() - want).abs() / ac.fp16_step(want)).max().item()
            print(f"{name}: constant row ({f}, {r}): max |got - (beta m_s + (1 - beta) sty)| = {off:.3f} fp16 steps")
            assert off <= 1.0, (name, f, r, off)
    if c.values == "const_col":              # sigma_s = 0 and m_s = sty = the constant: the output is the constant
        for col in ac.CONST_COLS:
            want = torch.full((c.F * c.N,), ac.CONST_COL_VALUE, dtype=torch.float64)
            off = ((out[:, c.C + col].double() - want).abs() / ac.fp16_step(want)).max().item()
            print(f"{name}: constant column {col}: max |got - {ac.CONST_COL_VALUE}| = {off:.3f} fp16 steps")
            assert off <= 1.0, (name, col, off)


@pytest.mark.parametrize("name", list(ac.SD3_CASES))
def test_sd3_adain_shift_case_against_float64(nat, name):
    _check_shift(nat, name)


@pytest.mark.parametrize("name", [ac.LD_CASE, ac.SD3_LD_CASE])
def test_shift_leading_dimension(nat, name):
    """ld = 3C + 24: a column-sliced view of a wider buffer, its pad columns and 40 rows behind it filled with NaN.  The pad stays
    bit-identical, and the result equals the ld = 3C run bit for bit."""
    b = ac.build_shift(name)
    c = b.case
    rows, ld = 3 * c.F * c.N, 3 * c.C + ac.LD_PAD
    dense = b.qkv.cuda()
    _shift(nat, b, dense)
    buf = torch.full((rows + ac.LD_TAIL_ROWS, ld), float("nan"), dtype=torch.float16, device="cuda")
    buf[:rows, :3 * c.C] = b.qkv.cuda()
    before = buf.clone()
    view = buf[:rows, :3 * c.C]
    assert view.stride() == (ld, 1) and not view.is_contiguous()
    _shift(nat, b, view)
    torch.cuda.synchronize()
    assert torch.equal(view, dense), f"{name}: ld = {ld} and ld = {3 * c.C} differ"
    assert torch.isfinite(view).all()
    raw = lambda t: t.view(torch.int16)
    assert torch.equal(raw(buf[:rows, 3 * c.C:]), raw(before[:rows, 3 * c.C:])), f"{name}: pad columns were written"
    assert torch.equal(raw(buf[rows:]), raw(before[rows:])), f"{name}: rows behind the buffer were written"
    with pytest.raises(ValueError, match="unit column stride"):
        _shift(nat, b, buf[:rows, ::2])


# F, N, C, heads, ld, what the message names
_REFUSALS = [
    ("c_mod_8", dict(C=36, ld=112), r"C=36"),
    ("c_2056", dict(C=2056, ld=6168), r"C=2056"),
    ("ld_mod_8", dict(C=40, ld=124), r"ld=124"),
    ("ld_below_3c", dict(C=40, ld=112), r"ld=112"),
    ("f_0", dict(F=0), r"F=0"),
    ("n_0", dict(N=0), r"N=0"),
    ("sd3_n_1", dict(N=1), r"N=1"),
    ("sd3_c_mod_heads", dict(C=40, heads=3, ld=120), r"heads=3"),
]


# C = 2056 is the UNet entry's limit alone (the SD3 kernels have no width limit: C = 2432 is one of their cases); N = 1 and C % heads are SD3's
_REFUSED = [("unet",) + r for r in _REFUSALS if not r[0].startswith("sd3_")] + [("sd3",) + r for r in _REFUSALS if r[0] != "c_2056"]


@pytest.mark.parametrize("entry,tag,args,names", _REFUSED, ids=[f"{r[0]}-{r[1]}" for r in _REFUSED])
def test_shift_entries_refuse_before_any_launch(nat, entry, tag, args, names):
    """a refused call names the value and writes nothing: the - 7 filled buffer and workspace are untouched after a synchronize"""
    a = dict(F=2, N=5, C=40, heads=5, ld=120)
    a.update(args)
    buf = torch.full((3 * 2 * 5 + 8, 6200), -7.0, dtype=torch.float16, device="cuda")
    ws = torch.full((1 << 16,), -7.0, dtype=torch.float32, device="cuda")
    lib = nat.load()
    if entry == "unet":
        rc = lib.univst_attention_adain_shift(buf.data_ptr(), a["ld"], a["F"], a["N"], a["C"], ac.ALPHA, ac.BETA, ac.GAMMA, ws.data_ptr(), nat.stream_ptr())
    else:
        rc = lib.univst_sd3_adain_shift(buf.data_ptr(), a["ld"], a["F"], a["N"], a["C"], a["heads"], ac.SD3_ALPHA, ac.BETA, ac.SD3_GAMMA, ws.data_ptr(),
                                        nat.stream_ptr())
    assert rc != 0, (entry, tag, a)
    with pytest.raises(RuntimeError, match=names):
        nat.check(rc, entry)
    torch.cuda.synchronize()
    assert (buf == -7).all() and (ws == -7).all(), (entry, tag, "a refused call wrote")


# ------------------------------------------------------------------------------------------------ latent AdaIN
def _latent_msg(name, what, got, b, bnd):
    err = (got.double() - b.ref.out).abs()
    ratio = err / bnd
    i = int(ratio.argmax())
    c = b.case
    ch, rem = divmod(i, c.F * c.h * c.w)
    f, px = divmod(rem, c.h * c.w)
    return ratio.max().item(), (f"{name}: {what}: max(err / bound) = {ratio.max().item():.3f} at channel {ch} frame {f} pixel {px}: got "
                                f"{got.reshape(-1)[i].item():.6g}, ref {b.ref.out.reshape(-1)[i].item():.6g}; max err {err.max().item():.3e}")


def _pair(nat, b, shards):
    """stats per shard, a float32 sum of the [C, 2] results (the all-reduce), apply per shard"""
    c = b.case
    Fl = c.F // shards
    cnt = [b.cnt[:, :, k * Fl:(k + 1) * Fl].contiguous().cuda() for k in range(shards)]
    sty = [b.sty[:, :, k * Fl:(k + 1) * Fl].contiguous().cuda() for k in range(shards)]
    st = [nat.latent_adain_stats(x) for x in cnt]
    assert st[0].shape == (c.C, 2) and st[0].dtype == torch.float32
    total = st[0].clone()
    for s in st[1:]:
        total += s
    out = [nat.latent_adain_apply(x, y, total, c.F * c.h * c.w) for x, y in zip(cnt, sty)]
    torch.cuda.synchronize()
    return torch.cat([o.cpu() for o in out], dim=2)


@pytest.mark.parametrize("name", list(ac.LATENT_CASES))
def test_latent_adain_case_against_float64(nat, name):
    """the one-launch kernel and the stats -> sum -> apply pair at 1, 2 and F shards: two identical runs, finite, max(err / bound) <= 1;
    one shard equals the one-launch kernel within 2 bounds; a constant style frame comes out as the constant"""
    b = ac.build_latent(name)
    c = b.case
    want = ac.LATENT_EXPECT.get(name, {})
    assert {k: b.path[k] for k in want} == want, b.path
    run = lambda: nat.latent_adain(b.cnt.cuda(), b.sty.cuda()).cpu()
    one = run()
    assert torch.equal(one, run()), f"{name}: two runs of the same call differ"
    assert one.shape == b.cnt.shape and one.dtype == torch.float16
    bnd1, bnd2 = ac.latent_bound(b), ac.latent_bound(b, pair=True)
    r, msg = _latent_msg(name, "one launch", one, b, bnd1)
    print(msg)
    assert torch.isfinite(one).all() and r <= 1.0, msg
    outs = {"one launch": one}
    for k in ac.shard_counts(c.F):
        got = _pair(nat, b, k)
        assert torch.equal(got, _pair(nat, b, k)), f"{name}: two runs of the {k}-shard pair differ"
        r, msg = _latent_msg(name, f"{k} shard{'s' if k > 1 else ''}", got, b, bnd2)
        print(msg)
        assert torch.isfinite(got).all() and r <= 1.0, msg
        outs[k] = got
    d = ((outs[1].double() - one.double()).abs() / bnd2).max().item()
    print(f"{name}: one shard vs one launch: {d:.3f} bounds")
    assert d <= 2.0, (name, d)
    if c.values == "const_style_frame":
        want = torch.tensor(ac.CONST_STYLE_VALUE).half().double()
        for what, o in outs.items():
            off = ((o[:, :, ac.CONST_STYLE_FRAME].double() - want).abs() / ac.fp16_step(want)).max().item()
            print(f"{name}: {what}: constant style frame off by {off:.3f} fp16 steps")
            assert off <= 1.0, (name, what, off)


def test_latent_adain_apply_refuses_what_it_cannot_read(nat):
    b = ac.build_latent("l2_odd")
    cnt, sty = b.cnt.cuda(), b.sty.cuda()
    st = nat.latent_adain_stats(cnt)
    with pytest.raises(ValueError):
        nat.latent_adain_stats(cnt[:, :, 1:])                                  # a frame slice is not contiguous
    with pytest.raises(ValueError):
        nat.latent_adain_apply(cnt, sty[:, :2], st, 105)
    with pytest.raises(ValueError):
        nat.latent_adain_apply(cnt, sty, st.double(), 105)
    with pytest.raises(RuntimeError, match="latent_adain_apply"):
        nat.latent_adain_apply(cnt, sty, st, 0)


# ------------------------------------------------------------------------------------------------ the loop's elementwise helpers
def _ew_check(what, got, ref, terms):
    bnd = 2.0 ** -11 * ref.abs() + 4 * 2.0 ** -24 * terms
    ratio = ((got.double().cpu() - ref).abs() / bnd.clamp_min(1e-300)).max().item()
    msg = f"{what}: max(err / bound) = {ratio:.3f}"
    print(msg)
    assert torch.isfinite(got).all() and ratio <= 1.0, msg


@pytest.mark.parametrize("fhw", [(1, 1, 1), (1, 3, 85), (1, 1, 257)], ids=["n1", "n255", "n257"])
def test_axpby_axpbypcz_mask_blend_against_float64(nat, fhw):
    """n = 1, 255 and 257 elements per channel (one thread, one short of a 256-thread block, one over): 2^-11 |ref| + 4 * 2^-24 sum |terms|"""
    g = torch.Generator().manual_seed(31 + fhw[2])
    shape = (1, 3, *fhw)
    x, y, z = (torch.randn(shape, generator=g).half() for _ in range(3))
    m = torch.rand(fhw, generator=g).half()
    xd, yd, zd, md = x.double(), y.double(), z.double(), m.double()
    X, Y, Z = x.cuda(), y.cuda(), z.cuda()
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float32))                # the coefficient the kernel is given
    a, b_, c_ = f32(0.97), f32(-0.13), f32(0.41)
    _ew_check("axpby", nat.axpby(X, Y, a, b_), a * xd + b_ * yd, (a * xd).abs() + (b_ * yd).abs())
    _ew_check("axpbypcz", nat.axpbypcz(X, Y, Z, a, b_, c_), a * xd + b_ * yd + c_ * zd, (a * xd).abs() + (b_ * yd).abs() + (c_ * zd).abs())
    _ew_check("mask_blend", nat.mask_blend(X, Y, m.cuda()), (1 - md) * xd + md * yd, ((1 - md) * xd).abs() + (md * yd).abs())
    got = nat.mask_blend(X, Y, None)
    _ew_check("mask_blend, no mask", got, xd, xd.abs())
    assert torch.equal(got.cpu(), x)


def _bilinear64(m, h, w):
    """float64 bilinear resize of [F, H, W] to [F, h, w], align_corners=False (source coordinate (i + 0.5) H / h - 0.5, clamped at 0)"""
    F, H, W = m.shape
    m = m.double()

    def axis(n_out, n_in):
        s = ((torch.arange(n_out, dtype=torch.float64) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0.0)
        i0 = s.floor().long().clamp_max(n_in - 1)
        i1 = (i0 + 1).clamp_max(n_in - 1)
        return i0, i1, s - i0
    y0, y1, ly = axis(h, H)
    x0, x1, lx = axis(w, W)
    top = m[:, y0][:, :, x0] * (1 - lx) + m[:, y0][:, :, x1] * lx
    bot = m[:, y1][:, :, x0] * (1 - lx) + m[:, y1][:, :, x1] * lx
    return top * (1 - ly)[None, :, None] + bot * ly[None, :, None]


@pytest.mark.parametrize("H,W,h,w", [(20, 36, 5, 7), (3, 5, 7, 4), (16, 16, 2, 2)])
def test_mask_resize_against_float64(nat, H, W, h, w):
    """20x36 -> 5x7 (a scale of 36 / 7), 3x5 -> 7x4 (upsampling: the clamp at 0 and the last-row guard), 16x16 -> 2x2 (exact) to 2^-11"""
    g = torch.Generator().manual_seed(H * 100 + W)
    m = (torch.rand(2, H, W, generator=g) > 0.5).to(torch.uint8)
    ref = _bilinear64(m, h, w)
    assert (ref - torch.nn.functional.interpolate(m[None].double(), size=(h, w), mode="bilinear", align_corners=False)[0]).abs().max().item() < 1e-12
    got = nat.mask_resize(m.cuda(), h, w).cpu()
    err = (got.double() - ref).abs().max().item()
    print(f"mask_resize {H}x{W} -> {h}x{w}: max err {err:.3e}")
    assert got.shape == (2, h, w) and torch.isfinite(got).all() and err <= 2.0 ** -11, err
    if (H, W, h, w) == (16, 16, 2, 2):
        assert torch.equal(got.double(), ref), "quarters are exact in fp16"
