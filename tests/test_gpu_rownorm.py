"""GPU: every path of the row-wise normalisations and of the MM-DiT elementwise operators — layernorm_kernel<1,4 / 2,2 / 4,1> (csrc/norm.hip),
adaln_modulate_kernel with one and two outputs, rms_heads_vec_kernel<4 / 8 / 16>, rms_heads_kernel, the q | k pair launch, gate_residual,
SiLU / GELU(tanh), the timestep embedding and patchify / unpatchify (csrc/sd3.hip) — through the C ABI, element by element against float64
(oracle/rownorm_ref.py).  The cases, their sentinels and what each is for: oracle/rownorm_cases.py; that they take the paths they are named
for, that a float32 emulation of the kernels meets the bounds below, and that the defects they are there to catch move the reference by
more than 8 bounds: tests/test_rownorm_cases.py (no GPU).

The bounds follow the kernels' arithmetic; u = 2^-24 is one float32 rounding, and every bound ends in the store `(half_t)(...)`:
2^-11 |ref| + 2^-25 (round to nearest fp16, half the smallest subnormal step absolute).

LayerNorm and adaLN, z = (x - mean) r g + b with r = 1 / sqrt(var + eps), g = gamma or 1 + scale[b], b = beta or shift[b]:

    bound = [|x - mean| r |g| + |b|] 8 u  +  mean_row |x| r |g| K u  +  |z - b| K u  +  store,      K = 8 + adds + 6

adds = 8 x the slots a lane has in use (C / 512 rounded up): `s += (float)v[r][i][e]` adds that many elements in a lane one after the other,
wave_sum adds 6 more (xor 32 .. 1), `/ C` rounds once: the mean is off by at most (adds + 6) u mean_row |x| and passes through r |g| — the
second term.  `q += d * d` sums adds squares, each of a difference with one rounding (2 u on the square, 1 u the product unless it is
contracted into the add), then 6 additions, `/ C`, `+ eps`, and rsqrtf at 1 ulp: under (adds + 14) u on the variance, half of it on r, times
|z - b| — the third term (the error of the mean enters the two-pass variance only squared: there is no rho^2 term as GroupNorm has).  The
store line `((float)v - mean) * rstd * g + b` is four roundings (five with adaLN's `1.f + sc`) on terms no larger than the bracket — the
first term, with 8 for 5.  On unit-scale data the whole is 1.01 x the store; a row of mean 300, sigma 0.5 has 3 .. 5 x the store from the
second term, which is what one float32 rounding of 300 is worth at that sigma.

Per-head RMSNorm, ref = x r w (scale0): |ref| K u + store, K = 8 + adds + 6.  The vec kernel adds 8 squares in a lane (fmaf, exact products
of fp16 values) and log2(LPH) <= 4 in the butterfly, the scalar kernel at most 4 (`ss += v[i] * v[i]`) and 6: with `/ d`, `+ eps` under
(adds + 8) u on the mean square, half of it on r; rsqrtf 1 ulp = 2 u, `* scl0`, and the two or three products of the store line: under 14 u.

gate_residual is one fmaf: store + |ref| u.  SiLU `t / (1 + __expf(-t))`: store + |ref| 8 u.  GELU(tanh): the same + 0.5 |x| 4 u: at x = -5.16
`1.f + tanhf(u)` cancels to about one float32 ulp of 1, so tanhf's own error (absolute, a few 2^-24) times 0.5 |x| is 3.4 store roundings of
the result there.  Timestep embedding, a = t freq, ex = ln(P) j / (half - shift): store + a (ex + 4) 2^-23 + 2^-22: the argument of expf is
off by a few u of ex, the frequency by that plus expf's own ulp, a by one more, and sin / cos move by as much as a does — at t = 981.25 a
value next to a zero crossing is 959 store roundings from float64; 2^-22 is sinf / cosf's own error at |result| <= 1.

Every ratio is err / bound against float64 on the same fp16 inputs, never against the kernel's own output.  Where the store dominates the
ratio sits just under 1 by construction.  Worst max(err / bound) per operator, CPU float32 emulation | MI355X:

    layernorm, 9 geometry cases        0.701 .. 0.989  |  0.701 .. 0.989
    layernorm, mean 300 / -2000        0.402 .. 0.551  |  0.402 .. 0.551
    adaln_modulate (y, y2)             0.814 .. 0.992  |  0.814 .. 0.992
    rmsnorm_heads vec / scalar         0.995 / 0.995   |  0.995 / 0.995
    q | k pair vec / scalar            0.993 / 0.985   |  0.993 / 0.985
    gate_residual                      0.996           |  0.996
    SiLU / GELU(tanh), all fp16        0.9995 / 0.9995 |  0.9995 / 0.9995
    timestep_embedding                 0.964           |  0.964

The device's __expf, tanhf, expf, logf, sinf, cosf and rsqrtf leave the figures where the host's libm puts them (the worst elements are the same
ones: the smallest subnormal input for the activations, t = 999 at dim 256 for the embedding), so no constant above was widened for them.

Every output pointer has guard rows behind it (filled with -7) that must come back untouched; the RMS buffers carry pad columns filled with 0
and then with NaN, which must not change and must not change the result.  Every test prints its figures (pytest -s) before it asserts and
repeats them in the assertion message."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import rownorm_cases as rc  # noqa: E402

GUARD_ROWS, GUARD_VALUE = 4, -7.0


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def _raw(t):
    return t.contiguous().view(torch.int16)


def _guarded(rows, C, dtype=torch.float16):
    """[rows + GUARD_ROWS, C] filled with -7: the call gets the pointer and `rows`"""
    return torch.full((rows + GUARD_ROWS, C), GUARD_VALUE, dtype=dtype, device="cuda")


def _guard_ok(buf, rows, what):
    assert (buf[rows:] == GUARD_VALUE).all(), f"{what}: rows behind the output were written"


def _judge(what, got, ref, bnd, path):
    """got fp16 [rows, C] (cpu), ref / bnd float64: print, then assert finite and max(err / bound) <= 1 -> the ratio"""
    assert got.shape == ref.shape and got.dtype == torch.float16, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    ratio = err / bnd
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    i = int(ratio.argmax())
    row, col = divmod(i, ref.shape[-1])
    msg = (f"{what}: max(err / bound) = {ratio.max().item():.4f} at row {row} column {col}: got {got.reshape(-1)[i].item():.6g}, "
           f"ref {ref.reshape(-1)[i].item():.6g}; max err {err.max().item():.3e}; path {path}")
    print(msg)
    assert torch.isfinite(got).all(), msg
    assert ratio.max().item() <= 1.0, msg
    return ratio.max().item()


def _path_holds(path, want, name):
    assert {k: path[k] for k in want} == want, (name, path)


# ------------------------------------------------------------------------------------------------ layernorm
def _run_ln(nat, b):
    c = b.case
    x, gamma, beta = b.x.cuda(), b.gamma.cuda(), b.beta.cuda()
    out = _guarded(c.rows, c.C)
    nat.check(nat.load().univst_layernorm(x.data_ptr(), out.data_ptr(), gamma.data_ptr(), beta.data_ptr(), c.rows, c.C, rc.LN_EPS, nat.stream_ptr()),
              "layernorm")
    torch.cuda.synchronize()
    _guard_ok(out, c.rows, c.name)
    return out[:c.rows].cpu()


@pytest.mark.parametrize("name", list(rc.LN_CASES))
def test_layernorm_case_against_float64(nat, name):
    """One case of LN_CASES through univst_layernorm: the path, two identical runs, finite, max(err / bound) <= 1, guard rows; the wrapper
    gives the same bits; the two constant rows come out within one fp16 step of beta."""
    b = rc.build_ln(name)
    _path_holds(b.path, rc.LN_EXPECT[name], name)
    got = _run_ln(nat, b)
    assert torch.equal(_raw(got), _raw(_run_ln(nat, b))), f"{name}: two runs of the same call differ"
    assert torch.equal(_raw(got), _raw(nat.layernorm(b.x.cuda(), b.gamma.cuda(), b.beta.cuda(), rc.LN_EPS).cpu())), name
    _judge(f"layernorm {name}", got, b.ref.out, rc.ln_bound(b), b.path)
    if name == rc.LN_CONST_CASE:
        want = b.beta.double()
        for r, v in rc.LN_CONST_ROWS:
            off = ((got[r].double() - want).abs() / rc.fp16_step(want)).max().item()
            print(f"layernorm {name}: constant row {r} (= {v}): max |got - beta| = {off:.3f} fp16 steps")
            assert off <= 1.0, (name, r, off)


# ------------------------------------------------------------------------------------------------ adaln_modulate
def _run_ada(nat, b):
    c = b.case
    rows = rc.ADA_B * rc.ADA_N
    x, mod = b.x.cuda(), b.mod.cuda()
    ch = lambda k: mod[:, k * c.C:(k + 1) * c.C]                          # chunk views, as the model passes them
    y = _guarded(rows, c.C)
    y2 = _guarded(rows, c.C) if c.two else None
    nat.check(nat.load().univst_adaln_modulate(x.data_ptr(), y.data_ptr(), ch(1).data_ptr(), ch(0).data_ptr(), mod.stride(0), rows, rc.ADA_N, c.C,
                                               rc.ADALN_EPS, nat.ptr(y2), ch(7).data_ptr() if c.two else None, ch(6).data_ptr() if c.two else None,
                                               nat.stream_ptr()), "adaln_modulate")
    torch.cuda.synchronize()
    _guard_ok(y, rows, c.name)
    if c.two:
        _guard_ok(y2, rows, c.name + " y2")
    w = nat.adaln_modulate(x.reshape(rc.ADA_B, rc.ADA_N, c.C), ch(1), ch(0), rc.ADALN_EPS, **(dict(scale2=ch(7), shift2=ch(6)) if c.two else {}))
    for a, d in zip(w if c.two else (w,), (y, y2)):                     # the wrapper, on the model's chunk views, gives the same bits
        assert torch.equal(_raw(a.reshape(rows, c.C)), _raw(d[:rows])), c.name
    return y[:rows].cpu(), (y2[:rows].cpu() if c.two else None)


@pytest.mark.parametrize("name", list(rc.ADA_CASES))
def test_adaln_modulate_case_against_float64(nat, name):
    """One case of ADA_CASES (B = 3, N = 5: rows ragged over the blocks, b steps at rows 5 and 10; scale / shift chunk views of [B, 6C] or
    [B, 9C]): the path, two identical runs, finite, max(err / bound) <= 1 for y and for y2, guard rows."""
    b = rc.build_ada(name)
    _path_holds(b.path, rc.ADA_EXPECT[name], name)
    y, y2 = _run_ada(nat, b)
    ya, y2a = _run_ada(nat, b)
    assert torch.equal(_raw(y), _raw(ya)) and (y2 is None or torch.equal(_raw(y2), _raw(y2a))), f"{name}: two runs of the same call differ"
    _judge(f"adaln_modulate {name} y", y, b.ref.out, rc.ada_bound(b), b.path)
    if b.case.two:
        _judge(f"adaln_modulate {name} y2", y2, b.ref2.out, rc.ada_bound(b, b.ref2), b.path)


# ------------------------------------------------------------------------------------------------ rmsnorm_heads
def _rms_buffer(c, x, fill):
    """a flat allocation holding [rows + GUARD_ROWS, ld] from ptr_off halfs in; pad columns and guard rows = fill -> (flat, view)"""
    C, ld = c.heads * c.d, c.heads * c.d + c.pad
    flat = torch.full((c.ptr_off + (c.rows + GUARD_ROWS) * ld,), fill, dtype=torch.float16, device="cuda")
    view = flat[c.ptr_off:].view(c.rows + GUARD_ROWS, ld)
    view[:c.rows, :C] = x.reshape(c.rows, C).cuda()
    return flat, view


def _run_rms(nat, b, fill):
    c = b.case
    C, ld = c.heads * c.d, c.heads * c.d + c.pad
    flat, view = _rms_buffer(c, b.x, fill)
    before = flat.clone()
    assert flat.data_ptr() % 16 == 0 and view.data_ptr() - flat.data_ptr() == 2 * c.ptr_off
    w = b.w.cuda()
    nat.check(nat.load().univst_rmsnorm_heads(view.data_ptr(), ld, c.rows, c.heads, c.d, w.data_ptr(), rc.RMS_EPS, nat.stream_ptr()), "rmsnorm_heads")
    torch.cuda.synchronize()
    keep = torch.ones_like(view, dtype=torch.bool)
    keep[:c.rows, :C] = False                                           # pad columns and guard rows
    bview = before[c.ptr_off:].view(c.rows + GUARD_ROWS, ld)
    assert torch.equal(_raw(view[keep]), _raw(bview[keep])), f"{c.name}: pad columns or rows behind the buffer were written (fill {fill})"
    assert torch.equal(_raw(flat[:c.ptr_off]), _raw(before[:c.ptr_off])), c.name
    return view[:c.rows, :C].cpu()


@pytest.mark.parametrize("name", list(rc.RMS_CASES))
def test_rmsnorm_heads_case_against_float64(nat, name):
    """One case of RMS_CASES through univst_rmsnorm_heads (ld, the pointer offset and the guard rows need the C entry): the path, two
    identical runs, pad columns of 0 and of NaN give the same bits and stay as they are, finite, max(err / bound) <= 1."""
    b = rc.build_rms(name)
    c = b.case
    _path_holds(b.path, rc.rms_expect(c), name)
    got = _run_rms(nat, b, 0.0)
    assert torch.equal(_raw(got), _raw(_run_rms(nat, b, 0.0))), f"{name}: two runs of the same call differ"
    assert torch.equal(_raw(got), _raw(_run_rms(nat, b, float("nan")))), f"{name}: the pad columns reached the result"
    C = c.heads * c.d
    _judge(f"rmsnorm_heads {name}", got, b.ref.out.reshape(c.rows, C), rc.rms_bound(b.ref.out, b.path["adds_per_lane"]).reshape(c.rows, C), b.path)


def _run_pair(nat, b, fill):
    c, C = b.case, b.C
    ld = 3 * C + c.pad
    buf = torch.full((c.rows + GUARD_ROWS, ld), fill, dtype=torch.float16, device="cuda")
    buf[:c.rows, :3 * C] = b.qkv.cuda()
    before = buf.clone()
    nat.rmsnorm_heads_pair_(buf[:c.rows], c.heads, c.d, 0, b.w0.cuda(), C, b.w1.cuda(), rc.RMS_EPS, b.scale0)
    torch.cuda.synchronize()
    assert torch.equal(_raw(buf[:, 2 * C:]), _raw(before[:, 2 * C:])), f"{c.name}: the v columns or the pad were written (fill {fill})"
    assert torch.equal(_raw(buf[c.rows:]), _raw(before[c.rows:])), f"{c.name}: rows behind the buffer were written"
    return buf[:c.rows, :2 * C].cpu()


@pytest.mark.parametrize("name", list(rc.PAIR_CASES))
def test_rmsnorm_heads_pair_case_against_float64(nat, name):
    """One case of PAIR_CASES through univst_rmsnorm_heads_pair on a fused [rows, 3C (+ 8)] buffer, c0 = 0 with w0 and scale0 = log2(e) / sqrt(d),
    c1 = C with w1: one launch of the vec kernel or two of the scalar one; v and the pad bit-identical to the input."""
    b = rc.build_pair(name)
    c, C = b.case, b.C
    _path_holds(b.path, rc.rms_expect(c), name)
    got = _run_pair(nat, b, 0.0)
    assert torch.equal(_raw(got), _raw(_run_pair(nat, b, 0.0))), f"{name}: two runs of the same call differ"
    if c.pad:
        assert torch.equal(_raw(got), _raw(_run_pair(nat, b, float("nan")))), f"{name}: the pad columns reached the result"
    _judge(f"rmsnorm_heads_pair {name}", got, b.ref[:, :2 * C], rc.rms_bound(b.ref[:, :2 * C], b.path["adds_per_lane"]), b.path)


# ------------------------------------------------------------------------------------------------ gate_residual, activation
@pytest.mark.parametrize("C", rc.GATE_C)
def test_gate_residual_against_float64(nat, C):
    """B = 3, N = 5, the gate a chunk view of [B, 6C]: two identical runs, max(err / bound) <= 1, guard rows; `out` aliasing `x` gives the same bits"""
    b = rc.build_gate(C)
    _path_holds(b.path, rc.GATE_EXPECT[C], C)
    rows = rc.ADA_B * rc.ADA_N
    x, y, mod = b.x.cuda(), b.y.cuda(), b.mod.cuda()
    gate = mod[:, 2 * C:3 * C]

    def run(alias):
        out = _guarded(rows, C)
        if alias:
            out[:rows] = x
        nat.check(nat.load().univst_gate_residual(out.data_ptr() if alias else x.data_ptr(), gate.data_ptr(), mod.stride(0), y.data_ptr(), out.data_ptr(),
                                                  rows, rc.ADA_N, C, nat.stream_ptr()), "gate_residual")
        torch.cuda.synchronize()
        _guard_ok(out, rows, f"gate_residual C={C}")
        return out[:rows].cpu()
    got = run(False)
    assert torch.equal(_raw(got), _raw(run(False))), f"C={C}: two runs of the same call differ"
    assert torch.equal(_raw(got), _raw(run(True))), f"C={C}: out aliasing x differs"
    assert torch.equal(_raw(got), _raw(nat.gate_residual(x.reshape(rc.ADA_B, rc.ADA_N, C), gate, y.reshape(rc.ADA_B, rc.ADA_N, C)).reshape(rows, C).cpu()))
    _judge(f"gate_residual C={C}", got, b.ref, rc.gate_bound(b.ref), b.path)


@pytest.mark.parametrize("which", rc.ACT_INPUTS)
@pytest.mark.parametrize("act,what", [(rc.ACT_SILU, "silu"), (rc.ACT_GELU_TANH, "gelu_tanh")])
def test_activation_against_float64(nat, act, what, which):
    """all 63 488 finite fp16 values in one call, and n = 8: two identical runs, max(err / bound) <= 1, the guard; `out` aliasing `x` gives the same bits"""
    b = rc.build_act(which)
    _path_holds(b.path, rc.ACT_EXPECT[which], which)
    n = b.x.numel()
    x = b.x.cuda()

    def run(alias):
        out = torch.full((n + 64,), GUARD_VALUE, dtype=torch.float16, device="cuda")
        if alias:
            out[:n] = x
        nat.check(nat.load().univst_activation(out.data_ptr() if alias else x.data_ptr(), out.data_ptr(), n, act, nat.stream_ptr()), "activation")
        torch.cuda.synchronize()
        assert (out[n:] == GUARD_VALUE).all(), f"{what} {which}: elements behind the output were written"
        return out[:n].cpu()
    got = run(False)
    assert torch.equal(_raw(got), _raw(run(False))), f"{what} {which}: two runs of the same call differ"
    assert torch.equal(_raw(got), _raw(run(True))), f"{what} {which}: out aliasing x differs"
    assert torch.equal(_raw(got), _raw(nat.activation(x, act).cpu()))
    ref = b.ref[act]
    ratio = (got.double() - ref).abs() / rc.act_bound(b.x, ref, act)
    i = int(ratio.argmax())
    print(f"{what} {which}: worst input x = {b.x[i].item()!r}")
    _judge(f"{what} {which}", got.reshape(1, n), ref.reshape(1, n), rc.act_bound(b.x, ref, act).reshape(1, n), b.path)


# ------------------------------------------------------------------------------------------------ timestep embedding, patchify
@pytest.mark.parametrize("name", list(rc.TS_CASES))
def test_timestep_embedding_case_against_float64(nat, name):
    b = rc.build_ts(name)
    c = b.case
    t = b.t.cuda()

    def run():
        out = _guarded(c.B, c.dim)
        nat.check(nat.load().univst_timestep_embedding(t.data_ptr(), out.data_ptr(), c.B, c.dim, c.flip, c.shift, 10000.0, nat.stream_ptr()), "timestep_embedding")
        torch.cuda.synchronize()
        _guard_ok(out, c.B, name)
        return out[:c.B].cpu()
    got = run()
    assert torch.equal(_raw(got), _raw(run())), f"{name}: two runs of the same call differ"
    assert torch.equal(_raw(got), _raw(nat.timestep_embedding(t, c.dim, bool(c.flip), c.shift).cpu()))
    _judge(f"timestep_embedding {name} t = {c.t}", got, b.ref, rc.ts_bound(b), b.path)


@pytest.mark.parametrize("p", rc.PATCHES)
def test_patchify_unpatchify_are_the_index_maps(nat, p):
    """B = 3, C = 16, 8 x 12, patch 1, 2, 4: bit-equal to the index map, both ways, with guard rows behind either output"""
    b = rc.build_patch(p)
    B, C, H, W = rc.PATCH_SHAPE
    nrows, K = b.want_rows.shape
    rows = _guarded(nrows, K)
    lat = b.lat.cuda()
    nat.check(nat.load().univst_sd3_patchify(lat.data_ptr(), rows.data_ptr(), B, C, H, W, p, nat.stream_ptr()), "sd3_patchify")
    out = _guarded(B * C * H, W)
    src = b.rows.cuda()
    nat.check(nat.load().univst_sd3_unpatchify(src.data_ptr(), out.data_ptr(), B, C, H, W, p, nat.stream_ptr()), "sd3_unpatchify")
    torch.cuda.synchronize()
    _guard_ok(rows, nrows, f"patchify {p}")
    _guard_ok(out, B * C * H, f"unpatchify {p}")
    print(f"patch {p}: rows {tuple(b.want_rows.shape)}, path {b.path}")
    assert torch.equal(_raw(rows[:nrows].cpu()), _raw(b.want_rows)), f"patchify {p}"
    assert torch.equal(_raw(out[:B * C * H].cpu().reshape(B, C, H, W)), _raw(b.want_lat)), f"unpatchify {p}"
    assert torch.equal(_raw(nat.sd3_patchify(lat, p).cpu()), _raw(b.want_rows)) and torch.equal(_raw(nat.sd3_unpatchify(src, B, C, H, W, p).cpu()), _raw(b.want_lat))


# ------------------------------------------------------------------------------------------------ refusals
# every one of these is a UV_REQUIRE of the entry itself, ahead of its only launch (csrc/abi.hip: univst_layernorm and uv_launch_layernorm's first
# line; csrc/sd3.hip: the entries below `extern "C"`).  Arguments: a dict over the defaults of the entry; `off`: a pointer moved by that many halfs.
_REFUSALS = [
    ("layernorm", "rows_0", dict(rows=0), "rows=0"),
    ("layernorm", "rows_2_31", dict(rows=2 ** 31), "rows=2147483648"),
    ("layernorm", "c_0", dict(C=0), "C=0"),
    ("layernorm", "c_12", dict(C=12), "C=12"),
    ("layernorm", "c_2056", dict(C=2056), "C=2056"),
    ("rmsnorm_heads", "ld_below_heads_d", dict(ld=184), "ld=184"),
    ("rmsnorm_heads", "d_0", dict(d=0), "head_dim"),
    ("rmsnorm_heads", "d_264", dict(d=264, ld=1024), "head_dim"),
    ("rmsnorm_heads", "rows_0", dict(rows=0), "bad argument"),
    ("rmsnorm_heads_pair", "overlap", dict(c1=96), "c1=96"),
    ("rmsnorm_heads_pair", "c1_past_ld", dict(c1=400), "c1=400"),
    ("rmsnorm_heads_pair", "c0_negative", dict(c0=-8), "c0=-8"),
    ("rmsnorm_heads_pair", "d_264", dict(d=264), "head_dim"),
    ("adaln_modulate", "c_4104", dict(C=4104), "C=4104"),
    ("adaln_modulate", "c_12", dict(C=12), "C=12"),
    ("adaln_modulate", "ld_mod_below_c", dict(ld=56), "ld_mod=56"),
    ("adaln_modulate", "ld_mod_mod_8", dict(ld=388), "ld_mod=388"),
    ("adaln_modulate", "x_misaligned", dict(off_x=4), "16-byte"),
    ("adaln_modulate", "scale_misaligned", dict(off_scale=4), "16-byte"),
    ("adaln_modulate", "y2_misaligned", dict(two=True, off_y2=2), "16-byte"),
    ("adaln_modulate", "y2_without_scale2", dict(two=True, no_scale2=True), "scale2"),
    ("gate_residual", "gate_misaligned", dict(off_gate=4), "16-byte"),
    ("gate_residual", "out_misaligned", dict(off_out=1), "16-byte"),
    ("gate_residual", "c_12", dict(C=12), "bad argument"),
    ("activation", "x_misaligned", dict(off_x=4), "16-byte"),
    ("activation", "out_misaligned", dict(off_out=4), "16-byte"),
    ("activation", "n_12", dict(n=12), "bad argument"),
    ("activation", "act_2", dict(act=2), "bad argument"),
    ("timestep_embedding", "dim_5", dict(dim=5), "bad argument"),
    ("timestep_embedding", "b_0", dict(B=0), "bad argument"),
    ("sd3_patchify", "h_mod_patch", dict(patch=3), "bad argument"),
    ("sd3_unpatchify", "patch_0", dict(patch=0), "bad argument"),
]


@pytest.mark.parametrize("entry,tag,args,names", _REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in _REFUSALS])
def test_entries_refuse_before_any_launch(nat, entry, tag, args, names):
    """a refused call names what is wrong and writes nothing: every buffer it was given is untouched after a synchronize"""
    lib, s = nat.load(), nat.stream_ptr()
    bufs = [torch.full((1 << 15,), GUARD_VALUE, dtype=torch.float16, device="cuda") for _ in range(7)]
    p = lambda i, key=None: bufs[i].data_ptr() + 2 * args.get(key, 0)
    if entry == "layernorm":
        a = dict(rows=5, C=64)
        a.update(args)
        rcode = lib.univst_layernorm(p(0), p(1), p(2), p(3), a["rows"], a["C"], 1e-5, s)
    elif entry == "rmsnorm_heads":
        a = dict(ld=192, rows=5, heads=3, d=64)
        a.update(args)
        rcode = lib.univst_rmsnorm_heads(p(0), a["ld"], a["rows"], a["heads"], a["d"], p(1), 1e-6, s)
    elif entry == "rmsnorm_heads_pair":
        a = dict(ld=392, d=64, c0=0, c1=128)                            # heads 2: blocks [0, 128) and [128, 256) of a [5, 3 * 128 + 8] buffer
        a.update(args)
        rcode = lib.univst_rmsnorm_heads_pair(p(0), a["ld"], 5, 2, a["d"], a["c0"], p(1), a["c1"], p(2), 1e-6, 0.18, s)
    elif entry == "adaln_modulate":
        a = dict(C=64, ld=384)
        a.update(args)
        two = a.get("two", False)
        rcode = lib.univst_adaln_modulate(p(0, "off_x"), p(1), p(2, "off_scale"), p(3), a["ld"], 15, 5, a["C"], 1e-6, p(4, "off_y2") if two else None,
                                          p(5) if two and not a.get("no_scale2") else None, p(6) if two else None, s)
    elif entry == "gate_residual":
        a = dict(C=64)
        a.update(args)
        rcode = lib.univst_gate_residual(p(0), p(1, "off_gate"), 384, p(2), p(3, "off_out"), 15, 5, a["C"], s)
    elif entry == "activation":
        a = dict(n=64, act=0)
        a.update(args)
        rcode = lib.univst_activation(p(0, "off_x"), p(1, "off_out"), a["n"], a["act"], s)
    elif entry == "timestep_embedding":
        a = dict(B=2, dim=6)
        a.update(args)
        t = torch.zeros(4, dtype=torch.float32, device="cuda")
        rcode = lib.univst_timestep_embedding(t.data_ptr(), p(0), a["B"], a["dim"], 1, 0.0, 10000.0, s)
    else:
        fn = lib.univst_sd3_patchify if entry == "sd3_patchify" else lib.univst_sd3_unpatchify
        rcode = fn(p(0), p(1), 3, 16, 8, 12, args["patch"], s)
    assert rcode != 0, (entry, tag)
    with pytest.raises(RuntimeError, match=names):
        nat.check(rcode, entry)
    torch.cuda.synchronize()
    assert all((b == GUARD_VALUE).all() for b in bufs), (entry, tag, "a refused call wrote")
