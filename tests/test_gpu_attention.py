"""GPU: every kernel of the attention launch table (csrc/attention.hip: ATTN_KERNELS, 61 instantiations) through the C ABI (univst_attention,
univst_attention_phase; explicit strides), element by element against float64 softmax(q k^T / sqrt(d) + ln(multiplicity)) v on the same fp16
inputs (oracle/attention_ref.py: reference; never the kernel's own output or another kernel's).  The cases, one smallest problem per symbol, and
their three data families: oracle/attention_cases.py; that each case selects the kernel it is named for, that the cases give exactly the launch
table, that a float32 / fp16 emulation of the kernels meets the bounds below and that the planted defects move the result by more than 8 bounds:
tests/test_attention_cases.py (no GPU).  Every test here checks the plan line first (the debug entry is host only).

The bound (attention_ref.bound).  u = 2^-24 is one float32 rounding, x_j the score of key j in log2 units (q.k c + lw, c = log2(e) / sqrt(d)), s_j the
float64 probabilities, ref = sum_j s_j v_j, T the number of 64-key tiles the launch walks, N its keys, L = sum_j 2^(x_j - max x) >= 1.

  store     `(half_t)(o * inv)`: 2^-11 |ref| + 2^-25.
  packed    the probabilities reach the PV MFMA as fp16.  Where they are v_cvt_pkrtz results (attn_body CF and ONES, both pipelined kernels, the text
            kernel) each is up to 2^-10 low, and the denominator sums those same packed values (the ones column of V, fdot2 against (1, 1), the
            text kernel's float sum of the halves): numerator and denominator carry the same weights s_j (1 - e_j), 0 <= e_j <= 2^-10, and the
            quotient is off by at most 2^-10 sum_j s_j |v_j - ref|.  attn_body without CF and without the ones column (`rs += e`, `(half_t)e`) sums
            the UNROUNDED exponentials and rounds the probabilities to nearest: 2^-11 sum_j s_j |v_j|.
  scores    a relative error rho on s_j, common to numerator and denominator, so rho sum_j s_j |v_j - ref|:
                rho = ln2 u (KS + 5) (max_j c sum_i |q_i k_ji| + max_j |x_j| + 8 + max |lw|) + 2^-22 [+ ln2 max |lw - fp16(lw)|]
            KS chained 16x16x32 MFMAs accumulate exact fp16 products in fp32 (one rounding of the running sum each, at most three inside), then
            `fmaf(sc, c, mc)` with mc = fmaf(-mrun, c, lw) (two roundings, c itself rounded) or, prescaled, the reference as MFMA accumulator / as
            two fp16 columns of Q' (exact: a multiple of 8 plus a multiple of 1/64): KS + 5 roundings of numbers no larger than the products'
            absolute sum plus the reference, which lies within DEFER = 8 of a score; v_exp_f32 is good to 1 ulp: 2^-22 with the rounding of its
            argument.  attn_pp40_kernel carries lw in an fp16 column of Q' (set_lw): the bracketed term, 2.4e-4 at lw = log2(3).
  PV        fp32: 2 MFMAs per tile onto O^T (one rounding of the running sum each, at most three inside), and at most one deferred rescale per
            tile (exp2 + product: 5 u): u (7 T + 3) sum_j s_j |v_j|; the denominator likewise, with 16 additions per lane and tile and two shuffles
            where it is summed on the VALU: u (21 T + 6) |ref|, which also covers 1 / l and the product of the store line.
  dropped   a probability below 2^-14 of the running reference is packed as an fp16 subnormal or as 0: 2^-24 absolute each, in units of a reference
            that only rises and ends no more than 1/128 above the maximum (the quantised references): 1.01 2^-24 sum_j (|v_j| + |ref|) / L.
  two-phase the merge reads the phase-1 rows as fp16: w1 (2^-11 |ref1| + 2^-25) with w1 the float64 weight of the first phase; its coefficients
            (attn_merge_coef: two exp2, a sum, 1 / den, two products; the state's own rounding) cost (2^-21 + ln2 u (|lse1| + |lse2| + 16)) (w1 |ref1|
            + w2 |ref2|).  Every key is packed once, in whichever launch, so the packed term is taken around the rows over the UNION.
  state     |m + log2(l) - lse| <= (2^-10 [packed kernels] + rho + u (21 T + 6) + 1.01 2^-24 N / L) / ln2 + 4 u (|lse| + max|x| + 8 + max|lw|).

On unit-scale data the store and the packed term are of one size and everything else is below a tenth of them.  On top, for every random case,
the whole-tensor figures of test_gpu_ops.py::test_attention_two_phase_error_is_rounding_level: relative rms < 6e-4, max < 2.5e-3 of the maximum.

The uniform family (q = 0, integer V, multiplicities 1, 2, 4) has exact sums: the store + 4 u |ref| (1 / l and the product) remain.  The
one-hot family must return the selected V row bit for bit.  A merge kernel runs these two families behind an EMPTY first phase (state 0, rows 3.0).

The state of a two-phase attention is "the reference of the exponentials and the denominator w.r.t. it"; the merge uses nothing narrower
(attn_merge_coef takes any m1 with l1 2^(m1 - m) in range), so the synthetic first phase runs with m at the row maximum and 2.6 above / 3.3 below.

Worst max(err / bound) per kernel family over its cases, CPU emulation | MI355X (the emulation keeps the kernels' packing, tile order and
deferred reference, so where those decide the worst element is the same one):

                                  one launch / first phase    state             merge, synthetic   chained           uniform
    attn_body plain (RTN, rs)     0.833 | 0.842               0.091 | 0.112     0.929 | 0.929      0.743 | 0.729     0.822 | 0.822
    attn_body ONES (d = 40)       0.904 | 0.904               0.639 | 0.702     0.849 | 0.849      0.789 | 0.789     0.822 | 0.822
    attn_body CF                  0.885 | 0.885               0.867 | 0.868     0.945 | 0.945      0.888 | 0.888     0.822 | 0.822
    attn_pp40_kernel<0,1,true>    0.930 | 0.930               0.911 | 0.912     0.899 | 0.898      0.851 | 0.851     0.822 | 0.822
    attn_pp40_kernel<1,0,false>   0.949 | 0.949                                                                      0.648 | 0.648
    attn_pp64_kernel              0.939 | 0.939               0.920 | 0.920     0.918 | 0.918      0.864 | 0.864     0.822 | 0.822
    attn_text_kernel              0.979 | 0.979                                                                      0.740 | 0.740

The state bound of the plain body is ten times what it shows: its l sums unrounded exponentials, so only the scores term is left, and that is
sized for the worst query of the case.  The one-hot family is bit-exact on all 75 cases; the worst whole-tensor figures of the random family
are rms 2.8e-4 and max 6.6e-4.

Every output has 4 guard rows behind it and 8 pad columns beside every row (ldo = C + 8), filled with -7, which must come back untouched —
through the merge launch too, which reads and rewrites `out`.  A second run has NaN in every element of the fused q | k | v buffer that the
launch may not read (q columns of rows past BF Nq; k | v columns of every source block that no src_idx row of THIS launch names within its
src_cnt: always block 3, which no table names) and must give the same bits, as must a repeated launch.  Every test prints its figures (pytest -s) before it asserts and repeats them in the assertion message."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import attention_cases as ac  # noqa: E402
from oracle import attention_ref as ar  # noqa: E402

GUARD_ROWS, GUARD_VALUE = 4, -7.0
RMS_MAX, ABS_MAX = 6e-4, 2.5e-3


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def _plan_is(nat, c, sym, phase=None):
    buf = C.create_string_buffer(4096)
    rc = nat.load().univst_debug_attention_plan(*ac.plan_args(c, phase), buf, 4096)
    line = buf.value.decode()
    assert rc == 0 and line.split(" ")[0] == sym, (c.name, sym, rc, line)
    return line


def _launch(nat, p, phase=0, buf=None, state_in=None, rows_in=None):
    """one launch of problem p through the C ABI: q, k, v are column slices of the fused buffer (ldq = ldkv = 3C), the output has ldo = C + 8
    and guard rows.  -> (rows fp16 [BF, Nq, C], state float32 [BF, heads, Nq, 2] or None), numpy; the guards are checked here."""
    c, Cc = p.case, p.C
    rows = c.BF * c.Nq
    x = torch.from_numpy(p.buf if buf is None else buf).cuda()
    assert x.is_contiguous() and x.shape[1] == 3 * Cc
    out = torch.full((rows + GUARD_ROWS, Cc + ac.PAD), GUARD_VALUE, dtype=torch.float16, device="cuda")
    if rows_in is not None:
        out[:rows, :Cc] = torch.from_numpy(rows_in.reshape(rows, Cc)).cuda()
    idx = torch.from_numpy(p.src_idx).cuda()
    cnt = None if p.src_cnt is None else torch.from_numpy(p.src_cnt).cuda()
    lw = None if p.src_logw is None else torch.from_numpy(p.src_logw).contiguous().cuda()
    q, k, v = x.data_ptr(), x.data_ptr() + 2 * Cc, x.data_ptr() + 4 * Cc
    lib, state = nat.load(), None
    if phase == 0:
        rc = lib.univst_attention(q, 3 * Cc, k, v, 3 * Cc, out.data_ptr(), Cc + ac.PAD, idx.data_ptr(), nat.ptr(cnt), nat.ptr(lw), p.nsrc, c.BF, c.Nq,
                                  c.Nkv, c.heads, c.d, int(p.pre), nat.stream_ptr())
    else:
        assert cnt is not None
        if phase == 1:
            state = torch.full((c.BF, c.heads, c.Nq, 2), float("nan"), dtype=torch.float32, device="cuda")
        sin = None if phase == 1 else torch.from_numpy(np.ascontiguousarray(state_in)).cuda()
        rc = lib.univst_attention_phase(q, 3 * Cc, k, v, 3 * Cc, out.data_ptr(), Cc + ac.PAD, idx.data_ptr(), cnt.data_ptr(), nat.ptr(lw), p.nsrc, c.BF,
                                        c.Nq, c.Nkv, c.heads, c.d, int(p.pre), nat.ptr(state), nat.ptr(sin), nat.stream_ptr())
    nat.check(rc, f"attention {c.name} phase {phase}")
    torch.cuda.synchronize()
    assert (out[rows:] == GUARD_VALUE).all(), f"{c.name}: rows behind the output were written"
    assert (out[:, Cc:] == GUARD_VALUE).all(), f"{c.name}: pad columns beside the output rows were written"
    got = out[:rows, :Cc].cpu().numpy().reshape(c.BF, c.Nq, Cc)
    return got, None if state is None else state.cpu().numpy()


def _same(a, b):
    return np.array_equal(a.view(np.int16), b.view(np.int16))


def _run(nat, p, phase=0, **kw):
    """_launch, twice, and once more on the NaN-poisoned buffer: identical bits (rows and state)"""
    got, st = _launch(nat, p, phase, **kw)
    again, st2 = _launch(nat, p, phase, **kw)
    assert _same(got, again) and (st is None or np.array_equal(st.view(np.int32), st2.view(np.int32))), f"{p.case.name}: two launches differ"
    pois, st3 = _launch(nat, p, phase, buf=ac.poisoned(p), **kw)
    assert _same(got, pois) and (st is None or np.array_equal(st.view(np.int32), st3.view(np.int32))), \
        f"{p.case.name}: NaN in elements the launch must not read changed the result"
    return got, st


def _judge(what, got, ref, bnd, backstop=False):
    """got fp16, ref / bnd float64 [BF, Nq, C]: print, then assert finite and max(err / bound) <= 1 (and the whole-tensor figures) -> the ratio"""
    assert got.shape == ref.shape and got.dtype == np.float16, (what, got.shape, ref.shape)
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(np.isnan(err / bnd), np.inf, err / bnd)
    i = tuple(int(t) for t in np.unravel_index(int(ratio.argmax()), ratio.shape))
    rms, mx = float(np.sqrt((err ** 2).mean() / max((ref ** 2).mean(), 1e-300))), float(err.max() / max(np.abs(ref).max(), 1e-300))
    msg = (f"{what}: max(err / bound) = {ratio.max():.4f} at (frame, query, column) {i}: got {float(got[i]):.6g}, ref {ref[i]:.6g}; "
           f"max err {err.max():.3e}; rms {rms:.2e} of the rms, max {mx:.2e} of the maximum")
    print(msg)
    assert np.isfinite(got.astype(np.float32)).all(), msg
    assert ratio.max() <= 1.0, msg
    if backstop:
        assert rms < RMS_MAX and mx < ABS_MAX, msg
    return float(ratio.max())


def _exact_family_launch(nat, name, family):
    """a uniform / one-hot problem through the case's own kernel: one launch, a first phase, or a merge behind an empty first phase"""
    c = ac.CASES[name]
    p = ac.build(name, family, "full" if c.phase else None)
    _plan_is(nat, c, c.sym)
    kw = {}
    if c.phase == 2:
        kw = dict(state_in=np.zeros((c.BF, c.heads, c.Nq, 2), dtype=np.float32), rows_in=np.full((c.BF, c.Nq, p.C), 3.0, dtype=np.float16))
    got, _ = _run(nat, p, c.phase, **kw)
    return p, got


# ------------------------------------------------------------------------------------------------ one launch
@pytest.mark.parametrize("name", ac.of_phase(0))
def test_random_case_against_float64(nat, name):
    c = ac.CASES[name]
    p = ac.build(name, "random")
    line = _plan_is(nat, c, c.sym)
    got, _ = _run(nat, p)
    r = ar.reference(p)
    _judge(f"{name} [{line}]", got, r.out, ar.bound(p, r, ar.traits(c.sym)), backstop=True)
    if c.Nkv == 1:                  # one key: the output is that V row
        want = np.stack([p.v16()[p.sources(bf)[0][0]].transpose(1, 0, 2).reshape(1, p.C).repeat(c.Nq, 0) for bf in range(c.BF)])
        assert _same(got, np.ascontiguousarray(want)), f"{name}: one key, and the output is not its V row"


@pytest.mark.parametrize("name", list(ac.CASES))
def test_uniform_case_is_the_mean_to_one_rounding(nat, name):
    p, got = _exact_family_launch(nat, name, "uniform")
    r = ar.reference(p)
    _judge(f"{name} uniform [{p.case.sym}]", got, r.out, ac.uniform_bound(p, r))


@pytest.mark.parametrize("name", list(ac.CASES))
def test_onehot_case_returns_the_selected_row(nat, name):
    p, got = _exact_family_launch(nat, name, "onehot")
    want = ac.selected_rows(p)
    bad = np.argwhere(got.view(np.int16) != want.view(np.int16))
    msg = f"{name} one-hot [{p.case.sym}]: {len(bad)} elements differ from the selected V row"
    if len(bad):
        bf, i, col = (int(t) for t in bad[0])
        h = col // p.case.d
        msg += (f"; first at (frame, query, column) {(bf, i, col)}: got {float(got[bf, i, col])}, want {float(want[bf, i, col])} = V of (source block, key) "
                f"{tuple(p.select[bf, h, i])}, head {h}; rows affected: {len({(int(a), int(b)) for a, b, _ in bad})}")
    print(msg)
    assert not len(bad), msg


# ------------------------------------------------------------------------------------------------ the two-phase kernels, each on its own
def _state_lse(st):
    with np.errstate(divide="ignore"):
        return st[..., 0].astype(np.float64) + np.log2(st[..., 1].astype(np.float64))


@pytest.mark.parametrize("name", ac.of_phase(1))
def test_first_phase_rows_and_state(nat, name):
    """TP = 1: rows against float64 over this launch's sources, m + log2(l) against the float64 log-sum-exp; a frame with src_cnt == 0 gets zero
    rows and l == 0 exactly"""
    c = ac.CASES[name]
    tr = ar.traits(c.sym)
    line = _plan_is(nat, c, c.sym)
    p = ac.build(name, "random", "full")
    got, st = _run(nat, p, 1)
    r = ar.reference(p)
    sr = np.abs(_state_lse(st) - r.lse) / ar.state_bound(p, r, tr)
    sr = float(np.where(np.isnan(sr), np.inf, sr).max())
    print(f"{name} [{line}]: state max(err / bound) = {sr:.4f}")
    _judge(f"{name} [{line}]", got, r.out, ar.bound(p, r, tr), backstop=True)
    assert sr <= 1.0, (name, sr)
    pe = ac.build(name, "random", "empty")
    gote, ste = _run(nat, pe, 1)
    empty = [bf for bf in range(c.BF) if not pe.sources(bf)]
    assert empty
    for bf in empty:
        assert not gote[bf].view(np.int16).any() and not ste[bf].view(np.int32)[..., 1].any() and np.isfinite(ste[bf]).all(), \
            f"{name}: frame {bf} has no source: its rows and l must be exactly 0"
    re_ = ar.reference(pe)
    keep = [bf for bf in range(c.BF) if bf not in empty]
    _judge(f"{name}, frame 0 without sources", gote[keep], re_.out[keep], ar.bound(pe, re_, tr)[keep])


@pytest.mark.parametrize("name", ac.of_phase(2))
def test_merge_on_a_synthetic_first_phase(nat, name):
    """TP = 2 behind a first phase made from float64 (rows rounded to fp16, m + log2 l = the float64 log-sum-exp): a wrong merge cannot be
    cancelled by a matching wrong first phase.  m at the row maximum, 2.6 above and 3.3 below it; a frame with src_cnt == 0 keeps its rows"""
    c = ac.CASES[name]
    tr = ar.traits(c.sym)
    line = _plan_is(nat, c, c.sym)
    p1 = ac.build(name, "random", "full")
    p2 = ac.merge_problem(p1, "full")
    r1, r2 = ar.reference(p1), ar.reference(p2)
    want, bnd = ar.merge_bound(p1, r1, r2, tr)
    rows1 = r1.out.astype(np.float16)
    worst = 0.0
    for shift in (0.0, 2.6, -3.3):
        launch = _run if shift == 0.0 else _launch
        got, _ = launch(nat, p2, 2, state_in=ar.synthetic_state(r1, shift), rows_in=rows1)
        worst = max(worst, _judge(f"{name} [{line}] m + {shift}", got, want, bnd, backstop=True))
    pe = ac.merge_problem(p1, "empty")
    gote, _ = _launch(nat, pe, 2, state_in=ar.synthetic_state(r1), rows_in=rows1)
    re_ = ar.reference(pe)
    wante, bnde = ar.merge_bound(p1, r1, re_, tr)
    for bf in range(c.BF):
        if not pe.sources(bf):
            assert _same(gote[bf], rows1[bf]), f"{name}: frame {bf} has no source in the merge launch: its rows must stay bit for bit"
        else:
            _judge(f"{name}, merge with frame 0 kept", gote[bf:bf + 1], wante[bf:bf + 1], bnde[bf:bf + 1])


@pytest.mark.parametrize("name", ac.of_phase(2))
def test_two_launches_chained(nat, name):
    """TP = 1 then TP = 2 against float64 over the union of the sources"""
    c = ac.CASES[name]
    first = ac.chain_first_symbol(c)
    _plan_is(nat, c, first, phase=1)
    line = _plan_is(nat, c, c.sym)
    p1 = ac.build(name, "random", "full")
    p2 = ac.merge_problem(p1, "full")
    rows1, st = _launch(nat, p1, 1)
    got, _ = _run(nat, p2, 2, state_in=st, rows_in=rows1)
    r1, r2 = ar.reference(p1), ar.reference(p2)
    union = ar.reference(p1, frames=[p1.sources(bf) + p2.sources(bf) for bf in range(c.BF)])
    _judge(f"{name} [{first} + {line}]", got, union.out, ar.chained_bound(p1, r1, r2, union, ar.traits(first), ar.traits(c.sym)), backstop=True)
