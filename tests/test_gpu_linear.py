"""GPU: every linear (mode 0) kernel of the GEMM launch table (csrc/gemm.hip: GEMM_KERNELS, 16 of its 23 instantiations) and splitk_reduce_kernel through
the C ABI (univst_linear, univst_linear_epi, univst_linear_gated, univst_linear_ln, univst_linear_sets), element by element against a float64
reference on the same fp16 / fp32 inputs (oracle/gemm_ref.py; never the kernel's own output or another kernel's).  The cases, one smallest ragged
problem per symbol and per plan output (split-K, register epilogue, tile order, weight sets), and their three data families: oracle/gemm_cases.py.
That each case selects the kernel it is named for on 256 compute units, that the cases give exactly the linear part of the launch table, that a
float32 / fp16 emulation of the kernels meets the bounds and that 15 planted defects each show: tests/test_gemm_cases.py (no GPU).

Every test first reads the plan for the DEVICE's compute-unit count (the debug entry is host only) and fails, without launching, when it names another
kernel, split count, epilogue form or tile order than the case is for.

The bounds are gemm_ref.bound's (its docstring derives every term); nothing is fitted to what the GPU gives.  random: max(err / bound) <= 1; integer and
onehot: bit for bit; statistics of a producer: under their bound against the float64 sums of the rows AS STORED, exact on the integer family.

Layout and poison, every launch: ldx = K + 8, ldr = N + 16, ldy = N + 8 (N + 1, N where the case says so), ld_gate = N + 24, ldrb = N + 8; 8 guard rows
in front of and behind Y and the statistics, filled with -7, which come back untouched like every pad column of Y; NaN in every pad column of X, R, gate
and rowbias, in 8 rows behind X, R, W, the statistics the kernel reads, in the elements behind bias, bias2, ln_wsum, ln_bias, in the row behind rowbias
and gate and in weight set S and its fp32 bias (one past the last): no NaN may reach an output.  Every launch runs twice into fresh buffers: the same
bits (the split order and the statistics order are fixed).  Split-K through univst_linear_epi: a workspace of exactly splits * M * N * 4 bytes is
used (it comes back without its NaN), one 4 bytes short is left alone (the launcher takes its own scratch); both give the bits of a launch without one.

N % 4 != 0 and an odd ldy are supported (include/univst.h): the 128-wide epilogue then stores 8 bytes at 2-byte aligned addresses, which global memory
accesses of gfx950 allow; s42_n98 / s42_n98_ldy98 / big3_ldy_odd check the values.

Worst max(err / bound) of the random family per path, float32 emulation | MI355X (the store rounding decides the worst element of every case, so the
two agree to four digits; pytest -s prints every figure):

    direct 256x320   plain 0.9864 | 0.9864   MM-DiT 0.9938 | 0.9938   LayerNorm fold 0.9692 | 0.9692   GEGLU 0.9677 | 0.9677   weight sets 0.9862 | 0.9862
                     register epilogue 0.9905 | 0.9905   tile orders 0.8164 | 0.8164
    X-resident       0.8127 | 0.8127
    128-wide         plain 0.9847 | 0.9847   MM-DiT 0.9819 | 0.9819   LayerNorm fold 0.9545 | 0.9545   GEGLU 0.9699 | 0.9699
    split-K          256x320 (K = 8200) 0.1953 | 0.1953, with GELU, gate and residual 0.8246 | 0.8246; 128-wide (K = 4104) 0.3355 | 0.3355, with gate and
                     residual 0.8458 | 0.8458 — the K-proportional term is loose there: the integer family holds these cases
    statistics       0.1422 | 0.1283

Integer and one-hot: bit-exact on all 39 cases they apply to.  No kernel defect showed."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import gemm_cases as gc  # noqa: E402
from oracle import gemm_ref as gr  # noqa: E402

GUARD_ROWS, GUARD_VALUE = 8, -7.0
ACT_NONE, ACT_GELU_TANH = -1, 1
NAN = float("nan")


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def _sync(what):
    """a GPU fault ends the session: nothing more is launched on a device that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"{what}: {e}", returncode=3)


def _plan_is(nat, c):
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    buf = C.create_string_buffer(4096)
    rc = nat.load().univst_debug_gemm_plan(*gc.plan_args(c, ncu), buf, 4096)
    line = buf.value.decode()
    assert rc == 0, f"{c.name}: the plan on {ncu} compute units refuses the case: {line}"
    q = gc.parse_plan(line)
    assert (q.sym, q.splits, q.epi, q.tgn, q.tgm) == (c.sym, c.splits, c.epi, c.tgn, c.tgm), \
        f"{c.name} is the case of {c.sym} (splits {c.splits}, epi_lds {c.epi}, tile order {c.tgn} x {c.tgm}), but on {ncu} compute units the plan is [{line}]: not testing another kernel in its place"
    return line


def _dev(a, ld=None, rows_behind=0):
    """a host array on the device, NaN in the pad columns (rows ld apart) and in rows_behind further rows (a 1-D array: that many further elements)"""
    a = np.asarray(a)
    if a.ndim == 1:
        out = np.full(a.shape[0] + rows_behind, NAN, dtype=a.dtype)
        out[:a.shape[0]] = a
    else:
        a2 = a.reshape(a.shape[0], -1)
        out = np.full((a2.shape[0] + rows_behind, ld or a2.shape[1]), NAN, dtype=a.dtype)
        out[:a2.shape[0], :a2.shape[1]] = a2
    return torch.from_numpy(out).cuda()


def _operands(p):
    """every input of problem p on the device, laid out and poisoned as the module docstring says"""
    c, lay = p.case, gc.layout(p.case)
    d = dict(X=_dev(p.x, lay.ldx, 8), W=_dev(p.w.reshape(-1, p.K), None, p.N))                 # behind W: one whole weight set of NaN
    for key, a in (("bias", p.bias), ("bias2", p.bias2), ("ln_wsum", p.ln_wsum), ("ln_bias", p.ln_bias)):
        d[key] = None if a is None else _dev(a, None, 64)
    d["bias32"] = None if p.bias32 is None else _dev(p.bias32, None, 1)
    d["R"] = None if p.R is None else _dev(p.R, lay.ldr, 8)
    d["rowbias"] = None if p.rowbias is None else _dev(p.rowbias, lay.ldrb, 1)
    d["gate"] = None if p.gate is None else _dev(p.gate, lay.ld_gate, 1)
    d["ln_stats"] = None if p.ln_stats is None else _dev(p.ln_stats, None, 8)
    return d


def _launch(nat, p, d, workspace=None, force_epi=False):
    """one launch into fresh output buffers -> (y fp16 [M, No], stats float32 [M, N / 160, 2] or None); guards and pads are checked here"""
    c, lay, lib = p.case, gc.layout(p.case), nat.load()
    M, N, K, No, G = p.M, p.N, p.K, p.No, GUARD_ROWS
    off = 4 if c.yoff else 0                                       # Y 8 bytes off a 16-byte boundary
    flat = torch.full((off + (M + 2 * G) * lay.ldy + 8,), GUARD_VALUE, dtype=torch.float16, device="cuda")
    rows = flat[off:off + (M + 2 * G) * lay.ldy].view(M + 2 * G, lay.ldy)
    Y = rows[G].data_ptr()
    assert (Y % 16 == 8) == c.yoff
    stats = torch.full((M + 2 * G, N // 160, 2), GUARD_VALUE, dtype=torch.float32, device="cuda") if p.stats_out else None
    st_ptr = None if stats is None else stats[G].data_ptr()
    ptr, s = nat.ptr, nat.stream_ptr()
    common = (ptr(d["X"]), lay.ldx, ptr(d["W"]))
    if c.sets:
        rc = lib.univst_linear_sets(*common, ptr(d["bias32"]), c.sets, ptr(d["R"]), lay.ldr, Y, lay.ldy, M, N, K, st_ptr, s)
    elif p.ln_stats is not None or p.stats_out:
        rc = lib.univst_linear_ln(*common, ptr(d["bias"]), ptr(d["R"]), lay.ldr, Y, lay.ldy, M, N, K, c.geglu, ptr(d["ln_stats"]), p.ln_eps, ptr(d["ln_wsum"]),
                                  ptr(d["ln_bias"]), st_ptr, s)
    elif p.act or p.gate is not None:
        rc = lib.univst_linear_gated(*common, ptr(d["bias"]), ptr(d["R"]), lay.ldr, Y, lay.ldy, M, N, K, ACT_GELU_TANH if p.act else ACT_NONE, ptr(d["gate"]),
                                     lay.ld_gate, p.rows_per_gate, s)
    elif p.rowbias is not None or p.bias2 is not None or workspace is not None or force_epi:
        rc = lib.univst_linear_epi(*common, ptr(d["bias"]), ptr(d["R"]), lay.ldr, Y, lay.ldy, M, N, K, c.geglu, ptr(d["rowbias"]), p.rows_per_rb, lay.ldrb,
                                   ptr(d["bias2"]), ptr(workspace), 0 if workspace is None else workspace.numel() * 4, s)
    else:
        rc = lib.univst_linear(*common, ptr(d["bias"]), ptr(d["R"]), lay.ldr, Y, lay.ldy, M, N, K, c.geglu, s)
    nat.check(rc, f"linear {c.name}")
    _sync(c.name)
    got = rows[G:G + M, :No].cpu().numpy()
    rows[G:G + M, :No] = GUARD_VALUE
    assert bool((flat == GUARD_VALUE).all()), f"{c.name}: guard rows around Y or pad columns beside its rows were written"
    st = None
    if stats is not None:
        st = stats[G:G + M].cpu().numpy()
        assert bool((stats[:G] == GUARD_VALUE).all()) and bool((stats[G + M:] == GUARD_VALUE).all()), f"{c.name}: rows around the statistics were written"
        assert np.isfinite(st).all(), f"{c.name}: non-finite statistics"
    assert np.isfinite(got.astype(np.float32)).all(), f"{c.name}: a NaN from an element the launch must not read, or an overflow, reached the output"
    return np.ascontiguousarray(got), st


def _bits(a):
    return a.view(np.int16 if a.dtype == np.float16 else np.int32)


def _run(nat, name, family):
    """the plan check, then the launch twice: identical bits -> (p, y, stats, plan line)"""
    c = gc.CASES[name]
    line = _plan_is(nat, c)
    p = gc.build(name, family)
    d = _operands(p)
    y, st = _launch(nat, p, d)
    y2, st2 = _launch(nat, p, d)
    assert np.array_equal(_bits(y), _bits(y2)) and (st is None or np.array_equal(_bits(st), _bits(st2))), f"{name} {family}: two launches differ"
    return p, y, st, line


def _judge_stats(what, st, y, exact):
    want, bnd = gr.stats_ref(y)
    if exact:
        assert np.array_equal(st.astype(np.float64), want), f"{what}: the statistics of integer rows are not exact"
        return
    q = np.abs(st.astype(np.float64) - want) / np.maximum(bnd, 1e-300)
    i = tuple(int(t) for t in np.unravel_index(int(q.argmax()), q.shape))
    msg = f"{what}: statistics max(err / bound) = {q.max():.4f} at (row, slot, sum | sumsq) {i}: got {st[i]:.8g}, the stored row gives {want[i]:.8g}"
    print(msg)
    assert q.max() <= 1.0, msg


RANDOM = [n for n in gc.CASES]
EXACT = [n for n, c in gc.CASES.items() if "integer" in gc.families(c)]


@pytest.mark.parametrize("name", RANDOM)
def test_random_case_against_float64(nat, name):
    p, y, st, line = _run(nat, name, "random")
    r = gr.reference(p)
    q = np.abs(y.astype(np.float64) - r.out) / gr.bound(p, r)
    q = np.where(np.isnan(q), np.inf, q)
    i = tuple(int(t) for t in np.unravel_index(int(q.argmax()), q.shape))
    msg = f"{name} [{line.split(' big_direct')[0]}]: max(err / bound) = {q.max():.4f} at (row, column) {i}: got {float(y[i]):.6g}, ref {r.out[i]:.6g}"
    print(msg)
    assert q.max() <= 1.0, msg
    if st is not None:
        _judge_stats(name, st, y, exact=False)


@pytest.mark.parametrize("name", EXACT)
def test_integer_case_is_bit_exact(nat, name):
    p, y, st, _ = _run(nat, name, "integer")
    want = gr.exact_output(p, gr.reference(p, with_err=False))
    bad = np.argwhere(_bits(y) != _bits(want))
    msg = f"{name} integer [{p.case.sym}]: {len(bad)} of {y.size} outputs differ from fp16 of the exact integer"
    if len(bad):
        i = tuple(int(t) for t in bad[0])
        msg += f"; first at (row, column) {i}: got {float(y[i])}, want {float(want[i])}; rows affected: {len(set(bad[:, 0].tolist()))}, columns: {len(set(bad[:, 1].tolist()))}"
    print(msg)
    assert not len(bad), msg
    if st is not None:
        _judge_stats(name, st, y, exact=True)


@pytest.mark.parametrize("name", EXACT)
def test_onehot_case_returns_the_selected_weight(nat, name):
    p, y, st, _ = _run(nat, name, "onehot")
    want = gc.onehot_output(p)
    bad = np.argwhere(_bits(y) != _bits(want))
    msg = f"{name} one-hot [{p.case.sym}]: {len(bad)} of {y.size} outputs differ from W[n][k(m)]"
    if len(bad):
        m, n = (int(t) for t in bad[0])
        k = int(gc.onehot_k(p.case)[m])
        read = np.nonzero(p.w[gr.row_set(p)[m], n] == y[m, n])[0].tolist()
        msg += (f"; first at (row, column) {(m, n)}: got {float(y[m, n])}, want {float(want[m, n])} = W[{n}][{k}]; the k of this weight row with the value "
                f"that came back: {read[:4]}; rows affected: {len(set(bad[:, 0].tolist()))}, columns: {len(set(bad[:, 1].tolist()))}")
    print(msg)
    assert not len(bad), msg
    if st is not None:
        _judge_stats(name, st, y, exact=False)


SPLIT_EPI = [n for n, c in gc.CASES.items() if c.splits > 1 and not (gc.has(c, "a") or gc.has(c, "g"))]


@pytest.mark.parametrize("name", SPLIT_EPI)
def test_split_k_workspace_of_the_caller_and_the_fall_back(nat, name):
    """univst_linear_epi: a workspace of exactly the plan's bytes holds the partials; one 4 bytes short is not touched; the bits are those of a launch without"""
    c = gc.CASES[name]
    _plan_is(nat, c)
    p = gc.build(name, "integer")
    d = _operands(p)
    floats = c.splits * p.M * p.N
    y, _ = _launch(nat, p, d, force_epi=True)
    ws = torch.full((floats,), NAN, dtype=torch.float32, device="cuda")
    y_ws, _ = _launch(nat, p, d, workspace=ws)
    assert bool(torch.isfinite(ws).all()), f"{name}: a workspace of exactly {floats * 4} bytes was not used (or not filled)"
    short = torch.full((floats - 1,), NAN, dtype=torch.float32, device="cuda")
    y_short, _ = _launch(nat, p, d, workspace=short)
    assert bool(torch.isnan(short).all()), f"{name}: a workspace 4 bytes short of {floats * 4} was written"
    assert np.array_equal(_bits(y), _bits(y_ws)) and np.array_equal(_bits(y), _bits(y_short)), f"{name}: the workspace changes the result"
    assert np.array_equal(_bits(y), _bits(gr.exact_output(p, gr.reference(p, with_err=False)))), f"{name}: not the exact integers"
