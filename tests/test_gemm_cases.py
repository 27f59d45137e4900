"""CPU: the cases of tests/test_gpu_linear.py (oracle/gemm_cases.py) and the reference, bounds and emulation they are judged by (oracle/gemm_ref.py).

 - every case goes through univst_debug_gemm_plan at 256 compute units and gives the symbol, the split count (+splitk_reduce), the epilogue form and
   the tile order it is named for; the mode-0 symbols of the cases are exactly the mode-0 symbols of the launch table;
 - every case keeps the tails it exists for;
 - the float32 / fp16 emulation of the kernels meets every bound on the random family (max(err / bound) <= 1, printed) and is bit-exact on the integer
   and one-hot families; the integer family reaches beyond 2048 (at least 0.5 % of the outputs, none at 65504) wherever a case has a residual;
 - the measured error of the GEGLU polynomial is the constant the bound uses;
 - planted defects, applied to the emulation, show on every case they apply to.  HOW each is caught:
       random family, by more than 8 bounds (the margin of the attention self-check)   last_k_dropped, tail_tile_dropped, split_dropped, split_twice,
           no_bias_ragged_tile, rowbias_neighbour, gate_neighbour, set_neighbour, R_with_ldy, stats_unrounded, stats_neighbour_slot, geglu_swapped,
           tile_groups_swapped, ln_next_row — on every case with K < 4096;
       integer family, as a bit mismatch                                               bias2_before_rounding on every case (one rounding apart: no
           bound can see it), and EVERY defect on the cases with K >= 4096, where the K-proportional term of the bound is loose — but for the two
           GELU cases there (big3_splitk_act_gate_res, s54_splitk_act_gate), which have no integer family and must show on the random one;
       stats_unrounded leaves integer data unchanged (fp16 holds those values exactly), so it is a random-family defect at every K (its cases have K <= 160)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import gemm_cases as gc
from oracle import gemm_ref as gr

MARGIN = 8.0


@pytest.fixture(scope="module")
def lib():
    from univst_amd import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native.load()


def _plan(lib, c, ncu=gc.NCU):
    buf = C.create_string_buffer(4096)
    rc = lib.univst_debug_gemm_plan(*gc.plan_args(c, ncu), buf, 4096)
    return rc, buf.value.decode()


@pytest.mark.parametrize("name", list(gc.CASES))
def test_case_selects_the_kernel_it_is_named_for(lib, name):
    c = gc.CASES[name]
    rc, line = _plan(lib, c)
    assert rc == 0, (name, line)
    q = gc.parse_plan(line)
    assert (q.sym, q.splits, q.reduce, q.epi, q.tgn, q.tgm) == (c.sym, c.splits, c.splits > 1, c.epi, c.tgn, c.tgm), (name, line)
    # the C ABI asks a shape predicate before it launches (univst_linear_sets, univst_linear_ln): the case has to pass it, or it could not be run
    f = dict(t.split("=") for t in line.split(" ") if "=" in t)
    if c.sets:
        assert f["big_direct"] == "1", (name, line)
    elif gc.has(c, "s"):
        assert f["fold_producer"] == "1", (name, line)
    if gc.has(c, "l") and c.geglu != 2:
        assert f["geglu_consumer" if c.geglu else "fold_consumer"] == "1", (name, line)


def test_cases_are_the_mode0_launch_table(lib):
    buf = C.create_string_buffer(8192)
    assert lib.univst_debug_gemm_plan(gc.NCU, *([0] * 15), buf, 8192) == 0

    def linear(sym):                      # gemm_big_kernel<MODE,..>, gemm_kernel<NF,MODE,..>; the X-resident kernel is a linear, the LDS-patch kernel a conv
        kernel, args = sym[:-1].split("<")
        at = {"gemm_big_kernel": 0, "gemm_kernel": 1}.get(kernel)
        return kernel == "geglu_xres_kernel" or (at is not None and args.split(",")[at] == "0")
    table = {s for s in buf.value.decode().split(";") if linear(s)}
    mine = {c.sym for c in gc.CASES.values()}
    assert len(table) == 16           # of 23: two X-resident, seven 256x320 and seven 128-wide instantiations
    assert mine == table, f"linear kernels without a case: {sorted(table - mine)}; cases of no kernel: {sorted(mine - table)}"


def test_cases_keep_their_tails():
    for name, c in gc.CASES.items():
        geo = gc.geometry(c)
        if not c.sets:
            assert c.M % 16 != 0 and c.M % geo.tile_m != 0, name                 # an M tail inside a 16-row fragment
        else:
            assert c.M % c.sets == 0 and c.sets % geo.tile_m == 0 and c.M // c.sets >= 3, name
        # a K tail of 8 or 32 (40 at K = 1000); the X-resident kernel exists for K = 320 alone, and order_gn2 (K = 832: the smallest whole number of k
        # tiles that puts a 1920-row weight past the 3 MB at which the plan groups tiles) is there for the tile order, with the K tail left to its two neighbours
        assert c.K % 64 in (8, 32, 40) or (c.geglu == 2 and c.K == 320) or name == "order_gn2", name
        if "ragged_n" in name or name in ("s42_n100", "s42_n98", "s42_n98_ldy98", "s42_plain", "s42_geglu", "s42_gate"):
            assert c.N % geo.tile_n != 0, name
        if c.splits > 1:
            nk, per = (c.K + 63) // 64, gc.ktps(c)
            assert (c.splits - 1) * per < nk <= c.splits * per, name            # every split has k tiles, the last one ends in the K tail ...
            assert nk < c.splits * per or not c.sym.startswith("gemm_big"), name   # ... and is short on the 256x320 tile
        if c.tgm:
            tiles = (c.M + geo.tile_m - 1) // geo.tile_m
            assert tiles > c.tgm and tiles % c.tgm != 0 and c.N // 320 > 4, name   # a ragged last row group
        if c.M > gc.ROWS_PER_BRANCH and (gc.has(c, "w") or gc.has(c, "g")):
            assert gc.ROWS_PER_BRANCH % geo.tile_m != 0, name                       # a tile straddles two rowbias / gate rows
        lay = gc.layout(c)
        assert lay.ldx > c.K and lay.ldr > lay.No and lay.ld_gate > c.N and lay.ldrb > c.N
    assert gc.CASES["s42_n100"].N % 8 != 0 and gc.CASES["s42_n98"].N % 4 != 0
    assert gc.layout(gc.CASES["s42_n98_ldy98"]).ldy == 98 and gc.layout(gc.CASES["big3_ldy_odd"]).ldy % 2 == 1


def test_geglu_polynomial_error_is_the_measured_one():
    worst, at, inside = gr.measure_geglu_erf2()
    print(f"geglu_erf2: largest |error| / max(1, |g| / 5) = {worst:.4e} at g = {at:.6g}; largest |error| over |g| <= 8 = {inside:.4e} (common.h: 2e-6)")
    assert 0.95 * gr.GEGLU_GELU_ERR <= worst <= gr.GEGLU_GELU_ERR
    assert inside <= 2e-6


def _ratio(y, r, bnd):
    q = np.abs(y.astype(np.float64) - r) / bnd
    return float(np.where(np.isnan(q), np.inf, q).max())


def _stats_ratio(st, y):
    want, bnd = gr.stats_ref(y)
    q = np.abs(st.astype(np.float64) - want) / np.maximum(bnd, 1e-300)
    return float(np.where(np.isnan(q), np.inf, q).max())


def _same(a, b):
    return np.array_equal(a.view(np.int16), b.view(np.int16))


def _applies(c, d):
    geo = gc.geometry(c)
    many = c.M > gc.ROWS_PER_BRANCH
    return {"last_k_dropped": True, "tail_tile_dropped": True, "split_dropped": c.splits > 1, "split_twice": c.splits > 1,
            "no_bias_ragged_tile": c.N % geo.tile_n != 0 and (gc.has(c, "b") or c.sets > 0) and not c.geglu,
            "rowbias_neighbour": gc.has(c, "w") and many, "gate_neighbour": gc.has(c, "g") and many, "set_neighbour": c.sets > 0,
            "R_with_ldy": gc.has(c, "r") and geo.ldr != geo.ldy, "bias2_before_rounding": gc.has(c, "2"), "stats_unrounded": gc.has(c, "s"),
            "stats_neighbour_slot": gc.has(c, "s") and c.N >= 320, "geglu_swapped": c.geglu > 0, "tile_groups_swapped": c.tgn > 0,
            "ln_next_row": gc.has(c, "l")}[d]


def _by_integer(c, d):
    """which family has to catch defect d on case c (module docstring)"""
    if "integer" not in gc.families(c) or d == "stats_unrounded":
        return False
    return d == "bias2_before_rounding" or c.K >= 4096


@pytest.mark.parametrize("name", list(gc.CASES))
def test_emulation_meets_the_bounds_and_defects_show(name):
    c = gc.CASES[name]
    geo = gc.geometry(c)
    defects = [d for d in gr.DEFECTS if _applies(c, d)]
    # ---- random family: the emulation is inside the bound, the defects of this family are far outside
    p = gc.build(name, "random")
    r = gr.reference(p)
    bnd = gr.bound(p, r)
    parts = gr.emu_partials(p)
    y, st = gr.emulate(p, parts=parts)
    ratio = _ratio(y, r.out, bnd)
    sratio = _stats_ratio(st, y) if st is not None else 0.0
    print(f"{name} [{c.sym}, splits {c.splits}] random: emulation max(err / bound) = {ratio:.4f}" + (f", statistics {sratio:.4f}" if st is not None else ""))
    assert ratio <= 1.0 and sratio <= 1.0, (name, ratio, sratio)
    for d in defects:
        if _by_integer(c, d):
            continue
        yd, sd = gr.emulate(p, d, geo, parts)
        rd = max(_ratio(yd, r.out, bnd), _stats_ratio(sd, yd) if sd is not None else 0.0)
        print(f"{name} random, {d}: {rd:.1f} bounds")
        assert rd > MARGIN, (name, d, rd)
    del r, bnd, parts
    if "integer" not in gc.families(c):
        return
    # ---- integer family: bit-exact, reaches beyond 2048; the defects of this family change bits
    p = gc.build(name, "integer")
    r = gr.reference(p, with_err=False)
    want = gr.exact_output(p, r)
    parts = gr.emu_partials(p)
    y, st = gr.emulate(p, parts=parts)
    assert np.abs(r.out).max() < 65504 and np.abs(r.v1).max() < 65504, name
    assert _same(y, want), f"{name}: the emulation is not bit-exact on the integer family"
    if st is not None:
        assert np.abs(want.astype(np.float64)).max() <= 256, name
        assert np.array_equal(st.astype(np.float64), gr.stats_ref(want)[0]), f"{name}: integer statistics are not exact"
    elif gc.has(c, "r") or gc.has(c, "w"):
        big = float((np.abs(r.v1) > 2048).mean())
        print(f"{name} integer: {100 * big:.2f} % of the outputs beyond 2048")
        assert big >= 0.005, (name, big)
    for d in defects:
        if not _by_integer(c, d):
            continue
        yd, sd = gr.emulate(p, d, geo, parts)
        n = int((yd.view(np.int16) != want.view(np.int16)).sum())
        print(f"{name} integer, {d}: {n} outputs differ")
        assert n > 0, (name, d)
    # ---- one-hot family: the emulation returns W[n][k(m)]
    p = gc.build(name, "onehot")
    y, st = gr.emulate(p)
    assert _same(y, gc.onehot_output(p)), f"{name}: the emulation is not bit-exact on the one-hot family"
    if st is not None:
        assert _stats_ratio(st, y) <= 1.0, name
