"""CPU: the inputs of tests/test_gpu_attention.py are what that file needs them to be.  Every case of oracle/attention_cases.py goes through
univst_debug_attention_plan (host only) and gives the kernel it is named for, and the cases together give exactly the launch table — a kernel
added to ATTN_KERNELS without a case fails here.  A float32 / fp16 emulation of the kernels' tile-wise online softmax (oracle/attention_ref.py:
64-key tiles, deferred reference, round-toward-zero packing, the two-launch merge) meets every bound of the GPU file on every case, the uniform
and one-hot families are exact as claimed, and each planted defect — the last key of a source dropped, one key tile's rescale skipped,
src_logw ignored, src_cnt ignored, two heads swapped, the source table read from the other frame's row, a phase-1 state with l off by one key —
moves the result by more than 8 bounds on every case it applies to (the ratios are printed: pytest -s)."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import attention_cases as ac
from oracle import attention_ref as ar

FACTOR = 8.0
RMS_MAX, ABS_MAX = 6e-4, 2.5e-3          # the whole-tensor figures of test_gpu_ops.py::test_attention_two_phase_error_is_rounding_level


@pytest.fixture(scope="module")
def lib():
    from univst_amd import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native.load()


def _plan(lib, args):
    buf = C.create_string_buffer(4096)
    rc = lib.univst_debug_attention_plan(*args, buf, 4096)
    return rc, buf.value.decode()


def _cnt_key(c):
    return "full" if c.phase else None


def _ratio(got, want, bnd):
    return float((np.abs(got.astype(np.float64) - want) / bnd).max())


# ------------------------------------------------------------------------------------------------ the plan
@pytest.mark.parametrize("name", list(ac.CASES))
def test_case_selects_the_kernel_it_is_named_for(lib, name):
    c = ac.CASES[name]
    rc, line = _plan(lib, ac.plan_args(c))
    assert rc == 0 and line.split(" ")[0] == c.sym, (name, rc, line)
    assert (c.BF, c.heads) == (2, 2) and ar.traits(c.sym).body in ("attn_body", "pp40", "pp64", "text")


def test_cases_cover_the_launch_table(lib):
    """set equality between the cases' symbols and ATTN_KERNELS, read from the entry's all-zero call"""
    table = set(_plan(lib, (0,) * 9)[1].split(";"))
    named = {c.sym for c in ac.CASES.values()}
    assert len(table) == 61
    assert named == table, f"no case for: {sorted(table - named)}; in no launch table: {sorted(named - table)}"
    # the second launch of the chained tests is the case's own kernel, the first whatever the plan gives that shape (one of the table's)
    for n in ac.of_phase(2):
        rc, line = _plan(lib, ac.plan_args(ac.CASES[n], phase=1))
        assert rc == 0 and line.split(" ")[0] in table, (n, line)


def test_shapes_leave_the_tails_the_cases_are_there_for():
    for c in ac.CASES.values():
        tr = ar.traits(c.sym)
        if tr.body == "attn_body":
            qb = int(c.sym.split("<")[1].split(",")[2].rstrip(">"))
            assert c.Nq > 64 * qb and c.Nq % (64 * qb) not in (0,) and c.Nq % 16 != 0, c.name
        if c.nsrc >= 2:
            assert c.Nkv == 141 and c.Nkv % ar.KT == 13
            assert all(row != sorted(row) or row[0] != 0 for row in ac.SRC_IDX[c.nsrc])          # not the identity
    text = {(c.d, c.Nkv) for c in ac.CASES.values() if c.sym.startswith("attn_text_kernel")}
    assert text == {(40, 13), (40, 80), (80, 13), (80, 80)}
    reg = {(c.Nkv, c.logw) for c in ac.CASES.values() if c.sym == "attn_pp40_kernel<1,0,false,0>"}
    assert reg >= {(81, False), (100, False), (128, False), (77, True)}
    assert {c.Nq for c in ac.CASES.values() if c.sym == "attn_pp64_kernel<0,2>"} == {200, 1064}
    for body in ("attn_body", "pp40", "pp64"):
        mine = [c for c in ac.CASES.values() if ar.traits(c.sym).body == body]
        assert any(c.nsrc == 3 and c.cnt == (1, 3) and c.logw for c in mine), body
        assert any(c.Nkv == 1 and c.nsrc == 1 for c in mine), body


# ------------------------------------------------------------------------------------------------ the emulation meets the bounds
@pytest.mark.parametrize("name", ac.of_phase(0) + ac.of_phase(1))
def test_emulation_meets_the_bound_one_launch(name):
    """random family: rows (and, first phase, the state) of the emulation within the bound; the whole-tensor backstop too"""
    c = ac.CASES[name]
    tr = ar.traits(c.sym)
    p = ac.build(name, "random", _cnt_key(c))
    r = ar.reference(p)
    got = ar.emulate(p, tr, phase=c.phase)
    if c.phase == 1:
        got, st = got
        with np.errstate(divide="ignore"):
            lse = st[..., 0].astype(np.float64) + np.log2(st[..., 1].astype(np.float64))
        sr = float((np.abs(lse - r.lse) / ar.state_bound(p, r, tr)).max())
        print(f"{name}: state max(err / bound) = {sr:.3f}")
        assert sr <= 1.0, (name, sr)
    ratio = _ratio(got, r.out, ar.bound(p, r, tr))
    e = got.astype(np.float64) - r.out
    rms, mx = float(np.sqrt((e ** 2).mean() / (r.out ** 2).mean())), float(np.abs(e).max() / np.abs(r.out).max())
    print(f"{name} [{c.sym}]: emulation max(err / bound) = {ratio:.3f}, rms {rms:.2e}, max {mx:.2e}")
    assert ratio <= 1.0 and rms < RMS_MAX and mx < ABS_MAX, (name, ratio, rms, mx)


@pytest.mark.parametrize("name", ac.of_phase(2))
def test_emulation_meets_the_bound_merge(name):
    """the merge launch on a synthetic float64 first phase (true maximum, and shifted by a non-integer either way), and chained behind the
    emulated first phase"""
    c = ac.CASES[name]
    tr = ar.traits(c.sym)
    p1 = ac.build(name, "random", "full")
    p2 = ac.merge_problem(p1, "full")
    r1, r2 = ar.reference(p1), ar.reference(p2)
    want, bnd = ar.merge_bound(p1, r1, r2, tr)
    for shift in (0.0, 2.6, -3.3):
        got = ar.emulate(p2, tr, phase=2, state_in=ar.synthetic_state(r1, shift), out_in=r1.out.astype(np.float16))
        ratio = _ratio(got, want, bnd)
        print(f"{name}: synthetic first phase, m + {shift}: max(err / bound) = {ratio:.3f}")
        assert ratio <= 1.0, (name, shift, ratio)
    o1, st = ar.emulate(p1, ar.traits(ac.chain_first_symbol(c)), phase=1)
    got = ar.emulate(p2, tr, phase=2, state_in=st, out_in=o1)
    union = ar.reference(p1, frames=[p1.sources(bf) + p2.sources(bf) for bf in range(c.BF)])
    cb = ar.chained_bound(p1, r1, r2, union, ar.traits(ac.chain_first_symbol(c)), tr)
    ratio = _ratio(got, union.out, cb)
    print(f"{name}: chained: max(err / bound) = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)


def test_chain_first_symbol_is_the_plan(lib):
    for n in ac.of_phase(2):
        c = ac.CASES[n]
        rc, line = _plan(lib, ac.plan_args(c, phase=1))
        assert rc == 0 and line.split(" ")[0] == ac.chain_first_symbol(c), (n, line)


# ------------------------------------------------------------------------------------------------ the exact families
@pytest.mark.parametrize("name", list(ac.CASES))
def test_uniform_and_onehot_references_are_exact(name):
    c = ac.CASES[name]
    tr = ar.traits(c.sym)
    pu = ac.build(name, "uniform", _cnt_key(c))
    assert not pu.q16().any()
    v = pu.v16().astype(np.float64)
    assert (v == np.round(v)).all() and np.abs(v).max() <= 20
    ru = ar.reference(pu)
    assert (ru.mx == 0.0).all() if pu.src_logw is None else True           # every score is 0: every probability 1
    ratio = _ratio(ar.emulate(pu, tr), ru.out, ac.uniform_bound(pu, ru))
    print(f"{name}: uniform: max(err / bound) = {ratio:.3f}")
    assert ratio <= 1.0, (name, ratio)
    po = ac.build(name, "onehot", _cnt_key(c))
    ro = ar.reference(po, detail=False)
    want = ac.selected_rows(po)
    # float64 puts all but 2^-40 of the weight on the selected key, and the emulation returns its V row bit for bit
    assert np.abs(ro.out - want.astype(np.float64)).max() <= 2 * 2048 * 1024 * 2.0 ** -40 and float(ro.L.max()) - 1.0 <= 1024 * 2.0 ** -40, name
    assert np.array_equal(ar.emulate(po, tr).view(np.int16), want.view(np.int16)), name
    vo = po.v16()
    assert (np.abs(vo.astype(np.float64)) >= 1).all() and (vo.astype(np.float64) == np.round(vo.astype(np.float64))).all()
    sel = po.select[..., 0] * c.Nkv + po.select[..., 1]
    if c.Nkv > 1:                                                            # the selection reaches the tail of the last and of the first source
        assert (po.select[..., 1] == c.Nkv - 1).any() and len(np.unique(sel)) >= min(c.Nq, c.Nkv) // 2, name


# ------------------------------------------------------------------------------------------------ sensitivity
def _applies(defect, c, p):
    if defect == "no_logw":
        return p.src_logw is not None and c.nsrc > 1
    if defect == "no_cnt":
        return p.src_cnt is not None and any(int(n) < c.nsrc for n in p.src_cnt)
    if defect == "skip_rescale":
        return c.nsrc * c.Nkv > ar.KT
    if defect == "drop_last_key":
        return c.Nkv > 1
    if defect == "state_l_off":
        return c.phase == 2
    return True


@pytest.mark.parametrize("name", list(ac.CASES))
def test_planted_defects_move_the_result_by_more_than_8_bounds(name):
    """the emulation with one defect, against the float64 reference and the bound of the right kernel: every defect that applies to the case
    shows in the uniform or in the random family by more than FACTOR bounds somewhere"""
    c = ac.CASES[name]
    tr = ar.traits(c.sym)
    worst = {}
    for family in ("uniform", "random"):
        p = ac.build(name, family, _cnt_key(c))
        todo = [d for d in ar.DEFECTS if _applies(d, c, p) and worst.get(d, 0.0) <= FACTOR]
        if not todo:
            continue
        r = ar.reference(p)
        one = ar.bound(p, r, tr) if family == "random" else ac.uniform_bound(p, r)
        for defect in todo:
            if defect == "state_l_off":
                p2 = ac.merge_problem(p, "full")
                tr1 = ar.traits(ac.chain_first_symbol(c))
                o1, st = ar.emulate(p, tr1, phase=1, defect=defect)
                got = ar.emulate(p2, tr, phase=2, state_in=st, out_in=o1)
                union = ar.reference(p, frames=[p.sources(bf) + p2.sources(bf) for bf in range(c.BF)])
                r2 = ar.reference(p2)
                want, bnd = union.out, ar.chained_bound(p, r, r2, union, tr1, tr)
                if family == "uniform":           # exact sums: what remains is the fp16 rounding of the phase-1 rows and the store
                    bnd = ac.uniform_bound(p, union) + ar._percol(p, ar.merge_weights(p, r, r2)[0]) * ar.store_bound(r.out)
            else:
                want, bnd, got = r.out, one, ar.emulate(p, tr, defect=defect)
            worst[defect] = max(worst.get(defect, 0.0), _ratio(got, want, bnd))
    print(f"{name}: " + ", ".join(f"{d} {w:.3g}" for d, w in worst.items()))
    assert all(w > FACTOR for w in worst.values()), (name, worst)


def test_every_defect_applies_to_some_cases():
    for defect in ar.DEFECTS:
        n = sum(_applies(defect, c, ac.build(name, "random", _cnt_key(c))) for name, c in ac.CASES.items())
        assert n >= 3, (defect, n)
