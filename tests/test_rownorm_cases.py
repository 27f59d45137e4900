"""CPU: the inputs of tests/test_gpu_rownorm.py are what that file needs them to be.  The path every case takes through layernorm_kernel,
adaln_modulate_kernel, the two RMS kernels and the elementwise kernels is restated in oracle/rownorm_cases.py and held here to what the case
is named for (EXPECT), and the cases together to every path the kernels have; a float32 emulation of the kernels in their own order of
operations meets the bounds on every case (the ratios are printed: pytest -s); and each defect the sentinels are there to catch — a chunk
or an element left out of the sums or counted twice, a row given its neighbour's batch row of the modulation, a head given its neighbour's
statistics, the q | k weights or the q scale on the wrong block — moves some element of the float64 reference by more than 8 bounds."""
import pytest
import torch

from oracle import rownorm_cases as rc
from oracle import rownorm_ref as rr
from oracle import sd3_ref

FACTOR = 8.0


def _holds(path, want, name):
    assert {k: path[k] for k in want} == want, (name, path)


# ------------------------------------------------------------------------------------------------ paths
@pytest.mark.parametrize("name", list(rc.LN_CASES))
def test_layernorm_case_takes_the_path_it_is_named_for(name):
    c = rc.LN_CASES[name]
    _holds(rc.layernorm_path(c.rows, c.C), rc.LN_EXPECT[name], name)
    assert c.C % 8 == 0 and 8 <= c.C <= 2048


@pytest.mark.parametrize("name", list(rc.ADA_CASES))
def test_adaln_case_takes_the_path_it_is_named_for(name):
    c = rc.ADA_CASES[name]
    _holds(rc.adaln_path(rc.ADA_B * rc.ADA_N, rc.ADA_N, c.C, c.two), rc.ADA_EXPECT[name], name)
    assert c.C % 8 == 0 and 8 <= c.C <= 4096


@pytest.mark.parametrize("name", list(rc.RMS_CASES) + list(rc.PAIR_CASES))
def test_rms_case_takes_the_path_it_is_named_for(name):
    if name in rc.PAIR_CASES:
        c = rc.PAIR_CASES[name]
        C = c.heads * c.d
        path = rc.rms_path(c.rows, c.heads, c.d, 3 * C + c.pad, 0, C)
    else:
        c = rc.RMS_CASES[name]
        path = rc.rms_path(c.rows, c.heads, c.d, c.heads * c.d + c.pad, ptr_off=c.ptr_off)
    _holds(path, rc.rms_expect(c), name)


def test_the_cases_reach_every_path():
    L = {n: rc.layernorm_path(c.rows, c.C) for n, c in rc.LN_CASES.items()}
    assert {p["inst"] for p in L.values()} == {(1, 4), (2, 2), (4, 1)}
    assert {(p["inst"], p["slots"]) for p in L.values()} == {((1, 4), 1), ((2, 2), 2), ((4, 1), 3), ((4, 1), 4)}
    for inst in ((1, 4), (2, 2)):                                       # a wave with only some of its RPW rows, an empty wave
        assert any(p["inst"] == inst and p["last_partial_rows"] for p in L.values()), inst
        assert any(p["inst"] == inst and p["last_empty_waves"] for p in L.values()), inst
    assert {p["lanes_last"] for p in L.values()} >= {1, 64} and any(p["empty_slots"] for p in L.values())
    # the template boundaries from both sides, and the width cap
    assert {c.C for c in rc.LN_CASES.values()} >= {8, 512, 520, 1024, 1032, 2048}
    A = {n: rc.adaln_path(15, 5, c.C, c.two) for n, c in rc.ADA_CASES.items()}
    assert {p["slots"] for p in A.values()} >= {1, 2, 3, 5, 8} and {p["outputs"] for p in A.values()} == {1, 2}
    assert {p["slots"] for p in A.values() if p["outputs"] == 2} >= {1, 3, 8}
    assert all(p["last_block_rows"] == 3 and p["batch_steps"] == (5, 10) for p in A.values())
    R = {n: rc.build_rms(n).path for n in rc.RMS_CASES}
    assert {p["LPH"] for p in R.values() if p["kernel"] == "vec"} == {4, 8, 16}
    assert max(p["blocks"] for p in R.values() if p["kernel"] == "vec") > 1
    S = [p for p in R.values() if p["kernel"] == "scalar"]
    assert {p["slots"] for p in S} == {1, 2, 3, 4} and {p["lanes_last"] for p in S} >= {2, 8, 32, 40, 64}
    assert max(p["blocks"] for p in S) > 1
    # d = 64 reaches the scalar kernel only through ld or the pointer
    assert R["scalar_d64_ld_plus_2"]["kernel"] == R["scalar_d64_pointer_plus_2"]["kernel"] == "scalar"
    assert rc.rms_path(5, 3, 64, 192)["kernel"] == "vec" and rc.rms_path(5, 3, 64, 192, 4)["kernel"] == "scalar"
    P = {n: rc.build_pair(n).path for n in rc.PAIR_CASES}
    assert {(p["kernel"], p["LPH"], p["launches"]) for p in P.values()} == {("vec", 8, 1), ("vec", 16, 1), ("scalar", 0, 2)}
    for kernel in ("vec", "scalar"):                                    # a last block with idle threads or waves, and a full one (both in the pair cases)
        assert {p["ragged"] for p in list(R.values()) + list(P.values()) if p["kernel"] == kernel} == {True, False}, kernel
    assert rc.sentinel_chunks(1) == [] and rc.sentinel_chunks(40) == [39] and rc.sentinel_chunks(64) == [63] and rc.sentinel_chunks(65) == [63, 64]
    assert rc.sentinel_chunks(129) == [63, 64, 127, 128] and rc.sentinel_chunks(256) == [63, 64, 127, 128, 191, 192, 255]
    assert rc.sentinel_chunks(512)[-3:] == [447, 448, 511] and len(rc.sentinel_chunks(512)) == 15
    assert rc.rms_sentinels(64, True) == [56, 63] and rc.rms_sentinels(2, False) == [1] and rc.rms_sentinels(192, False) == [63, 64, 127, 128, 191]
    for C in rc.GATE_C:
        _holds(rc.build_gate(C).path, rc.GATE_EXPECT[C], C)
    for which in rc.ACT_INPUTS:
        _holds(rc.build_act(which).path, rc.ACT_EXPECT[which], which)
    T = list(rc.TS_CASES.values())
    assert len(T) == 20 and {c.B for c in T} == {1, 5} and {(c.dim, c.shift) for c in T} == {(2, 0.0), (6, 0.0), (256, 0.0), (320, 0.0), (320, 1.0)}
    assert {c.flip for c in T} == {0, 1} and {t for c in T for t in c.t} == set(rc.TS_VALUES)
    assert {t for c in T if c.B == 1 for t in c.t} >= {981.25, 1000.0} and any(rc.build_ts(c.name).path["blocks"] > 1 for c in T)


# ------------------------------------------------------------------------------------------------ the references
def test_references_are_the_textbook_functions_in_float64():
    F = torch.nn.functional
    b = rc.build_ln("n4_c520_first_of_2x2")
    want = F.layer_norm(b.x.double(), (520,), b.gamma.double(), b.beta.double(), rc.LN_EPS)
    assert (b.ref.out - want).abs().max().item() <= 1e-11
    a = rc.build_ada("a2_c128_two_outputs")
    ln = F.layer_norm(a.x.double(), (128,), None, None, rc.ADALN_EPS).reshape(rc.ADA_B, rc.ADA_N, 128)
    for ref, k_scale, k_shift in ((a.ref, 1, 0), (a.ref2, 7, 6)):
        sc, sh = (a.mod.double()[:, k * 128:(k + 1) * 128] for k in (k_scale, k_shift))
        assert (ref.out - (ln * (1 + sc[:, None]) + sh[:, None]).reshape(15, 128)).abs().max().item() <= 1e-11
    r = rc.build_rms("scalar_d40_h3_r5")
    assert (r.ref.out - sd3_ref._rms(r.x.double(), r.w.double(), rc.RMS_EPS)).abs().max().item() <= 1e-11
    x = rc.all_finite_fp16()
    assert (rr.silu_ref(x) - F.silu(x.double())).abs().max().item() <= 1e-9
    assert ((rr.gelu_tanh_ref(x) - F.gelu(x.double(), approximate="tanh")).abs() / (1 + x.double().abs())).max().item() <= 1e-12
    t = rc.build_ts("t_b5_dim320_shift1_flip1")
    want = sd3_ref.timestep_embedding(t.t, 320, True, 1.0)                                          # float32: the layout and the frequencies
    assert (t.ref - want.double()).abs().max().item() <= 2e-4
    p = rc.build_patch(2)
    B, C, H, W = rc.PATCH_SHAPE
    conv = F.unfold(p.lat.double(), 2, stride=2).transpose(1, 2).reshape(-1, C * 4)                # the k order of the flattened conv weight
    assert torch.equal(conv, p.want_rows.double())
    ein = torch.einsum("nhwpqc->nchpwq", p.rows.reshape(B, H // 2, W // 2, 2, 2, C)).reshape(B, C, H, W)
    assert torch.equal(ein, p.want_lat)


def test_value_cases_are_what_they_are_named():
    for name, rho in (("v_mean300_c320", 500), ("v_mean300_c1280", 500), ("v_mean_m2000_c320", 500), ("v_mean_m2000_c1280", 500)):
        b = rc.build_ln(name)
        assert (b.ref.mean.abs() / b.ref.var.sqrt()).min().item() > rho
    b = rc.build_ln(rc.LN_CONST_CASE)
    for r, v in rc.LN_CONST_ROWS:
        assert (b.x[r] == v).all() and b.ref.var[r].item() == 0 and torch.equal(b.ref.out[r], b.beta.double())
    assert (rc.build_ada("av_mean300_c1536").ref.mean.abs().min().item()) > 299


# ------------------------------------------------------------------------------------------------ the emulation meets the bound
def _ratio(emu, ref, bnd):
    return ((emu - ref).abs() / bnd).max().item()


@pytest.mark.parametrize("name", list(rc.LN_CASES))
def test_float32_emulation_of_layernorm_meets_the_bound(name):
    b = rc.build_ln(name)
    r = _ratio(rr.emu_layernorm(b.x, b.gamma, b.beta, rc.LN_EPS), b.ref.out, rc.ln_bound(b))
    store = rc._store(b.ref.out)
    share = ((rc.ln_bound(b) - store) / store).median().item()
    print(f"layernorm {name}: emulation max(err / bound) {r:.3f}; median non-store / store part of the bound {share:.4f}")
    assert r <= 1.0, (name, r)
    if b.case.values == "normal":
        assert share <= 0.25, (name, share)             # one fp16 rounding plus a margin


@pytest.mark.parametrize("name", list(rc.ADA_CASES))
def test_float32_emulation_of_adaln_meets_the_bound(name):
    b = rc.build_ada(name)
    r = _ratio(rr.emu_adaln(b.x, b.scale, b.shift, rc.ADA_N, rc.ADALN_EPS), b.ref.out, rc.ada_bound(b))
    msg = f"adaln_modulate {name}: emulation max(err / bound) {r:.3f}"
    if b.case.two:
        r2 = _ratio(rr.emu_adaln(b.x, b.scale2, b.shift2, rc.ADA_N, rc.ADALN_EPS), b.ref2.out, rc.ada_bound(b, b.ref2))
        msg += f", second output {r2:.3f}"
        r = max(r, r2)
    print(msg)
    assert r <= 1.0, msg


def test_float32_emulation_of_rmsnorm_meets_the_bound():
    worst = {}
    for name in rc.RMS_CASES:
        b = rc.build_rms(name)
        emu = (rr.emu_rms_vec if b.path["kernel"] == "vec" else rr.emu_rms_scalar)(b.x, b.w, rc.RMS_EPS)
        r = _ratio(emu, b.ref.out, rc.rms_bound(b.ref.out, b.path["adds_per_lane"]))
        assert r <= 1.0, (name, r)
        worst[b.path["kernel"]] = max(worst.get(b.path["kernel"], 0.0), r)
    for name in rc.PAIR_CASES:
        b = rc.build_pair(name)
        c, C = b.case, b.C
        emu_fn = rr.emu_rms_vec if b.path["kernel"] == "vec" else rr.emu_rms_scalar
        q, k = (b.qkv[:, i * C:(i + 1) * C].reshape(c.rows, c.heads, c.d) for i in (0, 1))
        emu = torch.cat([emu_fn(q, b.w0, rc.RMS_EPS, b.scale0).reshape(c.rows, C), emu_fn(k, b.w1, rc.RMS_EPS).reshape(c.rows, C)], dim=1)
        r = _ratio(emu, b.ref[:, :2 * C], rc.rms_bound(b.ref[:, :2 * C], b.path["adds_per_lane"]))
        assert r <= 1.0, (name, r)
        worst["pair " + b.path["kernel"]] = max(worst.get("pair " + b.path["kernel"], 0.0), r)
    print("rmsnorm_heads: emulation worst max(err / bound): " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(worst.items())))


def test_float32_emulation_of_the_elementwise_operators_meets_the_bound():
    for C in rc.GATE_C:
        b = rc.build_gate(C)
        r = _ratio(rr.emu_gate_residual(b.x, b.gate, b.y, rc.ADA_N), b.ref, rc.gate_bound(b.ref))
        print(f"gate_residual C={C}: emulation max(err / bound) {r:.3f}")
        assert r <= 1.0, (C, r)
    for which in rc.ACT_INPUTS:
        b = rc.build_act(which)
        for act, emu, what in ((rc.ACT_SILU, rr.emu_silu, "silu"), (rc.ACT_GELU_TANH, rr.emu_gelu_tanh, "gelu_tanh")):
            ratio = (emu(b.x) - b.ref[act]).abs() / rc.act_bound(b.x, b.ref[act], act)
            i = int(ratio.argmax())
            print(f"{what} {which}: emulation max(err / bound) {ratio.max().item():.4f} at x = {b.x[i].item()}")
            assert ratio.max().item() <= 1.0, (what, which)
    worst = 0.0
    for name in rc.TS_CASES:
        b = rc.build_ts(name)
        c = b.case
        r = _ratio(rr.emu_timestep_embedding(b.t, c.dim, c.flip, c.shift), b.ref, rc.ts_bound(b))
        assert r <= 1.0, (name, r)
        worst = max(worst, r)
    print(f"timestep_embedding: emulation worst max(err / bound) {worst:.3f}")


def test_a_bare_store_bound_does_not_hold_for_gelu_and_the_embedding():
    """why the bounds carry arithmetic terms: the float32 result is several store roundings from float64 where 1 + tanh cancels and where the
    rounded argument sits next to a zero crossing"""
    b = rc.build_act("all_finite")
    r = ((rr.emu_gelu_tanh(b.x) - b.ref[rc.ACT_GELU_TANH]).abs() / rc._store(b.ref[rc.ACT_GELU_TANH])).max().item()
    t = rc.build_ts("t_b1_dim320_shift1_flip0")
    assert t.case.t == (981.25,)
    s = ((rr.emu_timestep_embedding(t.t, 320, 0, 1.0) - t.ref).abs() / rc._store(t.ref)).max().item()
    print(f"store roundings off float64: gelu_tanh {r:.1f}, timestep embedding at t = 981.25 {s:.1f}")
    assert r > 1.5 and s > 1.5


# ------------------------------------------------------------------------------------------------ the defects the sentinels are there to catch
def _chunk_defects(C, chunks):
    """(what, weight [C]): a sentinel chunk, or its element 0 / 7 alone, left out of the sums (0) or counted twice (2)"""
    for ch in chunks:
        for wgt in (0.0, 2.0):
            for what, cols in (("chunk", range(8 * ch, 8 * ch + 8)), ("element 0", [8 * ch]), ("element 7", [8 * ch + 7])):
                w = torch.ones(C, dtype=torch.float64)
                w[list(cols)] = wgt
                yield f"{what} of chunk {ch} x {wgt:g}", w


def _every_row_moved(mut, ref, bnd):
    """smallest over the rows of the largest move within the row, in bounds"""
    return ((mut - ref).abs() / bnd).max(dim=1).values.min().item()


@pytest.mark.parametrize("name", [c.name for c in rc.LN_GEOMETRY if c.C > 8])
def test_every_layernorm_sentinel_is_visible_in_every_row(name):
    b = rc.build_ln(name)
    bnd = rc.ln_bound(b)
    keep = torch.ones(b.case.rows, dtype=torch.bool)
    if name == rc.LN_CONST_CASE:
        keep[[r for r, _ in rc.LN_CONST_ROWS]] = False                  # a constant row has no sentinel: it is there for x - mean = 0
    assert b.sentinels == rc.sentinel_chunks(b.case.C // 8) and b.sentinels
    worst = float("inf")
    for what, w in _chunk_defects(b.case.C, b.sentinels):
        mut = rr.layernorm_ref(b.x, b.gamma, b.beta, rc.LN_EPS, col_weight=w).out
        m = _every_row_moved(mut[keep], b.ref.out[keep], bnd[keep])
        worst = min(worst, m)
        assert m > FACTOR, (name, what, m)
    # the last row (sigma 4x): given the statistics of the row before it
    x2 = b.x.clone()
    x2[-1] = b.x[-2] if b.case.rows > 1 else 0
    if b.case.rows > 1:
        other = rr.layernorm_ref(x2, b.gamma, b.beta, rc.LN_EPS)
        mut = (b.x[-1].double() - other.mean[-1]) * other.r[-1] * b.gamma.double() + b.beta.double()
        m = ((mut - b.ref.out[-1]).abs() / bnd[-1]).max().item()
        assert m > FACTOR, (name, "last row with its neighbour's statistics", m)
    print(f"layernorm {name}: sentinel chunks {b.sentinels}: smallest max move in a row {worst:.1f} bounds")


@pytest.mark.parametrize("name", [n for n, c in rc.ADA_CASES.items() if c.values == "normal"])
def test_every_adaln_sentinel_and_batch_step_is_visible(name):
    b = rc.build_ada(name)
    C = b.case.C
    outs = [(b.ref, b.scale, b.shift)] + ([(b.ref2, b.scale2, b.shift2)] if b.case.two else [])
    worst = float("inf")
    for ref, scale, shift in outs:
        bnd = rc.ada_bound(b, ref)
        for what, w in _chunk_defects(C, b.sentinels):
            m = _every_row_moved(rr.adaln_ref(b.x, scale, shift, rc.ADA_N, rc.ADALN_EPS, col_weight=w).out, ref.out, bnd)
            worst = min(worst, m)
            assert m > FACTOR, (name, what, m)
        for sh, rows in ((1, (4, 9)), (-1, (5, 10))):                  # the rows next to a step of b = r / rows_per_batch take the other side's row
            mut = rr.adaln_ref(b.x, scale, shift, rc.ADA_N, rc.ADALN_EPS, shift_rows=sh).out
            for r in rows:
                m = ((mut[r] - ref.out[r]).abs() / bnd[r]).max().item()
                assert m > FACTOR, (name, "batch row of the neighbour", r, m)
    if b.case.two:                                                      # the second output with the first pair of chunks
        m = ((b.ref.out - b.ref2.out).abs() / rc.ada_bound(b, b.ref2)).max(dim=1).values.min().item()
        assert m > FACTOR, (name, "y2 from scale / shift", m)
    print(f"adaln_modulate {name}: sentinel chunks {b.sentinels}: smallest max move in a row {worst if b.sentinels else float('nan'):.1f} bounds")


def test_every_rms_sentinel_and_head_is_visible():
    worst = float("inf")
    for name in rc.RMS_CASES:
        b = rc.build_rms(name)
        c = b.case
        bnd = rc.rms_bound(b.ref.out, b.path["adds_per_lane"])
        for e in b.sentinels:
            for wgt in (0.0, 2.0):
                w = torch.ones(c.d, dtype=torch.float64)
                w[e] = wgt
                m = ((rr.rms_ref(b.x, b.w, rc.RMS_EPS, elem_weight=w).out - b.ref.out).abs() / bnd).amax(dim=-1).min().item()
                worst = min(worst, m)
                assert m > FACTOR, (name, e, wgt, m)
        if c.heads > 1:                                                 # every head with the statistics of the next one
            mut = b.x.double() * b.ref.r.roll(1, dims=1) * b.w.double()
            m = ((mut - b.ref.out).abs() / bnd).amax(dim=-1).min().item()
            assert m > FACTOR, (name, "neighbouring head's rstd", m)
    print(f"rmsnorm_heads: smallest max move of a (row, head) by a dropped or doubled sentinel element {worst:.1f} bounds")
    for name in rc.PAIR_CASES:
        b = rc.build_pair(name)
        c, C = b.case, b.C
        bnd = rc.rms_bound(b.ref[:, :2 * C], b.path["adds_per_lane"])
        defects = {"weights swapped": rr.rms_pair_ref(b.qkv, c.heads, c.d, 0, b.w1, C, b.w0, rc.RMS_EPS, b.scale0),
                   "scale0 on the k block": rr.rms_pair_ref(b.qkv, c.heads, c.d, C, b.w1, 0, b.w0, rc.RMS_EPS, b.scale0),
                   "scale0 on neither": rr.rms_pair_ref(b.qkv, c.heads, c.d, 0, b.w0, C, b.w1, rc.RMS_EPS, 1.0)}
        defects["scale0 on both"] = defects["scale0 on neither"] * b.scale0
        for what, mut in defects.items():
            m = ((mut[:, :2 * C] - b.ref[:, :2 * C]).abs() / bnd).max(dim=1).values.min().item()
            assert m > FACTOR, (name, what, m)
        assert torch.equal(b.ref[:, 2 * C:], b.qkv[:, 2 * C:].double())


def test_gate_batch_step_is_visible():
    for C in rc.GATE_C:
        b = rc.build_gate(C)
        bnd = rc.gate_bound(b.ref)
        for sh, rows in ((1, (4, 9)), (-1, (5, 10))):
            mut = rr.gate_residual_ref(b.x, b.gate, b.y, rc.ADA_N, shift_rows=sh)
            for r in rows:
                m = ((mut[r] - b.ref[r]).abs() / bnd[r]).max().item()
                assert m > FACTOR, (C, r, m)
