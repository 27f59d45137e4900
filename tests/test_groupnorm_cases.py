"""CPU: the inputs of tests/test_gpu_groupnorm.py are what that file needs them to be.  The launch plan of every case is read out of the
library (univst_debug_groupnorm_plan: host code, no GPU) and held to the route and geometry the case is named for, so a moved threshold
fails here instead of quietly taking a route out of the GPU test; and every sentinel row of oracle/groupnorm_cases.py is shown, on the
float64 reference alone, to move the output by at least 8 bounds on at least 1 % of its unit when it is dropped from the statistics or
counted twice."""
import pytest
import torch

from oracle import groupnorm_cases as gc
from oracle.groupnorm_ref import groupnorm_ref

FACTOR, SHARE = 8.0, 0.01


@pytest.mark.parametrize("name", list(gc.CASES))
def test_plan_readout_gives_the_route_and_geometry_the_case_is_for(name):
    c = gc.CASES[name]
    pl = gc.plan(c)
    want = gc.EXPECT[name]
    assert {k: pl[k] for k in want} == want, (name, pl)
    assert pl["fold"] == 0 and pl["sharded"] == 0
    C = c.C1 + c.C2
    if pl["route"] == gc.SMALL:
        assert (pl["stats_grid_x"], pl["stats_grid_y"]) == (c.G, c.S) and pl["reduce_grid"] == pl["tail_grid_x"] == pl["lds_stats"] == 0
        assert c.rps * c.S * C * 2 <= 4 << 20 and c.S * c.G >= 48 and (C // c.G) % 2 == 0
    else:
        assert pl["block"] == C // 8 * pl["TR"] and pl["lds_stats"] == 3 * pl["TR"] * C * 4 <= 64 * 1024
        assert (pl["stats_grid_x"], pl["stats_grid_y"]) == (pl["nchunk"], c.S) and (pl["tail_grid_x"], pl["tail_grid_y"]) == (pl["nblk"], c.S)
        assert (pl["nchunk"] - 1) * pl["rpc"] < c.rps <= pl["nchunk"] * pl["rpc"] and pl["nchunk"] <= 512          # the workspace holds 512 chunks per unit
        assert (pl["nblk"] - 1) * pl["rpb"] < c.rps <= pl["nblk"] * pl["rpb"]
        assert c.rps * c.S * C * 2 < 10e6


def test_the_edges_the_cases_are_named_for():
    P = {n: gc.plan(gc.CASES[n]) for n in gc.CASES}
    last = lambda n: gc.CASES[n].rps - (P[n]["nchunk"] - 1) * P[n]["rpc"]                    # rows of the last chunk
    assert last("c01_tr6_ragged_last_chunk") == 16 and 16 % 6 == 4
    assert P["c04_tr1_two_chunks"]["rpc"] == 3 and last("c04_tr1_two_chunks") == 2
    # case 5 really is capped: its uncapped plan has 4 rows per chunk (TR = 1, 4 rows per thread-row) = 525 chunks > 512
    assert -(-2100 // (1 * 4)) == 525 > 512 and P["c05_tr1_chunk_cap"]["nchunk"] == 420 and P["c05_tr1_chunk_cap"]["rpc"] == 5
    assert P["c06_block320"]["block"] == 320 > 256
    assert gc.CASES["c07_tr64_empty_thread_rows"].rps == 7 and P["c07_tr64_empty_thread_rows"]["TR"] - 7 == 57
    c8 = gc.CASES["c08_odd_group_width"]                                                      # small in every respect but the group width
    assert c8.C1 // c8.G == 15 and c8.S * c8.G >= 48 and c8.rps * c8.S * c8.C1 * 2 < 4 << 20 and P[c8.name]["route"] == gc.STREAM
    assert gc.plan(c8._replace(C1=128))["route"] == gc.SMALL                                  # an even width of about the same size: one launch
    c11 = gc.CASES["c11_stream_by_size_3_units"]                                              # small in every respect but the size
    assert c11.S * c11.G >= 48 and c11.rps * c11.S * c11.C1 * 2 > 4 << 20 and P[c11.name]["route"] == gc.STREAM
    a, b = gc.CASES["c16a_small_exactly_4mib"], gc.CASES["c16b_stream_one_row_over"]
    assert a.rps * a.S * a.C1 * 2 == 4 << 20 and b.rps == a.rps + 1 and P[a.name]["route"] == gc.SMALL and P[b.name]["route"] == gc.STREAM
    c3, c13 = gc.CASES["c03_tr2_straddle"], gc.CASES["c13_small_straddle"]
    for c in (c3, c13):
        assert c.C1 % ((c.C1 + c.C2) // c.G) != 0                                             # a group straddles the two sources
    # the routes this file cannot reach from the C ABI are still in the read-out
    assert gc.plan(gc.CASES["c01_tr6_ragged_last_chunk"], world=8)["sharded"] == 1
    assert gc.plan(gc.CASES["c14_small_257_rows"], world=8)["tail_grid_x"] > 0
    assert gc.plan(gc.CASES["c01_tr6_ragged_last_chunk"]._replace(rps=1008), producer_stats=True)["route"] == gc.PRODUCER
    pf = gc.plan(gc.CASES["c01_tr6_ragged_last_chunk"], fold_n=gc.FOLD_N)
    assert pf["fold"] == 1 and pf["route"] == gc.STREAM and pf["nchunk"] == 42 and (pf["tail_grid_x"], pf["tail_grid_y"]) == (10, 1)


def test_plan_readout_reports_the_launchers_errors():
    from univst_amd import _native
    for bad, msg in ((dict(G=7), "not divisible"), (dict(C1=36), "multiples of 8"), (dict(rps=0), "must be positive")):
        with pytest.raises(RuntimeError, match=msg):
            gc.plan(gc.CASES["c01_tr6_ragged_last_chunk"]._replace(**bad))
    assert _native.load().univst_debug_groupnorm_plan(320, 0, 1000, 1000, 32, 0, 1, 0, None) != 0


@pytest.mark.parametrize("name", [c.name for c in gc.GEOMETRY_CASES])
def test_every_sentinel_row_is_visible_in_the_output(name):
    """dropping a sentinel row from the statistics (weight 0), or counting it twice (weight 2), moves at least 1 % of its unit by 8 bounds"""
    b = gc.build(name)
    c = b.case
    if c.rps == 1:                  # a one-row unit has no row count to get wrong: every positive weight gives the same statistics
        assert b.sentinels == [(0, 0), (1, 0)]
        return
    assert len(b.sentinels) >= 2 * len(gc.sentinel_units(c.S))
    bnd = gc.bound(b)
    worst = 1.0
    for u, row in b.sentinels:
        sl = gc.unit_slice(b, u)
        for w in (0.0, 2.0):
            moved = (gc.reweighted_unit(b, u, row, w) - b.ref.out[sl]).abs() >= FACTOR * bnd[sl]
            share = moved.double().mean().item()
            worst = min(worst, share)
            assert share >= SHARE, (name, u, row, w, share)
    print(f"{name}: {len(b.sentinels)} sentinel rows, smallest share of elements moved by >= {FACTOR:g} bounds: {worst:.3f}")


@pytest.mark.parametrize("tag", ["stream", "small"])
def test_eps_case_separates_the_two_eps(tag):
    b5, b6 = gc.build(f"tiny_var_eps5_{tag}"), gc.build(f"tiny_var_eps6_{tag}")
    assert torch.equal(b5.x1, b6.x1) and torch.equal(b5.gamma, b6.gamma) and (b5.case.eps, b6.case.eps) == (1e-5, 1e-6)
    assert set((b5.x1.double() * 1024).unique().tolist()) == {0.0, 1.0, 2.0, 3.0}
    assert (b5.ref.sigma ** 2).max() < 2e-6 and (b5.ref.sigma ** 2).min() > 1e-6
    far = (b5.ref.out - b6.ref.out).abs() >= FACTOR * torch.maximum(gc.bound(b5), gc.bound(b6))
    cpg = 320 // 32
    per_group = far.reshape(-1, b5.case.rps, 32, cpg).double().mean(dim=(1, 3))
    assert per_group.min().item() >= 0.5, per_group.min().item()


@pytest.mark.parametrize("tag", ["stream", "small"])
def test_value_cases_are_what_they_are_named(tag):
    lm = gc.build(f"large_mean_{tag}")
    rho = (lm.ref.mean.abs() / lm.ref.sigma)
    assert rho.min() > 500 and (lm.ref.mean - 200).abs().max() < 0.1
    cg = gc.build(f"const_group_{tag}")
    assert (cg.ref.sigma[:, gc.CONST_GROUP] == 0).all() and (cg.ref.sigma > 0).sum() == cg.ref.sigma.numel() - cg.case.S
    cols = slice(gc.CONST_GROUP * 10, gc.CONST_GROUP * 10 + 10)
    assert torch.equal(cg.ref.z[:, cols], cg.beta.double()[cols].expand(cg.ref.z.shape[0], 10))


@pytest.mark.parametrize("name", ["c03_tr2_straddle", "c08_odd_group_width", "c14_small_257_rows"])
def test_reference_is_torch_group_norm_in_float64(name):
    b = gc.build(name)
    c = b.case
    x = b.x1.double() if b.x2 is None else torch.cat([b.x1.double(), b.x2.double()], dim=1)
    C = x.shape[1]
    nchw = x.reshape(c.S, c.rps, C).permute(0, 2, 1)                                         # [S, C, rows_per_stat]
    want = torch.nn.functional.group_norm(nchw, c.G, b.gamma.double(), b.beta.double(), c.eps)
    if c.silu:
        want = torch.nn.functional.silu(want)
    want = want.permute(0, 2, 1).reshape(-1, C)
    assert (b.ref.out - want).abs().max().item() <= 1e-12
    w = torch.ones(c.rps * c.S, dtype=torch.float64)                                         # unit weights change nothing
    assert torch.equal(groupnorm_ref(b.x1, b.gamma, b.beta, c.G, c.eps, c.rps, c.silu, b.x2, row_weight=w).out, b.ref.out)
