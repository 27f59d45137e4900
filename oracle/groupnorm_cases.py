"""Designed inputs for tests/test_gpu_groupnorm.py (csrc/norm.hip through the C ABI) and the bound its outputs are held to.

Every case names the route and the launch geometry it is there for (EXPECT); tests/test_groupnorm_cases.py holds the library's plan read-out
(univst_debug_groupnorm_plan) to them without a GPU, so a moved threshold fails there instead of quietly un-covering a route.  The base data are
ordinary (per-channel mean + unit normal, gamma = 1 + 0.1 n, beta = 0.1 n, all rounded to fp16); on top of them SENTINEL rows carry + 32 on every
channel.  They sit where a row-range mistake of the kernels would drop or double-count a row — first / last row of the unit, of chunk 0 and of the
last chunk, the first row of the last (partial) thread-row stride of a ragged chunk, rows 255 / 256 of the one-launch kernel — and one such row
moves the group variance by about 1024 / rows_per_stat, which is far outside the bound below (asserted on the CPU for every sentinel)."""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

from oracle.groupnorm_ref import groupnorm_ref

SMALL, STREAM, PRODUCER = 0, 1, 2
SENTINEL = 32.0
PLAN_FIELDS = ("route", "fold", "sharded", "block", "TR", "nchunk", "rpc", "nblk", "rpb", "lds_stats", "lds_tail",
               "stats_grid_x", "stats_grid_y", "reduce_grid", "tail_grid_x", "tail_grid_y")

Case = namedtuple("Case", "name C1 C2 G rps S eps silu values")


def _c(name, C1, C2, G, rps, S, eps, silu, values="normal"):
    return Case(name, C1, C2, G, rps, S, eps, silu, values)


# route / edge per case: see EXPECT
GEOMETRY_CASES = [
    _c("c01_tr6_ragged_last_chunk", 320, 0, 32, 1000, 1, 1e-5, True),
    _c("c02_tr3", 640, 0, 32, 1000, 1, 1e-5, True),
    _c("c03_tr2_straddle", 640, 320, 32, 2100, 1, 1e-5, True),
    _c("c04_tr1_two_chunks", 1280, 0, 32, 5, 1, 1e-6, False),
    _c("c05_tr1_chunk_cap", 1280, 640, 32, 2100, 1, 1e-5, True),
    _c("c06_block320", 1280, 1280, 32, 777, 1, 1e-5, True),
    _c("c07_tr64_empty_thread_rows", 32, 0, 8, 7, 1, 1e-6, False),
    _c("c08_odd_group_width", 120, 0, 8, 40, 12, 1e-6, False),
    _c("c09_vae128_tr16", 128, 0, 32, 1500, 1, 1e-6, True),
    _c("c10_vae512_tr4", 512, 0, 32, 4099, 1, 1e-6, True),
    _c("c11_stream_by_size_3_units", 320, 0, 32, 2731, 3, 1e-5, True),
    _c("c12_small_fewer_rows_than_threads", 1280, 0, 32, 40, 6, 1e-6, False),
    _c("c13_small_straddle", 640, 320, 32, 160, 2, 1e-5, True),
    _c("c14_small_257_rows", 320, 0, 32, 257, 2, 1e-5, True),
    _c("c15_small_single_row", 320, 0, 32, 1, 2, 1e-6, False),
    _c("c16a_small_exactly_4mib", 512, 0, 32, 2048, 2, 1e-6, False),
    _c("c16b_stream_one_row_over", 512, 0, 32, 2049, 2, 1e-6, False),
]
# value cases on the geometry of case 1 (streaming) and case 14 (one launch); no sentinels: the values are the point
VALUE_CASES = [_c(f"{name}_{tag}", 320, 0, 32, rps, S, eps, silu, values)
               for tag, rps, S in (("stream", 1000, 1), ("small", 257, 2))
               for name, values, eps, silu in (("large_mean", "large_mean", 1e-5, True), ("tiny_var_eps5", "tiny_var", 1e-5, False),
                                               ("tiny_var_eps6", "tiny_var", 1e-6, False), ("const_group", "const_group", 1e-5, True))]
CASES = {c.name: c for c in GEOMETRY_CASES + VALUE_CASES}
CONST_GROUP, CONST_VALUE = 5, 0.5

# what the plan read-out must say (block = (C / 8) x TR; nchunk x rpc: the statistics pass; nblk: the apply pass)
_S = dict(route=SMALL, block=0, TR=0, nchunk=0, rpc=0, nblk=0)
EXPECT = {
    "c01_tr6_ragged_last_chunk": dict(route=STREAM, block=240, TR=6, nchunk=42, rpc=24, nblk=84),           # last chunk: 16 rows = 2 strides + 4
    "c02_tr3": dict(route=STREAM, block=240, TR=3, nchunk=84, rpc=12, nblk=167),
    "c03_tr2_straddle": dict(route=STREAM, block=240, TR=2, nchunk=263, rpc=8, nblk=525),                 # group 21 = channels 630 .. 659
    "c04_tr1_two_chunks": dict(route=STREAM, block=160, TR=1, nchunk=2, rpc=3, nblk=3),                   # 3 + 2 rows
    "c05_tr1_chunk_cap": dict(route=STREAM, block=240, TR=1, nchunk=420, rpc=5, nblk=1050),               # 525 chunks of 4 rows -> capped at 512 -> rpc 5
    "c06_block320": dict(route=STREAM, block=320, TR=1, nchunk=195, rpc=4, nblk=389),                     # C / 8 = 320 > 256
    "c07_tr64_empty_thread_rows": dict(route=STREAM, block=256, TR=64, nchunk=1, rpc=7, nblk=1),          # 57 of 64 thread-rows see no row
    "c08_odd_group_width": dict(route=STREAM, block=255, TR=17, nchunk=1, rpc=40, nblk=2),                # S * G = 96 and 115 KB, but 15 channels per group
    "c09_vae128_tr16": dict(route=STREAM, block=256, TR=16, nchunk=24, rpc=63, nblk=47),
    "c10_vae512_tr4": dict(route=STREAM, block=256, TR=4, nchunk=257, rpc=16, nblk=513),
    "c11_stream_by_size_3_units": dict(route=STREAM, block=240, TR=6, nchunk=114, rpc=24, nblk=228),
    "c12_small_fewer_rows_than_threads": _S, "c13_small_straddle": _S, "c14_small_257_rows": _S, "c15_small_single_row": _S,
    "c16a_small_exactly_4mib": _S,
    "c16b_stream_one_row_over": dict(route=STREAM, block=256, TR=4, nchunk=129, rpc=16, nblk=257),
}
for _v in VALUE_CASES:
    EXPECT[_v.name] = EXPECT["c01_tr6_ragged_last_chunk"] if _v.rps == 1000 else _S


def plan(case, fold_n=0, world=1, producer_stats=False):
    """the library's own account of what it launches for the case (host code, no GPU)"""
    import ctypes
    from univst_amd import _native
    out = (ctypes.c_int * len(PLAN_FIELDS))()
    _native.check(_native.load().univst_debug_groupnorm_plan(case.C1, case.C2, case.rps * case.S, case.rps, case.G, fold_n, world, int(producer_stats), out),
                  "debug_groupnorm_plan")
    return dict(zip(PLAN_FIELDS, out))


def sentinel_rows(pl, rps):
    """rows of one stat unit, from the plan"""
    rows = {0, rps - 1}
    if pl["route"] == SMALL:
        rows |= {r for r in (255, 256) if r < rps}                     # thread 255's first row, thread 0's second row
    else:
        TR, rpc = pl["TR"], pl["rpc"]
        for ch in (0, pl["nchunk"] - 1):
            r0, r1 = ch * rpc, min((ch + 1) * rpc, rps)
            rows |= {r0, r1 - 1}
            if (r1 - r0) % TR:                                          # ragged: the last stride covers fewer than TR rows
                rows.add(r0 + (r1 - r0 - 1) // TR * TR)
    return sorted(rows)


def sentinel_units(S):
    return list(range(S)) if S <= 3 else [0, S - 1]


@lru_cache(maxsize=2)
def build(name):
    """-> x1, x2 (fp16 [rows, C1], [rows, C2] or None), gamma, beta (fp16 [C]), sentinels [(unit, row)], plan, ref (GnRef, float64)"""
    c = CASES[name]
    g = torch.Generator().manual_seed(1000 + sorted(CASES).index(name.replace("eps6", "eps5")))       # the two eps cases share their data
    C, rows, cpg = c.C1 + c.C2, c.rps * c.S, (c.C1 + c.C2) // c.G
    if c.values == "large_mean":                                        # |mean| = 800 sigma: the one-pass fp32 variance cancels without the pivot
        x = 200.0 + 0.25 * torch.randn(rows, C, generator=g)
    elif c.values == "tiny_var":                                        # sigma^2 = 1.25 * 2^-20 = 1.2e-6: eps decides the answer
        x = torch.randint(0, 4, (rows, C), generator=g).float() * 2.0 ** -10
    else:
        x = torch.randn(C, generator=g) + torch.randn(rows, C, generator=g)
    if c.values == "const_group":
        x[:, CONST_GROUP * cpg:(CONST_GROUP + 1) * cpg] = CONST_VALUE
    pl = plan(c)
    sent = []
    if c.values == "normal":
        sent = [(u, r) for u in sentinel_units(c.S) for r in sentinel_rows(pl, c.rps)]
        for u, r in sent:
            x[u * c.rps + r] += SENTINEL
    x = x.half()
    gamma = (1.0 + 0.1 * torch.randn(C, generator=g)).half()
    beta = (0.1 * torch.randn(C, generator=g)).half()
    x1 = x[:, :c.C1].contiguous()
    x2 = x[:, c.C1:].contiguous() if c.C2 else None
    ref = groupnorm_ref(x1, gamma, beta, c.G, c.eps, c.rps, c.silu, x2)
    return SimpleNamespace(case=c, x1=x1, x2=x2, gamma=gamma, beta=beta, sentinels=sent, plan=pl, ref=ref)


def bound(b, ref=None):
    """[rows, C] float64: what |kernel - ref| may be, element by element (derivation: tests/test_gpu_groupnorm.py).
        pre   = [(|x| + |mean|) r |gamma| + |beta|] * 8 * 2^-24  +  |z - beta| (rho^2 + 8) 2^-25
        bound = 1.1 pre + 2^-11 |ref| + 2^-25
    r = 1 / sqrt(sigma^2 + eps), rho = |mean| / sigma of the element's group (a constant group has z = beta: its rstd term is 0)."""
    c = b.case
    ref = b.ref if ref is None else ref
    C = c.C1 + c.C2
    cpg = C // c.G
    x = b.x1.double() if b.x2 is None else torch.cat([b.x1.double(), b.x2.double()], dim=1)
    per_elem = lambda t: t.repeat_interleave(cpg, dim=1).repeat_interleave(c.rps, dim=0)       # [S, G] -> [rows, C]
    mean, sigma = per_elem(ref.mean), per_elem(ref.sigma)
    r = 1.0 / torch.sqrt(sigma ** 2 + c.eps)
    gam, bet = b.gamma.double().abs(), b.beta.double()
    zb = (ref.z - bet).abs()
    rstd_term = torch.where(sigma > 0, zb * ((mean / sigma) ** 2 + 8.0), torch.zeros_like(zb)) * 2.0 ** -25
    pre = ((x.abs() + mean.abs()) * r * gam + bet.abs()) * 8 * 2.0 ** -24 + rstd_term
    return 1.1 * pre + 2.0 ** -11 * ref.out.abs() + 2.0 ** -25


def unit_slice(b, u):
    c = b.case
    return slice(u * c.rps, (u + 1) * c.rps)


def reweighted_unit(b, u, row, weight):
    """float64 output of unit u when `row` enters its statistics with `weight` (0: dropped, 2: counted twice)"""
    c = b.case
    sl = unit_slice(b, u)
    w = torch.ones(c.rps, dtype=torch.float64)
    w[row] = weight
    return groupnorm_ref(b.x1[sl], b.gamma, b.beta, c.G, c.eps, c.rps, c.silu, None if b.x2 is None else b.x2[sl], row_weight=w).out


# --------------------------------------------------------------------------- fold tail
FOLD_N = 37            # not a multiple of the 4 output rows a block of gn_fold_linear_kernel takes


def fold_weights(C):
    """w [37, C] with |w| in [0.02, 0.1] (no product w * gamma * rstd falls into the fp16 subnormals), bias [37]"""
    g = torch.Generator().manual_seed(77)
    w = (0.02 + 0.08 * torch.rand(FOLD_N, C, generator=g)) * (torch.randint(0, 2, (FOLD_N, C), generator=g) * 2 - 1)
    return w.half(), (0.1 * torch.randn(FOLD_N, generator=g)).half()
