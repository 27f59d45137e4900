"""The cases of tests/test_gpu_linear.py: for every linear (mode 0) kernel of the GEMM launch table (csrc/gemm.hip: GEMM_KERNELS) the smallest
problem that selects it on 256 compute units and still leaves an M tail (M % 16 == 8, or M = 37 / 300), a K tail (K % 64 == 8 or 32) and, where
the path allows one, a ragged last column tile; then the same kernels under the other plan outputs: split-K on both tiles (also with the MM-DiT
epilogue inside splitk_reduce_kernel), the register epilogue of the 256x320 tile (Y 8 bytes off a 16-byte boundary, ldy = N + 1), the tile
orders tile_gn / tile_gm with a ragged row group, weight sets, N % 8 != 0 and N % 4 != 0.  tests/test_gemm_cases.py holds every case to the
plan fields written here.  A conv case would be one more entry with its geometry in `opt` and a gather in build().

Layout (the GPU test): ldx = K + 8, ldr = N + 16, ldy = N + 8 (N + 1 / N where the case says so), ld_gate = N + 24, ldrb = N + 8; rowbias and gate
rows change every 1000 output rows, which no tile height divides: a tile straddles two of them.

Families (build(name, family)):
  random   x seeded normal, w normal / sqrt(K), column K - 1 of both times 8 (a lost K tail moves most outputs by hundreds of bounds); LayerNorm
           cases: rows with mean 0.7, every third row mean 30;
  integer  x in -3 .. 3, w in -2 .. 2, bias / rowbias / bias32 integers up to 64, R (without one: rowbias) up to 2047, bias2 in -3 .. 3, gate in {-2, -1, 1, 2}: every
           float32 partial sum, in any order, is an exact integer below 2^24, so the output is fp16(v) or fp16(fp16(v) + bias2) BIT FOR BIT; with R
           at least 0.5 % of the outputs lie beyond 2048, where fp16 drops odd integers (the store rounding and its ties).  Statistics producers keep
           |Y| <= 256 (bias, R up to 16), so both fp32 sums are exact too.  Not for GELU, GEGLU, the LayerNorm fold;
  onehot   x[m] has a single 1 at k = (7 m + 3) mod K, W[n][k] is an integer code of (set, n, k) in 1 .. 2047 (1 .. 255 for the statistics producers),
           every other operand is present and neutral (0, gate 1): the output is W[n][k(m)] bit for bit, and a mismatch names the k that was read."""
import functools
from types import SimpleNamespace

import numpy as np

from oracle import gemm_ref as gr

BIAS, RES, ROWBIAS, LN_STATS, STATS_OUT, ACT, GATE = 1, 2, 4, 8, 16, 32, 64
Y_UNALIGNED, LDY_ODD = 2048, 16384
NCU = 256
ROWS_PER_BRANCH = 1000
FAMILIES = ("random", "integer", "onehot")
B3, B4, SM = "gemm_big_kernel<0,3,%d>", "gemm_big_kernel<0,4,%d>", "gemm_kernel<%d,0,%d,%d>"


def _case(name, sym, M, N, K, ops="", splits=1, epi=None, tgn=0, tgm=0, **opt):
    """ops: letters of the operands / epilogue — b bias, r residual, w rowbias, 2 bias2, a GELU(tanh), g gate, s stats_out, l LayerNorm fold.
    opt: geglu = 1 / 2, sets = rows per weight set, yoff (Y 8 bytes off), ldy = "odd" (N + 1) / "n" (N)."""
    big = sym.startswith("gemm_big")
    if epi is None:
        epi = (0 if opt.get("yoff") or opt.get("ldy") == "odd" else (3 if opt.get("geglu") else 1)) if big else 0
    return SimpleNamespace(name=name, sym=sym, M=M, N=N, K=K, ops=ops, splits=splits, epi=epi, tgn=tgn, tgm=tgm, geglu=opt.get("geglu", 0),
                           sets=opt.get("sets", 0), yoff=bool(opt.get("yoff")), ldy_mode=opt.get("ldy", "pad"))


def _make():
    cs = [
        # ---- the direct 256x320 tile: 192 rows (151 / 228 tiles) and 256 rows (194 tiles)
        _case("big3_plain", B3 % 0, 28808, 320, 72, "brw2"),
        _case("big3_ragged_n", B3 % 0, 14408, 648, 72, "br"),
        _case("big3_geglu", B3 % 0, 28808, 320, 72, "b", geglu=1),
        _case("big4_rowbias_only", B4 % 0, 24584, 640, 72, "bw2"),
        _case("big4_plain", B4 % 0, 24584, 640, 72, "br"),
        _case("big4_ragged_n", B4 % 0, 12296, 1288, 72, "brw"),
        _case("big3_stats", B3 % 1, 28808, 320, 160, "bs"),
        _case("big3_stats_res", B3 % 1, 28808, 320, 160, "brs"),
        _case("big4_stats", B4 % 1, 24584, 640, 160, "bs"),
        _case("big4_stats_res", B4 % 1, 24584, 640, 160, "brs"),
        _case("big3_ln", B3 % 2, 28808, 320, 160, "lr"),
        _case("big3_ln_geglu", B3 % 2, 38152, 320, 160, "l", geglu=1),      # (the C ABI takes a GEGLU consumer only with 150 tiles of BOTH heights)
        _case("big4_ln", B4 % 2, 24584, 640, 160, "l"),
        _case("big4_ln_geglu", B4 % 2, 24584, 640, 160, "l", geglu=1),
        _case("big3_act", B3 % 3, 28808, 320, 72, "ba"),
        _case("big3_gate", B3 % 3, 28808, 320, 72, "bg"),
        _case("big3_act_gate_res", B3 % 3, 28808, 320, 72, "bagr"),
        _case("big3_act_gate_res_ragged_n", B3 % 3, 14408, 648, 72, "bagr"),
        # ---- the X-resident GEGLU kernel
        _case("xres_n256", "geglu_xres_kernel<0>", 300, 256, 320, "b", geglu=2),
        _case("xres_n256_nobias", "geglu_xres_kernel<0>", 300, 256, 320, "", geglu=2),
        _case("xres_n512", "geglu_xres_kernel<0>", 300, 512, 320, "b", geglu=2),
        _case("xres_ln_n256", "geglu_xres_kernel<2>", 300, 256, 320, "l", geglu=2),
        _case("xres_ln_n512", "geglu_xres_kernel<2>", 300, 512, 320, "l", geglu=2),
        # ---- the 128-wide tile: 128 x 128, 128 x 160, 64 x 128
        _case("s44_one_tile", SM % (4, 4, 0), 37, 128, 72, "brw2"),
        _case("s44_514_tiles", SM % (4, 4, 0), 32776, 256, 72, "br"),
        _case("s44_geglu", SM % (4, 4, 0), 32776, 256, 72, "b", geglu=1),
        _case("s44_act", SM % (4, 4, 0), 37, 128, 72, "ba"),
        _case("s54_plain", SM % (5, 4, 0), 300, 160, 72, "brw2"),
        _case("s54_act_gate_res", SM % (5, 4, 0), 300, 160, 72, "bagr"),
        _case("s42_plain", SM % (4, 2, 0), 300, 96, 72, "br"),
        _case("s42_geglu", SM % (4, 2, 0), 300, 96, 72, "b", geglu=1),
        _case("s42_gate", SM % (4, 2, 0), 300, 96, 72, "bg"),
        _case("s42_n100", SM % (4, 2, 0), 300, 100, 72, "brw2"),
        _case("s42_n98", SM % (4, 2, 0), 300, 98, 72, "br"),
        _case("s42_n98_ldy98", SM % (4, 2, 0), 300, 98, 72, "br", ldy="n"),
        _case("s54_stats", SM % (5, 4, 1), 300, 160, 72, "brs"),
        _case("s54_stats_2slots", SM % (5, 4, 1), 300, 320, 72, "bs"),
        _case("s44_ln", SM % (4, 4, 2), 37, 128, 160, "l"),
        _case("s54_ln", SM % (5, 4, 2), 300, 160, 160, "lr"),
        _case("s42_ln", SM % (4, 2, 2), 300, 128, 160, "l"),
        # ---- split-K: 5 splits of 26 k tiles on the 256x320 tile (the last one short and ending in the K tail), 13 / .. on the 128-wide one
        _case("big4_splitk", B4 % 0, 3080, 640, 8200, "brw2", splits=5),
        _case("big4_splitk_yoff", B4 % 0, 3080, 640, 8200, "br", splits=5, yoff=1),
        _case("big3_splitk_act_gate_res", B3 % 3, 3080, 640, 8200, "bagr", splits=5),
        _case("s42_splitk", SM % (4, 2, 0), 300, 96, 4104, "brw2", splits=13),
        _case("s44_splitk", SM % (4, 4, 0), 37, 128, 4104, "br", splits=13),
        _case("s54_splitk", SM % (5, 4, 0), 300, 160, 4104, "brw2", splits=13),
        _case("s54_splitk_act_gate", SM % (5, 4, 0), 300, 160, 4104, "bag", splits=13),
        _case("s54_splitk_gate_res", SM % (5, 4, 0), 300, 160, 4104, "bgr", splits=13),
        # ---- the register epilogue of the 256x320 tile
        _case("big3_yoff", B3 % 0, 28808, 320, 72, "brw2", yoff=1),
        _case("big3_ldy_odd", B3 % 0, 28808, 320, 72, "brw2", ldy="odd"),
        _case("big4_yoff", B4 % 0, 24584, 640, 72, "brw2", yoff=1),
        _case("big4_ldy_odd", B4 % 0, 24584, 640, 72, "br", ldy="odd"),
        _case("big3_act_gate_res_yoff", B3 % 3, 28808, 320, 72, "bagr", yoff=1),
        # ---- tile order: 34 row tiles of 192 in groups of 8 (the last group has 2); an odd column-tile count; ragged N
        _case("order_gn2", B3 % 0, 6408, 1920, 832, "br", tgn=2, tgm=8),
        _case("order_gn0_odd", B3 % 0, 7688, 1600, 1000, "br", tgn=0, tgm=8),
        _case("order_gn2_ragged_n", B3 % 0, 6408, 1608, 1000, "br", tgn=2, tgm=8),
        # ---- weight sets (an fp32 bias per set): 200 and 4 sets on the 192-row tile, 96 on the 256-row tile (univst_linear_sets wants 150 tiles of BOTH
        # heights: 38400 rows, not the 28800 the plan alone would take)
        _case("sets200_res", B3 % 0, 38400, 320, 72, "r", sets=192),
        _case("sets200_stats", B3 % 1, 38400, 320, 72, "s", sets=192),
        _case("sets4_res", B3 % 0, 38400, 320, 72, "r", sets=9600),
        _case("sets4_stats", B3 % 1, 38400, 320, 72, "rs", sets=9600),
        _case("sets96_res", B4 % 0, 24576, 640, 72, "r", sets=256),
        _case("sets96_stats", B4 % 1, 24576, 640, 72, "s", sets=256),
    ]
    return {c.name: c for c in cs}


CASES = _make()


def has(c, op):
    return op in c.ops


def families(c):
    exact = not (has(c, "a") or has(c, "l") or c.geglu)
    return FAMILIES if exact else ("random",)


def plan_args(c, ncu=NCU):
    """the arguments of univst_debug_gemm_plan"""
    flags = (BIAS * has(c, "b") | RES * has(c, "r") | ROWBIAS * has(c, "w") | LN_STATS * has(c, "l") | STATS_OUT * has(c, "s") | ACT * has(c, "a")
             | GATE * has(c, "g") | Y_UNALIGNED * c.yoff | LDY_ODD * (c.ldy_mode == "odd"))
    return (ncu, 0, c.M, c.N, c.K, c.geglu, flags, c.sets, 0, 0, 0, 0, 0, 1, 1, 0)


def parse_plan(line):
    """the plan text -> SimpleNamespace(sym, splits, reduce, epi, tgn, tgm)"""
    f = dict(t.split("=") for t in line.split(" ") if "=" in t)
    return SimpleNamespace(sym=line.split(" ")[0], splits=int(f["splits"]), reduce="+splitk_reduce" in line, epi=int(f["epi_lds"]),
                           tgn=int(f["tile_gn"]), tgm=int(f["tile_gm"]))


def layout(c):
    No = c.N // 2 if c.geglu else c.N
    return SimpleNamespace(No=No, ldx=c.K + 8, ldr=No + 16, ldy={"pad": No + 8, "odd": No + 1, "n": No}[c.ldy_mode], ld_gate=c.N + 24, ldrb=c.N + 8)


def geometry(c, sym=None):
    """what the planted epilogue defects need to know of the launch"""
    sym = sym or c.sym
    lay = layout(c)
    if sym.startswith("gemm_big"):
        tile_n, tile_m = 320, 192 if sym.split(",")[1] == "3" else 256
    elif sym.startswith("geglu_xres"):
        tile_n, tile_m = 256, 128
    else:
        a = sym[sym.index("<") + 1:-1].split(",")
        tile_n, tile_m = 32 * int(a[0]), 32 * int(a[2])
    return SimpleNamespace(tile_n=tile_n, tile_m=tile_m, tile_gm=c.tgm, ldr=lay.ldr, ldy=lay.ldy)


def _seed(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def _half(a):
    with np.errstate(over="raise"):
        return np.asarray(a).astype(np.float16)


def onehot_k(c):
    return (7 * np.arange(c.M) + 3) % c.K


def ktps(c):
    """k tiles per split, as uv_gemm_plan forms them"""
    nk = (c.K + 63) // 64
    return (nk + c.splits - 1) // c.splits if c.splits > 1 else 0


@functools.lru_cache(maxsize=3)
def build(name, family):
    """-> a gemm_ref problem with .case and .family (splits / ktps: the case's; they shape the emulation and the bound only)"""
    c = CASES[name]
    assert family in families(c), (name, family)
    rng = np.random.default_rng(_seed(name) + 7 * FAMILIES.index(family))
    M, N, K = c.M, c.N, c.K
    nsets = M // c.sets if c.sets else 1
    nb = (M + ROWS_PER_BRANCH - 1) // ROWS_PER_BRANCH
    stats = has(c, "s")
    kw = dict(geglu=c.geglu, act=has(c, "a"), stats_out=stats, splits=c.splits, ktps=ktps(c), rows_per_set=c.sets)
    if family == "random":
        x = rng.standard_normal((M, K))
        w = rng.standard_normal((nsets, N, K)) / np.sqrt(K)
        if has(c, "l"):
            x += np.where(np.arange(M) % 3 == 2, 30.0, 0.7)[:, None]
        x[:, K - 1] *= 8.0
        w[:, :, K - 1] *= 8.0
        small = lambda *s: rng.standard_normal(s)                                   # noqa: E731
        bias, rowbias, R, bias2, bias32 = small(N), small(nb, N), small(M, N), 0.5 * small(N), small(nsets, N)
        gate = 1.0 + 0.5 * small(nb, N)
    elif family == "integer":
        x = rng.integers(-3, 4, (M, K)).astype(np.float64)
        w = rng.integers(-2, 3, (nsets, N, K)).astype(np.float64)
        lim, rlim = (16, 16) if stats else (64, 2047)
        bias, rowbias, bias32 = (rng.integers(-lim, lim + 1, s).astype(np.float64) for s in ((N,), (nb, N), (nsets, N)))
        if has(c, "w") and not has(c, "r"):            # no residual: the row bias carries the large integers
            rowbias = rng.integers(-rlim, rlim + 1, (nb, N)).astype(np.float64)
        R = rng.integers(-rlim, rlim + 1, (M, N)).astype(np.float64)
        bias2 = rng.integers(-3, 4, N).astype(np.float64)
        gate = rng.choice(np.array([-2.0, -1.0, 1.0, 2.0]), (nb, N))
    else:
        x = np.zeros((M, K))
        x[np.arange(M), onehot_k(c)] = 1.0
        s_, n_, k_ = np.meshgrid(np.arange(nsets), np.arange(N), np.arange(K), indexing="ij")
        code = 1 + (n_ * 37 + k_ * 101 + s_ * 11) % (255 if stats else 2047)              # never 0: the kernel could not return a -0
        w = code * np.where((n_ + k_) % 2 == 0, 1.0, -1.0)
        bias, rowbias, R, bias2, bias32 = np.zeros(N), np.zeros((nb, N)), np.zeros((M, N)), np.zeros(N), np.zeros((nsets, N))
        gate = np.ones((nb, N))
    x16, w16 = _half(x), _half(w)
    if has(c, "b"):
        kw["bias"] = _half(bias)
    if c.sets:
        kw["bias32"] = bias32.astype(np.float32)
    if has(c, "w"):
        kw.update(rowbias=_half(rowbias), rows_per_rb=ROWS_PER_BRANCH)
    if has(c, "r"):
        kw["R"] = _half(R)
    if has(c, "2"):
        kw["bias2"] = _half(bias2)
    if has(c, "g"):
        kw.update(gate=_half(gate), rows_per_gate=ROWS_PER_BRANCH)
    if has(c, "l"):
        # the statistics a sound producer leaves (the float64 sums of the fp16 rows, rounded to fp32), W = fp16(gamma W0), wsum, lnb in fp32
        xs = x16.astype(np.float64).reshape(M, K // 160, 160)
        gamma = 1.0 + 0.3 * rng.standard_normal(K)
        w16 = _half(w16.astype(np.float64) * gamma[None, None])
        kw.update(ln_stats=np.stack([xs.sum(2), (xs * xs).sum(2)], axis=-1).astype(np.float32), ln_eps=1e-5,
                  ln_wsum=w16[0].astype(np.float64).sum(1).astype(np.float32), ln_bias=(0.1 * rng.standard_normal(N)).astype(np.float32))
    p = gr.problem(x16, w16, **kw)
    p.case, p.family = c, family
    return p


def onehot_output(p):
    """W[set(m)][n][k(m)], fp16 [M, N]"""
    c = p.case
    return np.ascontiguousarray(p.w[gr.row_set(p), :, onehot_k(c)])
