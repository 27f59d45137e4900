"""Float64 reference, per-element bounds and a float32 / fp16 emulation of the linears (mode 0) of csrc/gemm.hip: gemm_big_kernel,
gemm_kernel, geglu_xres_kernel and splitk_reduce_kernel with every epilogue gemm_epilogue_row documents.  Convolutions (mode 1) are not here;
a conv case would add its gather in front of reference() / emu_partials() and reuse everything behind them.

A Problem holds the LOGICAL operands (no pad columns; the GPU test lays them out), all as the kernel gets them: fp16, or fp32 for bias32,
ln_stats, ln_wsum, ln_bias.  The epilogue order (gemm_epilogue_row / gemm_epilogue_lds / splitk_reduce_kernel, all the same):

    v = acc [LayerNorm fold: rstd (acc - mean wsum) + lnb] + bias (or bias32 of the row's weight set) + rowbias[m / rows_per_rb]
    v = GELUtanh(v) if act;  v *= gate[m / rows_per_gate];  v += R;  y = fp16(v);  y = fp16(y + bias2) if bias2
    GEGLU: y = fp16(x gelu_erf(g)), x / g the [16 x | 16 gate] blocks (order 1) or the X-resident interleave (order 2) of v

Bounds (bound()): u16 = 2^-11 (one fp16 rounding), u32 = 2^-24 (one float32 rounding), 2^-25 half an fp16 subnormal step, S the absolute sum
of everything added in float32: sum_k |x_k w_k| + |bias| + |rowbias| (+ |R|).

  accumulate  (K + 8 + splits) u32 S: K products are exact (fp16 x fp16 in fp32), every running sum rounds once, in any order: at most K - 1 + the
              partial sums of the splits + the epilogue's additions, each relative to a partial sum that S bounds;
  store       u16 |v| (1 + 2 u16) + 2^-25 (+ u16 times the error above); bias2: a second u16 |v + bias2| + 2^-25;
  GELU(tanh)  x rcp(1 + exp2(-2 log2e u)): the argument a = 2 log2e u carries 3 roundings (2.1 u32 |a| on the exponential, times 1 - sigma <= 1), rcp
              and exp2 are good to 1 ulp, the sum and the product round once: |gelu| (6 + 2.1 |a|) u32, and the error of its input times |gelu'| <= 1.13;
  gate, R     |gate| times the error so far, + 4 u32 (|gate act| + |R|);
  LN fold     mean = s1 / K, var = s2 / K - mean^2 from `slots` fp32 additions each: d_mean = (slots + 2) u32 sum|s1_slot| / K,
              d_var = (slots + 3) u32 (sum|s2_slot| / K + 2 mean^2) + 2 |mean| d_mean (the cancellation: absolute, so relative to var + eps it grows with
              mean^2 / var), rsqrtf 1 ulp: d_rstd = rstd (d_var / (2 (var + eps)) + 3 u32); then
              rstd (acc error + d_mean |wsum| + 2 u32 (|acc| + |mean wsum|)) + d_rstd |acc - mean wsum| + 2 u32 (|rstd (..)| + |lnb|);
  GEGLU       |gelu_erf(g)| e_x + |x| (1.13 e_g + 1.25 GEGLU_GELU_ERR max(1, |g| / 5)) + 6 u32 |ref|: e_x, e_g the accumulate errors of the two halves.
  statistics  (stats_ref) of the 160 stored values y of a slot: 24 u32 sum|y| and 24 u32 sum y^2 — a value passes through at most 23 float32 additions
              on its way into the slot's sum (gemm_kernel: 20 per lane, two shuffles, the other wave column; gemm_epilogue_lds: 8 + 5 + two shuffles), and
              the squares enter by fmaf: one rounding per addition there too.

GEGLU_GELU_ERR is measured (measure_geglu_erf2(); tests/test_gemm_cases.py re-measures it): the largest |0.5 g (1 + S(g)) - gelu_erf(g)| / max(1, |g| / 5) of
the float32 restatement of common.h geglu_erf2 against float64 erf over every finite fp16 g and 2^22 evenly spaced points of [-8, 8]; the GEGLU term of
the bound is 1.25 GEGLU_GELU_ERR max(1, |g| / 5) |x| (the polynomial is smooth: between grid points 4e-6 apart it cannot move by a quarter of its error)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

U16, U32, SUB = 2.0 ** -11, 2.0 ** -24, 2.0 ** -25
F32, F64 = np.float32, np.float64
BK = 64
# measured: 1.9139e-06 at g = 4.99946 (1.9101e-06 at g = 5 on the fp16 grid).  common.h claims |gelu error| <= 2e-6: it holds for |g| <= 8.  Past the clamp at 5
# the error is |g| / 2 times that of the clamped erf (1 - erf(5 / sqrt 2) = 5.7e-7) plus one float32 rounding of the product, so it grows in proportion to
# |g| (3.9e-3 at g = 32800: 1.2e-7 of the value): the term is GEGLU_GELU_ERR max(1, |g| / 5), which the measurement holds over every finite fp16 g.
GEGLU_GELU_ERR = 1.92e-6
GELU_C = math.sqrt(2.0 / math.pi)
GEGLU_COEF = (2.827276369e-01, -1.405918177e-01, 1.030358595e-01, -8.090256480e-02, 6.295351729e-02, -4.642625655e-02, 3.247217962e-02,
              -2.261424982e-02, 1.353305501e-02, -5.053833458e-03, 2.749192302e-03, -3.353461957e-03, 1.470752778e-03)


def problem(x, w, **kw):
    """x fp16 [M, K]; w fp16 [N, K] or [sets, N, K].  Optional: bias fp16 [N]; bias32 fp32 [sets, N] with rows_per_set; rowbias fp16 [B, N] with
    rows_per_rb; R fp16 [M, N]; bias2 fp16 [N]; act (bool); gate fp16 [G, N] with rows_per_gate; geglu 0 / 1 / 2; ln_stats fp32 [M, K / 160, 2] with
    ln_eps, ln_wsum, ln_bias fp32 [N]; stats_out (bool); splits, ktps (the plan's: how the emulation splits K)."""
    p = SimpleNamespace(x=x, w=w if w.ndim == 3 else w[None], bias=None, bias32=None, rows_per_set=0, rowbias=None, rows_per_rb=1, R=None, bias2=None,
                        act=False, gate=None, rows_per_gate=1, geglu=0, ln_stats=None, ln_eps=1e-5, ln_wsum=None, ln_bias=None, stats_out=False,
                        splits=1, ktps=0)
    p.__dict__.update(kw)
    p.M, p.K = x.shape
    p.N = p.w.shape[1]
    p.No = p.N // 2 if p.geglu else p.N
    return p


def row_set(p):
    return (np.arange(p.M) // p.rows_per_set) if p.rows_per_set else np.zeros(p.M, dtype=np.int64)


def _matmul_sets(p, x, w, sets=None):
    """x [M, k] times w [sets, N, k]^T, every row with the weights of its set"""
    if w.shape[0] == 1:
        return x @ w[0].T
    sets = row_set(p) if sets is None else sets
    out = np.empty((p.M, p.N), dtype=x.dtype)
    for s in np.unique(sets):
        rows = np.nonzero(sets == s)[0]
        out[rows] = x[rows] @ w[s].T
    return out


# ------------------------------------------------------------------------------------------------ GEGLU row orders
def geglu_rows(N, order):
    """-> (xi, gi) [N / 2]: the weight rows that hold x and gate of output column h"""
    h = np.arange(N // 2)
    if order == 1:
        xi = (h // 16) * 32 + h % 16
        return xi, xi + 16
    n = np.arange(N)
    nt, wn, i, g, r = n // 256, (n % 256) // 64, (n % 64) // 16, (n % 16) // 4, n % 4
    col = nt * 128 + wn * 32 + i * 8 + g * 2 + (r & 1)
    xi, gi = np.empty(N // 2, dtype=np.int64), np.empty(N // 2, dtype=np.int64)
    xi[col[r < 2]] = n[r < 2]
    gi[col[r >= 2]] = n[r >= 2]
    return xi, gi


def erf64(z):
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(z, dtype=F64))).numpy()


def gelu_erf64(g):
    return 0.5 * g * (1.0 + erf64(g / math.sqrt(2.0)))


def gelu_tanh64(v):
    return 0.5 * v * (1.0 + np.tanh(GELU_C * (v + 0.044715 * v ** 3)))


def _fma(a, b, c):
    """fmaf on float32 arrays: the float64 product of two float32 values is exact, the sum rounds to float64 and then to float32 (a double
    rounding that differs from the fused result in about 2^-29 of the cases, by one float32 ulp: far inside every bound)"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def emu_geglu_erf2(x, g):
    """common.h geglu_erf2 on float32 arrays, operation by operation"""
    x, g = x.astype(F32), g.astype(F32)
    gc = np.clip(g, F32(-5.0), F32(5.0))
    s = _fma(gc * F32(0.08), gc, np.full_like(gc, -1.0))
    p = np.full_like(gc, GEGLU_COEF[-1])
    for c in GEGLU_COEF[-2::-1]:
        p = _fma(p, s, np.full_like(gc, c))
    S = gc * p
    t = (x * F32(0.5)) * g
    return _fma(t, S, t)


def measure_geglu_erf2():
    """-> (largest |emu(1, g) - gelu_erf(g)| / max(1, |g| / 5), the g where it is, the largest unscaled error over |g| <= 8) over every finite fp16 g and
    2^22 evenly spaced points of [-8, 8]"""
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16).astype(F64)
    worst, at, inside = 0.0, 0.0, 0.0
    for g in (h[np.isfinite(h)], np.linspace(-8.0, 8.0, 1 << 22).astype(F32).astype(F64)):
        err = np.abs(emu_geglu_erf2(np.ones_like(g), g).astype(F64) - gelu_erf64(g))
        inside = max(inside, float(err[np.abs(g) <= 8.0].max()))
        err = err / np.maximum(1.0, np.abs(g) / 5.0)
        i = int(err.argmax())
        if err[i] > worst:
            worst, at = float(err[i]), float(g[i])
    return worst, at, inside


def emu_gelu_tanh(v):
    """common.h gelu_tanh_f on a float32 array: u = 0.79788456f * fmaf(0.044715f * x * x, x, x); x * rcp(1 + exp2(u * -2.88539f))"""
    v = v.astype(F32)
    u = F32(0.7978845608028654) * _fma((F32(0.044715) * v) * v, v, v)
    with np.errstate(over="ignore"):
        e = np.exp2((u * F32(-2.8853900817779268)).astype(F64)).astype(F32)
        return v * (F32(1.0) / (F32(1.0) + e)).astype(F32)


# ------------------------------------------------------------------------------------------------ float64 reference
def ln_rows64(p):
    """(mean, rstd, d_mean, d_rstd) float64 [M] from the fp32 slot statistics as epi_const_stage forms them"""
    st = p.ln_stats.astype(F64)
    slots = st.shape[1]
    s1, s2 = st[..., 0].sum(1), st[..., 1].sum(1)
    mean = s1 / p.K
    var = np.maximum(s2 / p.K - mean * mean, 0.0)
    rstd = 1.0 / np.sqrt(var + p.ln_eps)
    d_mean = (slots + 2) * U32 * np.abs(st[..., 0]).sum(1) / p.K
    d_var = (slots + 3) * U32 * (np.abs(st[..., 1]).sum(1) / p.K + 2 * mean * mean) + 2 * np.abs(mean) * d_mean
    d_rstd = rstd * (d_var / (2 * (var + p.ln_eps)) + 3 * U32)
    return mean, rstd, d_mean, d_rstd


def reference(p, with_err=True):
    """-> out float64 [M, No] (the exact value whose roundings the kernel stores), err float64 [M, No]: the bound of everything in front of the store,
    v1: the value the first rounding sees (out - bias2).  with_err = False (the exact families) leaves the absolute sums out: err is then meaningless"""
    x, w = p.x.astype(F64), p.w.astype(F64)
    acc = _matmul_sets(p, x, w)
    S = _matmul_sets(p, np.abs(x), np.abs(w)) if with_err else np.zeros_like(acc)
    e_acc = (p.K + 8 + p.splits) * U32
    v = acc
    if p.ln_stats is not None:
        mean, rstd, d_mean, d_rstd = (t[:, None] for t in ln_rows64(p))
        ws, lnb = p.ln_wsum.astype(F64)[None], p.ln_bias.astype(F64)[None]
        inner = acc - mean * ws
        v = rstd * inner + lnb
        err = (rstd * (e_acc * S + d_mean * np.abs(ws) + 2 * U32 * (np.abs(acc) + np.abs(mean * ws))) + d_rstd * np.abs(inner)
               + 2 * U32 * (np.abs(rstd * inner) + np.abs(lnb)))
        S = None
    add = np.zeros((p.M, p.N))
    if p.bias is not None:
        add = add + p.bias.astype(F64)[None]
    if p.bias32 is not None:
        add = add + p.bias32.astype(F64)[row_set(p)]
    if p.rowbias is not None:
        add = add + p.rowbias.astype(F64)[np.arange(p.M) // p.rows_per_rb]
    v = v + add
    if S is not None:
        S = S + np.abs(add)
        err = None
    else:
        err = err + 4 * U32 * (np.abs(v) + np.abs(add))
    if p.geglu:
        xi, gi = geglu_rows(p.N, p.geglu)
        e = e_acc * S if err is None else err
        xv, gv = v[:, xi], v[:, gi]
        out = xv * gelu_erf64(gv)
        err = np.abs(gelu_erf64(gv)) * e[:, xi] + np.abs(xv) * (1.13 * e[:, gi] + 1.25 * GEGLU_GELU_ERR * np.maximum(1.0, np.abs(gv) / 5.0)) + 6 * U32 * np.abs(out)
        return SimpleNamespace(out=out, err=err, v1=out)
    if p.act or p.gate is not None:
        e = e_acc * S if err is None else err
        mag = np.abs(v)
        if p.act:
            a = 2.0 * math.log2(math.e) * GELU_C * np.abs(v + 0.044715 * v ** 3)
            v = gelu_tanh64(v)
            e = 1.13 * e + np.abs(v) * (6 + 2.1 * a) * U32
            mag = np.abs(v)
        if p.gate is not None:
            gt = p.gate.astype(F64)[np.arange(p.M) // p.rows_per_gate]
            v, e, mag = v * gt, e * np.abs(gt), mag * np.abs(gt)
        err = e + 4 * U32 * (mag + (np.abs(p.R.astype(F64)) if p.R is not None else 0.0))
        if p.R is not None:
            v = v + p.R.astype(F64)
    elif p.R is not None:
        r = p.R.astype(F64)
        v = v + r
        err = e_acc * (S + np.abs(r)) if err is None else err + 2 * U32 * (np.abs(v) + np.abs(r))
    elif err is None:
        err = e_acc * S
    out = v + p.bias2.astype(F64)[None] if p.bias2 is not None else v
    return SimpleNamespace(out=out, err=err, v1=v)


def bound(p, r):
    b = U16 * np.abs(r.v1) * (1 + 2 * U16) + SUB + r.err * (1 + U16)
    if p.bias2 is not None:
        b = b + U16 * np.abs(r.out) + SUB
    return b


def exact_output(p, r):
    """integer / one-hot families: every float32 partial sum is an exact integer below 2^24, so the output is fp16(v), or fp16(fp16(v) + bias2)"""
    y = r.v1.astype(np.float16)
    if p.bias2 is not None:
        y = (y.astype(F64) + p.bias2.astype(F64)[None]).astype(np.float16)
    return y


def stats_ref(y16):
    """(sum, sum of squares) float64 [M, N / 160, 2] of the fp16 values AS STORED, and their bound (24 float32 roundings deep)"""
    y = y16.astype(F64).reshape(y16.shape[0], -1, 160)
    st = np.stack([y.sum(2), (y * y).sum(2)], axis=-1)
    bnd = np.stack([24 * U32 * np.abs(y).sum(2), 24 * U32 * (y * y).sum(2)], axis=-1)
    return st, bnd


# ------------------------------------------------------------------------------------------------ float32 / fp16 emulation
def emu_partials(p, only=None, drop_last_k=False, drop_tail_tile=False, sets=None):
    """float32 partial sums [splits][M, N]: k tiles of 64 accumulated in float32, split s over the tiles [s ktps, (s + 1) ktps).
    only: compute that split alone.  drop_last_k / drop_tail_tile: the planted K defects.  sets: another set per row."""
    nk = (p.K + BK - 1) // BK
    ktps = p.ktps if p.splits > 1 else nk
    x, w = p.x.astype(F32), p.w.astype(F32)
    if drop_last_k:
        x = x.copy()
        x[:, p.K - 1] = 0
    out = []
    for s in range(p.splits):
        if only is not None and s != only:
            out.append(None)
            continue
        acc = np.zeros((p.M, p.N), dtype=F32)
        for kt in range(s * ktps, min((s + 1) * ktps, nk)):
            if drop_tail_tile and kt == nk - 1:
                continue
            k0, k1 = kt * BK, min((kt + 1) * BK, p.K)
            acc += _matmul_sets(p, x[:, k0:k1], w[:, :, k0:k1], sets)
        out.append(acc)
    return out


def emu_ln_rows(p):
    st = p.ln_stats
    s1, s2 = np.zeros(p.M, dtype=F32), np.zeros(p.M, dtype=F32)
    for e in range(st.shape[1]):
        s1 = s1 + st[:, e, 0]
        s2 = s2 + st[:, e, 1]
    inv = F32(1.0) / F32(p.K)
    mean = s1 * inv
    var = np.maximum(_fma(-mean, mean, s2 * inv), F32(0.0))
    return mean, (1.0 / np.sqrt((var + F32(p.ln_eps)).astype(F64))).astype(F32)


def emu_epilogue(p, parts, defect=None, geo=None):
    """splitk_reduce_kernel's sum in split order, then the epilogue in float32 -> (y fp16 [M, No], stats float32 [M, N / 160, 2] or None).
    defect: one of DEFECTS; geo: what the epilogue defects need to know of the launch (tile_n, tile_m, tile_gm, ldr, ldy)."""
    acc = parts[0].copy()
    for s in range(1, len(parts)):
        if defect == "split_dropped" and s == 1:
            continue
        acc += parts[s]
        if defect == "split_twice" and s == 1:
            acc += parts[s]
    rows = np.arange(p.M)
    v = acc
    if p.ln_stats is not None:
        mean, rstd = emu_ln_rows(p)
        if defect == "ln_next_row":
            mean, rstd = np.roll(mean, -1), np.roll(rstd, -1)
        t = _fma(np.broadcast_to(-mean[:, None], v.shape), np.broadcast_to(p.ln_wsum[None], v.shape), v)
        v = _fma(np.broadcast_to(rstd[:, None], v.shape), t, np.broadcast_to(p.ln_bias[None], v.shape))
    if p.bias is not None or p.bias32 is not None:
        sets = row_set(p)
        if defect == "set_neighbour":
            sets = (sets + 1) % p.w.shape[0]
        b = np.broadcast_to(p.bias.astype(F32)[None], v.shape) if p.bias is not None else p.bias32[sets]
        if defect == "no_bias_ragged_tile":
            b = b.copy()
            b[:, (p.N // geo.tile_n) * geo.tile_n:] = 0
        v = v + b
    if p.rowbias is not None:
        i = rows // p.rows_per_rb
        v = v + p.rowbias.astype(F32)[(i + 1) % p.rowbias.shape[0] if defect == "rowbias_neighbour" else i]
    if p.geglu:
        xi, gi = geglu_rows(p.N, p.geglu)
        if defect == "geglu_swapped":
            xi, gi = gi, xi
        with np.errstate(over="ignore"):           # (a planted defect may overflow fp16: inf is what the store would give)
            return emu_geglu_erf2(v[:, xi], v[:, gi]).astype(np.float16), None
    if p.act:
        v = emu_gelu_tanh(v)
    if p.gate is not None:
        i = rows // p.rows_per_gate
        v = v * p.gate.astype(F32)[(i + 1) % p.gate.shape[0] if defect == "gate_neighbour" else i]
    if p.R is not None:
        R = p.R
        if defect == "R_with_ldy":          # the residual rows read ldy apart in a buffer whose rows are ldr apart
            buf = np.zeros((p.M, geo.ldr), dtype=np.float16)
            buf[:, :p.N] = p.R
            R = buf.ravel()[(rows[:, None] * geo.ldy + np.arange(p.N)[None]) % buf.size]
        v = v + R.astype(F32)
    if p.bias2 is not None and defect == "bias2_before_rounding":
        y = (v + p.bias2.astype(F32)[None]).astype(np.float16)
    else:
        y = v.astype(np.float16)
        if p.bias2 is not None:
            y = (y.astype(F32) + p.bias2.astype(F32)[None]).astype(np.float16)
    st = None
    if p.stats_out:
        t = (v if defect == "stats_unrounded" else y.astype(F32)).reshape(p.M, -1, 160)
        st = np.stack([t.sum(2, dtype=F32), (t * t).sum(2, dtype=F32)], axis=-1)
        if defect == "stats_neighbour_slot":
            st = np.roll(st, 1, axis=1)
    if defect == "tile_groups_swapped":     # row tile 0 (first group) and row tile tile_gm (second group) take each other's place
        a, b = slice(0, geo.tile_m), slice(geo.tile_gm * geo.tile_m, (geo.tile_gm + 1) * geo.tile_m)
        y = y.copy()
        y[a], y[b] = y[b].copy(), y[a].copy()
    return y, st


DEFECTS = ("last_k_dropped", "tail_tile_dropped", "split_dropped", "split_twice", "no_bias_ragged_tile", "rowbias_neighbour", "gate_neighbour",
           "set_neighbour", "R_with_ldy", "bias2_before_rounding", "stats_unrounded", "stats_neighbour_slot", "geglu_swapped", "tile_groups_swapped",
           "ln_next_row")


def emulate(p, defect=None, geo=None, parts=None):
    """the stand-in for the kernel.  parts: the partial sums of the sound emulation (emu_partials(p)), reused where the defect leaves them alone"""
    if defect in ("last_k_dropped", "tail_tile_dropped"):
        last = p.splits - 1
        new = emu_partials(p, only=last, drop_last_k=defect == "last_k_dropped", drop_tail_tile=defect == "tail_tile_dropped")[last]
        parts = (list(parts[:last]) if parts is not None else emu_partials(p)[:last]) + [new]
    elif defect == "set_neighbour":
        parts = emu_partials(p, sets=(row_set(p) + 1) % p.w.shape[0])
    elif parts is None:
        parts = emu_partials(p)
    return emu_epilogue(p, parts, defect, geo)
