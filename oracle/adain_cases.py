"""Designed inputs for tests/test_gpu_adain.py (csrc/pnp.hip and the SD3 shift of csrc/sd3.hip through the C ABI), the path each takes
through the kernels, and the bounds their outputs are held to.

The kernels have no plan read-out: which loop a row falls into is a few lines of integer arithmetic, restated here in plain Python
(shift_path, sd3_path, latent_path) next to the kernel lines it mirrors.  Every case names the path values it is there for (EXPECT);
tests/test_adain_cases.py holds the restatement to them without a GPU, shows that a float32 emulation in the kernels' own order meets the
bounds, and that the defects the cases are there to catch move the float64 reference by more than 8 bounds.

Base data of the geometry cases: 0.2 + 1.5 n rounded to fp16.  On top of them SENTINEL style rows carry + 32 x 1.5 on every K | V column,
at the rows each loop boundary of colstats_kernel owns (row 31, row 32, the last row an unrolled iteration reads, the first row of the
32-row tail, row N - 1), in the first and the last frame.  The SD3 cases carry them on the stylised rows as well: sd3_group_stats reads
colstats of that branch too."""
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

from oracle import adain_ref as ar

SENTINEL = 32.0
ALPHA, BETA, GAMMA = 0.65, 0.484, 3.0                 # the UNet plugin's alpha / gamma, beta of step 13 of a 0 .. 25 window
SD3_ALPHA, SD3_GAMMA = 0.8, 2.0                       # what csrc/sd3.hip passes

ShiftCase = namedtuple("ShiftCase", "name F N C heads values")          # heads = 0: the UNet shift
LatentCase = namedtuple("LatentCase", "name C F h w values")


# ------------------------------------------------------------------------------------------------ paths
def colstats_phases(N):
    """colstats_kernel, per row phase t = 0 .. 31 (thread row tr): None when the phase is empty (tr >= N), else
    (unrolled iterations, tail iterations, rows read by the unrolled loop, rows read by the tail loop).  Row t itself is the pivot."""
    out = []
    for t in range(32):
        if t >= N:
            out.append(None)
            continue
        r, un, tail, urows, trows = t + 32, 0, 0, [], []
        while r + 224 < N:                             # for (; r + 224 < N; r += 256): rows r, r + 32, .. r + 224
            urows += [r + 32 * u for u in range(8)]
            un, r = un + 1, r + 256
        while r < N:                                   # for (; r < N; r += 32)
            trows.append(r)
            tail, r = tail + 1, r + 32
        assert 1 + len(urows) + len(trows) == (N - t + 31) // 32          # the merge weight nt
        out.append((un, tail, urows, trows))
    return out


def shift_path(F, N, C):
    """what uv_launch_adain_shift launches for (F, N, C), and which loops of colstats_kernel its rows fall into"""
    nch8 = C // 8                                      # 16-byte chunks per row: lane + 64 i < nch8
    nch = (nch8 + 63) // 64
    ph = [p for p in colstats_phases(N) if p is not None]
    return dict(inst=1 if nch <= 1 else 2 if nch == 2 else 4, nch=nch, lanes_last=nch8 - 64 * (nch - 1),
                empty_phases=32 - len(ph), unrolled=tuple(sorted({p[0] for p in ph})), tail=tuple(sorted({p[1] for p in ph})),
                phases_unrolled=sum(p[0] > 0 for p in ph), phases_tail=sum(p[1] > 0 for p in ph),
                col_blocks=(2 * C + 63) // 64, col_partial=(2 * C) % 64 != 0,
                row_blocks=(F * N + 3) // 4, row_ragged=(F * N) % 4 != 0)


def sd3_path(F, N, C, heads):
    p = shift_path(F, N, C)
    return dict(stats_blocks=(F * 2 * heads + 127) // 128, d=C // heads, idle_lanes=C < 64, empty_phases=p["empty_phases"], unrolled=p["unrolled"],
                tail=p["tail"], col_partial=p["col_partial"], row_ragged=p["row_ragged"])


def latent_path(C, F, h, w):
    """the 1024-thread blocks of latent_adain_kernel / _stats / _apply: strides over a frame (HW) and over the channel (n)"""
    HW, n = h * w, F * h * w
    return dict(HW=HW, n=n, idle_threads=max(0, 1024 - HW), strides_hw=-(-HW // 1024), ragged_hw=HW % 1024 != 0, strides_n=-(-n // 1024))


def sentinel_rows(N):
    ph = [p for p in colstats_phases(N) if p is not None]
    rows = {31, 32, N - 1}
    urows = [r for p in ph for r in p[2]]
    trows = [r for p in ph for r in p[3]]
    if urows:
        rows.add(max(urows))
    if trows:
        rows.add(min(trows))
    return sorted(r for r in rows if 0 <= r < N)


# ------------------------------------------------------------------------------------------------ cases
def _s(name, F, N, C, heads=0, values="normal"):
    return ShiftCase(name, F, N, C, heads, values)


SHIFT_GEOMETRY = [
    _s("g1_n2_empty_phases", 1, 2, 8),
    _s("g2_ragged_rows_partial_cols", 3, 5, 40),
    _s("g3_phases_of_2_and_1_rows", 2, 40, 64),
    _s("g4_one_phase_unrolled", 1, 257, 320),
    _s("g5_inst2_12_tail_phases", 2, 300, 640),
    _s("g6_two_unrolled_nch3", 1, 577, 1032),
    _s("g7_inst4_c1280", 2, 33, 1280),
    _s("g8_width_limit", 1, 64, 2048),
    _s("g9_4096_blocks", 4, 4096, 64),
]
SHIFT_VALUES = [_s(f"v_{v}", 2, 300, 640, 0, v) for v in ("mean30", "mean800", "const_row", "const_col")]
SD3_GEOMETRY = [
    _s("s1_smallest", 1, 2, 24, 3),
    _s("s2_two_stats_blocks", 3, 5, 1536, 24),
    _s("s3_d8_idle_lanes", 2, 300, 40, 5),
    _s("s4_sd35_large_text", 1, 333, 2432, 38),
    _s("s5_ragged_rows_partial_cols", 3, 5, 40, 5),
]
SD3_VALUES = [_s(f"sv_{v}", 2, 300, 1536, 24, v) for v in ("mean30", "mean800")]
SHIFT_CASES = {c.name: c for c in SHIFT_GEOMETRY + SHIFT_VALUES}
SD3_CASES = {c.name: c for c in SD3_GEOMETRY + SD3_VALUES}
LD_CASE = "g2_ragged_rows_partial_cols"
SD3_LD_CASE = "s5_ragged_rows_partial_cols"
LD_PAD, LD_TAIL_ROWS = 24, 40

_G5 = dict(inst=2, nch=2, lanes_last=16, empty_phases=0, unrolled=(1,), tail=(0, 1), phases_tail=12, col_blocks=20, col_partial=False, row_ragged=False)
EXPECT = {
    "g1_n2_empty_phases": dict(inst=1, nch=1, lanes_last=1, empty_phases=30, unrolled=(0,), tail=(0,), col_blocks=1, col_partial=True, row_blocks=1, row_ragged=True),
    "g2_ragged_rows_partial_cols": dict(inst=1, nch=1, lanes_last=5, empty_phases=27, col_blocks=2, col_partial=True, row_blocks=4, row_ragged=True),
    "g3_phases_of_2_and_1_rows": dict(inst=1, empty_phases=0, unrolled=(0,), tail=(0, 1), phases_tail=8, col_blocks=2, col_partial=False),
    "g4_one_phase_unrolled": dict(inst=1, nch=1, lanes_last=40, unrolled=(0, 1), phases_unrolled=1, tail=(0, 7), phases_tail=31, row_ragged=True),
    "g5_inst2_12_tail_phases": _G5,
    "g6_two_unrolled_nch3": dict(inst=4, nch=3, lanes_last=1, unrolled=(2,), tail=(1, 2), phases_tail=32, col_partial=True, row_ragged=True),
    "g7_inst4_c1280": dict(inst=4, nch=3, lanes_last=32, unrolled=(0,), tail=(0, 1), phases_tail=1, col_partial=False, row_ragged=True),
    "g8_width_limit": dict(inst=4, nch=4, lanes_last=64, unrolled=(0,), tail=(1,), col_blocks=64),
    "g9_4096_blocks": dict(inst=1, unrolled=(15,), tail=(7,), row_blocks=4096, row_ragged=False),
    "s1_smallest": dict(stats_blocks=1, d=8, idle_lanes=True, empty_phases=30, col_partial=True, row_ragged=True),
    "s2_two_stats_blocks": dict(stats_blocks=2, d=64, idle_lanes=False, empty_phases=27, row_ragged=True),
    "s3_d8_idle_lanes": dict(stats_blocks=1, d=8, idle_lanes=True, unrolled=(1,), tail=(0, 1), col_partial=True),
    "s4_sd35_large_text": dict(stats_blocks=1, d=64, unrolled=(1,), tail=(1, 2), row_ragged=True),
    "s5_ragged_rows_partial_cols": dict(stats_blocks=1, d=8, idle_lanes=True, empty_phases=27, col_partial=True, row_ragged=True),
}
for _v in SHIFT_VALUES:
    EXPECT[_v.name] = _G5
for _v in SD3_VALUES:
    EXPECT[_v.name] = dict(stats_blocks=1, d=64, unrolled=(1,), tail=(0, 1))


def _l(name, C, F, h, w, values="normal"):
    return LatentCase(name, C, F, h, w, values)


LATENT_GEOMETRY = [
    _l("l1_hw6", 4, 1, 2, 3),
    _l("l2_odd", 4, 3, 5, 7),
    _l("l3_sd3_call_hw1056", 16, 1, 33, 32),
    _l("l4_16_frames_hw64", 4, 16, 8, 8),
    _l("l5_hw4096", 4, 4, 64, 64),
]
LATENT_VALUES = [_l(f"lv_{v}_{tag}", *shape, v) for v in ("mean3", "const_style_frame") for tag, shape in (("odd", (4, 3, 5, 7)), ("hw4096", (4, 4, 64, 64)))]
LATENT_CASES = {c.name: c for c in LATENT_GEOMETRY + LATENT_VALUES}
LATENT_EXPECT = {
    "l1_hw6": dict(HW=6, idle_threads=1018, strides_hw=1, strides_n=1),
    "l2_odd": dict(HW=35, n=105, strides_n=1),
    "l3_sd3_call_hw1056": dict(HW=1056, n=1056, idle_threads=0, strides_hw=2, ragged_hw=True),
    "l4_16_frames_hw64": dict(HW=64, n=1024, idle_threads=960, strides_n=1),
    "l5_hw4096": dict(HW=4096, strides_hw=4, ragged_hw=False, strides_n=16),
}
CONST_STYLE_FRAME, CONST_STYLE_VALUE = 1, 0.7


def shard_counts(F):
    return [k for k in sorted({1, 2, F}) if k <= F and F % k == 0]


# ------------------------------------------------------------------------------------------------ data
def _seed(table, name):
    return 2000 + sorted(table).index(name)


CONST_ROWS = ((0, 7), (1, 299))          # (frame, row) of the stylised branch whose K and V are constant over C
CONST_ROW_VALUE = 0.75
CONST_COLS = (5, 640 + 639)              # K column 5 and V column C - 1 of the style branch are constant over N
CONST_COL_VALUE = 1.25


@lru_cache(maxsize=4)
def build_shift(name):
    """-> qkv (fp16 [3 F N, 3C]), sentinels [(frame, row)], path, ref (ShiftRef, float64)"""
    sd3 = name in SD3_CASES
    c = (SD3_CASES if sd3 else SHIFT_CASES)[name]
    g = torch.Generator().manual_seed(_seed(SD3_CASES if sd3 else SHIFT_CASES, name))
    F, N, C = c.F, c.N, c.C
    FN = F * N
    n = torch.randn(3 * FN, 3 * C, generator=g)
    if c.values == "mean30":
        x = 7.5 + 0.25 * n
    elif c.values == "mean800":
        x = 200.0 + 0.25 * n
    else:
        x = 0.2 + 1.5 * n
    sent = []
    if c.values == "normal":
        sent = [(f, r) for f in sorted({0, F - 1}) for r in sentinel_rows(N)]
        for f, r in sent:
            x[FN + f * N + r, C:] += SENTINEL * 1.5
            if sd3:
                x[2 * FN + f * N + r, C:] += SENTINEL * 1.5
    if c.values == "const_row":
        for f, r in CONST_ROWS:
            x[2 * FN + f * N + r, C:] = CONST_ROW_VALUE
    if c.values == "const_col":
        for col in CONST_COLS:
            x[FN:2 * FN, C + col] = CONST_COL_VALUE
    qkv = x.half()
    if sd3:
        ref = ar.sd3_shift_ref(qkv, F, N, C, c.heads, SD3_ALPHA, BETA, SD3_GAMMA)
        path = sd3_path(F, N, C, c.heads)
    else:
        ref = ar.shift_ref(qkv, F, N, C, ALPHA, BETA, GAMMA)
        path = shift_path(F, N, C)
    return SimpleNamespace(case=c, qkv=qkv, sentinels=sent, path=path, ref=ref, sd3=sd3)


def shift_args(b):
    c = b.case
    return (SD3_ALPHA, BETA, SD3_GAMMA) if b.sd3 else (ALPHA, BETA, GAMMA)


def row_weight(b, frame, row, weight):
    w = torch.ones(b.case.F * b.case.N, dtype=torch.float64)
    w[frame * b.case.N + row] = weight
    return w


def latent_sentinels(c):
    """flat indices within a channel (content) and within frame 0 (style) that carry a sentinel: the last element thread 1023 reads in
    its first stride, the first of thread 0's second stride, and the last element"""
    HW, n = c.h * c.w, c.F * c.h * c.w
    return sorted({i for i in (1023, 1024, n - 1) if i < n}), sorted({i for i in (1023, 1024, HW - 1) if i < HW})


@lru_cache(maxsize=4)
def build_latent(name):
    """-> cnt, sty (fp16 [1, C, F, h, w]), path, ref (LatentRef, float64)"""
    c = LATENT_CASES[name]
    g = torch.Generator().manual_seed(_seed(LATENT_CASES, name))
    shape = (1, c.C, c.F, c.h, c.w)
    cnt = torch.randn(shape, generator=g)
    sty = 0.7 * torch.randn(shape, generator=g) + 0.1
    if c.values == "mean3":
        cnt += 3.0
    if c.values == "const_style_frame":
        sty[:, :, CONST_STYLE_FRAME] = CONST_STYLE_VALUE
    if c.values == "normal" and c.h * c.w > 6:
        ci, si = latent_sentinels(c)
        cnt.view(c.C, -1)[:, ci] += SENTINEL
        sty[0, :, 0].reshape(c.C, -1)[:, si] += SENTINEL * 0.7          # a view: frame 0 of a contiguous tensor
    cnt, sty = cnt.half(), sty.half()
    return SimpleNamespace(case=c, cnt=cnt, sty=sty, path=latent_path(c.C, c.F, c.h, c.w), ref=ar.latent_adain_ref(cnt, sty))


# ------------------------------------------------------------------------------------------------ bounds
def shift_bound(b, ref=None):
    """[F N, 3C] float64 for the stylised rows: what |kernel - ref| may be, element by element (derivation: tests/test_gpu_adain.py).
        K | V:  2^-11 |ref| + K 2^-24 (T + beta r sigma_s A + 4 beta sigma_s) + 2^-25,   T = beta (|x - mu| r sigma_s + |m_s|) + (1 - beta) |sty|
        Q:      2^-11 |ref| + 4 * 2^-24 (|q0| + 3 |q2|) + 2^-25
    UNet shift: K = max(C / 64, N / 32) + 16, A = mean |x| of the row.  SD3 shift: K = N / 32 + 16, A = 2 mean |x| of the (frame, head) group."""
    c = b.case
    ref = b.ref if ref is None else ref
    F, N, C = c.F, c.N, c.C
    FN = F * N
    alpha, beta, gamma = shift_args(b)
    q = b.qkv.double()
    out = ref.out[2 * FN:]
    bq = 2.0 ** -11 * out[:, :C].abs() + 4 * 2.0 ** -24 * (q[:FN, :C].abs() + 3.0 * q[2 * FN:, :C].abs()) + 2.0 ** -25
    sig, m = ref.std.reshape(F, 1, 2, C), ref.mean.reshape(F, 1, 2, C)
    T = beta * ((ref.x - ref.mu).abs() * ref.r * sig + m.abs()) + (1.0 - beta) * ref.sty.abs()
    if b.sd3:
        K, A = N / 32 + 16, 2.0 * ref.A
    else:
        K, A = max(C / 64, N / 32) + 16, ref.A
    bkv = 2.0 ** -11 * out[:, C:].abs().reshape(F, N, 2, C) + K * 2.0 ** -24 * (T + beta * ref.r * sig * A + 4.0 * beta * sig) + 2.0 ** -25
    return torch.cat([bq, bkv.reshape(FN, 2 * C)], dim=1)


def store_share(b):
    """median over the K | V elements of (bound - store part) / store part: how much the bound adds to one fp16 rounding"""
    c = b.case
    bnd = shift_bound(b)[:, c.C:]
    store = 2.0 ** -11 * b.ref.out[2 * c.F * c.N:, c.C:].abs() + 2.0 ** -25
    return ((bnd - store) / store).median().item()


def latent_bound(b, pair=False):
    """[1, C, F, h, w] float64.  With z = (c - cmu) r sstd the variable part of the output, A_c / A_s the mean |content| of the channel /
    mean |style| of the (channel, frame), K = max(n, 1024) / 1024 + 16:
        one launch:  2^-11 |ref| + K 2^-24 (|z| + r sstd A_c + A_s) + 2^-25
        stats/apply: the same + |z| ((rho_c^2 + 8) + (rho_s^2 + 8)) 2^-25,  rho_c = |cmu| / sigma_c, rho_s = |s[0] - smu| / sstd (s[0]: the frame's first element, the kernel's pivot; 0 where sstd = 0)"""
    c = b.case
    ref = b.ref
    cd, sd = b.cnt.double(), b.sty.double()
    n = c.F * c.h * c.w
    K = max(n, 1024) / 1024 + 16
    cmu, csig = ref.cmu.reshape(1, c.C, 1, 1, 1), ref.csigma.reshape(1, c.C, 1, 1, 1)
    smu, sstd = ref.smu.reshape(1, c.C, c.F, 1, 1), ref.sstd.reshape(1, c.C, c.F, 1, 1)
    r = 1.0 / torch.sqrt(csig ** 2 + ar.EPS)
    z = (cd - cmu).abs() * r * sstd
    A_c = cd.abs().mean(dim=(2, 3, 4), keepdim=True)
    A_s = sd.abs().mean(dim=(3, 4), keepdim=True)
    bnd = 2.0 ** -11 * ref.out.abs() + K * 2.0 ** -24 * (z + r * sstd * A_c + A_s) + 2.0 ** -25
    if pair:
        rho_c = cmu.abs() / csig
        pv = sd[:, :, :, :1, :1]                                          # latent_adain_apply_kernel sums about the frame's first element
        rho_s = torch.where(sstd > 0, (pv - smu).abs() / sstd.clamp_min(1e-300), torch.zeros_like(sstd))
        bnd = bnd + z * ((rho_c ** 2 + 8.0) + (rho_s ** 2 + 8.0)) * 2.0 ** -25
    return bnd


def fp16_step(v):
    """spacing of the fp16 numbers at |v| (float64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return 2.0 ** (e - 10)


# ------------------------------------------------------------------------------------------------ float32 emulation, kernel order
_LANE = torch.arange(64)


def _wave_sum(v):
    """wave_sum: v += shfl_xor(v, o) for o = 32 .. 1, on the last axis (64 lanes), float32"""
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    return v


def emu_colstats(x):
    """colstats_kernel on x [F, N, cols] (fp16 values): float32 sums about the phase's pivot in row order, Chan merge of the 32 phases in
    double -> (mean, std) float32 [F, cols]"""
    F, N, cols = x.shape
    x = x.float()
    rows = -(-N // 32)
    pad = torch.zeros(F, rows * 32, cols)
    pad[:, :N] = x
    pad = pad.reshape(F, rows, 32, cols)
    valid = (torch.arange(rows * 32).reshape(rows, 32) < N)
    pv = pad[:, 0]                                                       # [F, 32, cols]: row t of phase t (zeros for an empty phase)
    s, q = torch.zeros_like(pv), torch.zeros_like(pv)
    for k in range(1, rows):
        t = (pad[:, k] - pv) * valid[k][None, :, None]
        s = s + t
        q = q + t * t
    n = torch.zeros(F, cols, dtype=torch.float64)
    mu, m2 = n.clone(), n.clone()
    for t in range(min(32, N)):
        nt = float((N - t + 31) // 32)
        st, qt = s[:, t].double(), q[:, t].double()
        mt, m2t = pv[:, t].double() + st / nt, qt - st * st / nt
        dl, ntot = mt - mu, n + nt
        m2 = m2 + m2t + dl * dl * n * nt / ntot
        mu = mu + dl * nt / ntot
        n = ntot
    var = (m2 / (N - 1 if N > 1 else 1)).clamp_min(0.0)
    return mu.float(), var.sqrt().float()


def _h(x):
    return x.half().double()


def emu_shift(qkv, F, N, C, alpha, beta, gamma):
    """uv_launch_adain_shift in float32, one rounding to fp16 at the store -> float64 [F N, 3C] (the stylised rows)"""
    FN = F * N
    f32 = torch.float32
    a, b_, g = torch.tensor(alpha, dtype=f32), torch.tensor(beta, dtype=f32), torch.tensor(gamma, dtype=f32)
    one = torch.tensor(1.0, dtype=f32)
    mean, std = emu_colstats(qkv[FN:2 * FN, C:].reshape(F, N, 2 * C))
    q = qkv.float()
    oq = g * (a * q[:FN, :C] + (one - a) * q[2 * FN:, :C])
    nch8 = C // 8
    nch = (nch8 + 63) // 64
    outs = [oq]
    for t in range(2):
        x = q[2 * FN:, (1 + t) * C:(2 + t) * C]
        xp = torch.zeros(FN, nch * 64 * 8)
        xp[:, :C] = x
        xp = xp.reshape(FN, nch, 64, 8)                                   # chunk ch = lane + 64 i
        ok = (torch.arange(nch * 64).reshape(nch, 64) < nch8)
        s = torch.zeros(FN, 64)
        for i in range(nch):
            for e in range(8):
                s = s + xp[:, i, :, e]
        mu = (_wave_sum(s) / torch.tensor(float(C), dtype=f32))[:, :1]
        qq = torch.zeros(FN, 64)
        for i in range(nch):
            for e in range(8):
                d = (xp[:, i, :, e] - mu) * ok[i][None]
                qq = qq + d * d
        rstd = 1.0 / torch.sqrt(_wave_sum(qq)[:, :1] / torch.tensor(float(C), dtype=f32) + torch.tensor(1e-5, dtype=f32))
        sp = std[:, t * C:(t + 1) * C].repeat_interleave(N, dim=0)
        mp = mean[:, t * C:(t + 1) * C].repeat_interleave(N, dim=0)
        ad = (x - mu) * rstd * sp + mp
        outs.append(b_ * ad + (one - b_) * q[FN:2 * FN, (1 + t) * C:(2 + t) * C])
    return _h(torch.cat(outs, dim=1))


def emu_sd3_shift(qkv, F, N, C, heads, alpha, beta, gamma):
    """univst_sd3_adain_shift: two colstats, sd3_group_stats_kernel in double on their float32 outputs, sd3_shift_kernel in float32"""
    FN, d = F * N, C // heads
    f32 = torch.float32
    a, b_, g, one = (torch.tensor(v, dtype=f32) for v in (alpha, beta, gamma, 1.0))
    smean, sstd = emu_colstats(qkv[FN:2 * FN, C:].reshape(F, N, 2 * C))
    cmean, cstd = emu_colstats(qkv[2 * FN:, C:].reshape(F, N, 2 * C))
    m, s = cmean.double().reshape(F, 2 * heads, d), cstd.double().reshape(F, 2 * heads, d)
    mean_g = m.sum(dim=-1) / d
    var = (((N - 1) * s * s + N * m * m).sum(dim=-1) / (float(N) * d) - mean_g * mean_g).clamp_min(0.0)
    mu = mean_g.float().repeat_interleave(d, dim=1).repeat_interleave(N, dim=0)             # [FN, 2C]
    rstd = (1.0 / torch.sqrt(var + 1e-5)).float().repeat_interleave(d, dim=1).repeat_interleave(N, dim=0)
    q = qkv.float()
    oq = g * (a * q[:FN, :C] + (one - a) * q[2 * FN:, :C])
    ad = (q[2 * FN:, C:] - mu) * rstd * sstd.repeat_interleave(N, dim=0) + smean.repeat_interleave(N, dim=0)
    return _h(torch.cat([oq, b_ * ad + (one - b_) * q[FN:2 * FN, C:]], dim=1))


def _block_sums(x, valid=None):
    """the 1024-thread strided float32 sum of the latent kernels on x [..., n]: per-thread sums in index order, wave_sum, the 16 wave
    totals added in double -> float64 [...]"""
    n = x.shape[-1]
    k = -(-n // 1024)
    pad = torch.zeros(*x.shape[:-1], k * 1024)
    pad[..., :n] = x
    pad = pad.reshape(*x.shape[:-1], k, 1024)
    s = torch.zeros(*x.shape[:-1], 1024)
    for i in range(k):
        s = s + pad[..., i, :]
    return _wave_sum(s.reshape(*x.shape[:-1], 16, 64))[..., 0].double().sum(dim=-1)


def _sq_dev(x, mu):
    d = x - mu
    return d * d


def emu_latent(cnt, sty):
    """latent_adain_kernel in float32 -> float64 [1, C, F, h, w]"""
    _, C, F, h, w = cnt.shape
    HW, n = h * w, F * h * w
    f32 = torch.float32
    c, s = cnt.float().reshape(C, n), sty.float().reshape(C, F, HW)
    cmu = (_block_sums(c).float() / torch.tensor(float(n), dtype=f32))[:, None]
    crstd = 1.0 / torch.sqrt(_block_sums(_sq_dev(c, cmu)).float()[:, None] / torch.tensor(float(n), dtype=f32) + torch.tensor(1e-5, dtype=f32))
    smu = (_block_sums(s).float() / torch.tensor(float(HW), dtype=f32))[..., None]
    sstd = torch.sqrt(_block_sums(_sq_dev(s, smu)).float()[..., None] / torch.tensor(float(HW - 1 if HW > 1 else 1), dtype=f32))
    out = (c.reshape(C, F, HW) - cmu[:, None]) * crstd[:, None] * sstd + smu
    return _h(out).reshape(1, C, F, h, w)


def emu_latent_pair(cnt, sty, shards):
    """latent_adain_stats per shard, a float32 sum of the [C, 2] results, latent_adain_apply per shard -> float64 [1, C, F, h, w]"""
    _, C, F, h, w = cnt.shape
    HW, n = h * w, F * h * w
    st = torch.zeros(C, 2)
    Fl = F // shards
    for k in range(shards):
        c = cnt[:, :, k * Fl:(k + 1) * Fl].float().reshape(C, Fl * HW)
        st = st + torch.stack([_block_sums(c).float(), _block_sums(c * c).float()], dim=1)
    mu = st[:, 0].double() / n
    var = (st[:, 1].double() / n - mu * mu).clamp_min(0.0)
    cmu, crstd = mu.float()[:, None, None], (1.0 / torch.sqrt(var + 1e-5)).float()[:, None, None]
    s = sty.float().reshape(C, F, HW)
    pv = s[..., :1]                                                      # sums about the frame's first element
    x, y = _block_sums(s - pv), _block_sums((s - pv) * (s - pv))
    m = x / HW
    v = ((y - x * m) / (HW - 1 if HW > 1 else 1)).clamp_min(0.0)
    smu, sstd = (pv[..., 0].double() + m).float()[..., None], v.sqrt().float()[..., None]
    out = (cnt.float().reshape(C, F, HW) - cmu) * crstd * sstd + smu
    return _h(out).reshape(1, C, F, h, w)
