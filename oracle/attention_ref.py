"""Float64 reference of the multi-source attention (csrc/attention.hip) on the fp16 inputs, the per-element error bounds that
tests/test_gpu_attention.py holds the kernels to (derived there), and a float32 / fp16 emulation of the kernels' tile-wise online softmax:
64-key tiles in source order, a deferred reference (DEFER = 8 log2 units), probabilities packed to fp16 round-toward-zero (or to nearest where
the kernel does), fp32 accumulation, the (m, l) state of a first phase and the merge of a second.  The emulation takes a `defect` so that
tests/test_attention_cases.py can show that the cases tell a wrong kernel from a right one.

Everything is numpy on [BF, heads, Nq, d] / [S, heads, Nkv, d] views; a Problem carries the operands exactly as the kernel sees them."""
import math
import re
from types import SimpleNamespace

import numpy as np

LOG2E = 1.4426950408889634
LN2 = math.log(2.0)
U = 2.0 ** -24            # one float32 rounding
KT = 64                   # keys per tile (attention.hip: KT)
DEFER = 8.0               # attention.hip: DEFER
DEFECTS = ("drop_last_key", "skip_rescale", "no_logw", "no_cnt", "swap_heads", "other_frame_row", "state_l_off")


def scale_log2e(d):
    return LOG2E / math.sqrt(d)


def traits(sym):
    """what the bound and the emulation need to know about a kernel symbol:
    matched   the denominator sums the packed fp16 probabilities that multiply V (ones column, fdot2, text kernel); else it sums the unrounded
              exponentials and the probabilities are rounded to nearest (attn_body without CF and without the ones column);
    quant     the reference is quantised to 1/64 (the two pipelined kernels);
    lw16      the source's log2 multiplicity rides in an fp16 column of Q' (attn_pp40_kernel: set_lw);
    ks        32-wide k steps of one score (chained QK^T MFMAs)."""
    m = re.match(r"(attn_kernel|attn_kernel_occ3|attn_kernel_occ2)<(\d+),(\d+),(\d+)(?:,(true|false),(\d))?>$", sym)
    if m:
        dpad, dv16, cf = int(m.group(2)), int(m.group(3)), m.group(5) == "true"
        return SimpleNamespace(body="attn_body", matched=cf or dv16 == 3, quant=False, lw16=False, ks=dpad // 32, cf=cf)
    if sym.startswith("attn_pp40_kernel"):
        return SimpleNamespace(body="pp40", matched=True, quant=True, lw16=True, ks=2, cf=True)
    if sym.startswith("attn_pp64_kernel"):
        return SimpleNamespace(body="pp64", matched=True, quant=True, lw16=False, ks=2, cf=True)
    m = re.match(r"attn_text_kernel<(\d+)>$", sym)
    if m:
        return SimpleNamespace(body="text", matched=True, quant=False, lw16=False, ks=(int(m.group(1)) + 31) // 32, cf=False)
    raise ValueError(sym)


class Problem:
    """The operands of one launch.  buf fp16 [rows, 3C]: q = columns 0..C of rows bf * Nq + i, k / v = columns C..2C / 2C..3C of rows
    s * Nkv + j (S source blocks).  qref float64 [BF, Nq, C]: the queries the reference uses (q, or q' / c for a prescaled q')."""

    def __init__(self, buf, BF, heads, Nq, Nkv, S, d, q_prescaled, src_idx, src_cnt=None, src_logw=None):
        self.buf, self.BF, self.heads, self.Nq, self.Nkv, self.S, self.d, self.pre = buf, BF, heads, Nq, Nkv, S, d, bool(q_prescaled)
        self.C = heads * d
        self.src_idx = np.asarray(src_idx, dtype=np.int32)
        self.nsrc = self.src_idx.shape[1]
        self.src_cnt = None if src_cnt is None else np.asarray(src_cnt, dtype=np.int32)
        self.src_logw = None if src_logw is None else np.asarray(src_logw, dtype=np.float32)
        self.c = scale_log2e(d)

    def q16(self):
        return self.buf[:self.BF * self.Nq, :self.C].reshape(self.BF, self.Nq, self.heads, self.d).transpose(0, 2, 1, 3)

    def k16(self):
        return self.buf[:self.S * self.Nkv, self.C:2 * self.C].reshape(self.S, self.Nkv, self.heads, self.d).transpose(0, 2, 1, 3)

    def v16(self):
        return self.buf[:self.S * self.Nkv, 2 * self.C:3 * self.C].reshape(self.S, self.Nkv, self.heads, self.d).transpose(0, 2, 1, 3)

    def qref(self):
        q = self.q16().astype(np.float64)
        return q / self.c if self.pre else q

    def sources(self, bf, src_idx=None, src_cnt=None, src_logw=None):
        """[(source block, log2 multiplicity)] of frame bf"""
        idx = self.src_idx if src_idx is None else np.asarray(src_idx)
        cnt = self.src_cnt if src_cnt is None else np.asarray(src_cnt)
        lw = self.src_logw if src_logw is None else np.asarray(src_logw)
        n = idx.shape[1] if cnt is None else int(cnt[bf])
        return [(int(idx[bf, s]), 0.0 if lw is None else float(lw[bf, s])) for s in range(n)]


def _rows(x):
    """[BF, heads, Nq, d] -> [BF, Nq, heads * d], the layout of the output"""
    BF, H, N, d = x.shape
    return x.transpose(0, 2, 1, 3).reshape(BF, N, H * d)


def reference(p, frames=None, detail=True):
    """float64 softmax(q k^T / sqrt(d) + ln(multiplicity)) v per frame over frames[bf] = [(source block, log2 multiplicity)] (default: the
    problem's own tables).  out [BF, Nq, C]; per (bf, head, query): lse (log2 units: log2 of the sum of 2^x), mx = max x, L = sum 2^(x - mx);
    with detail the sums the bounds are made of: A = sum_j s_j |v_j - out|, absv = sum_j s_j |v_j|, vsum = sum_j |v_j| (all [BF, Nq, C]), qk =
    max_j c sum_i |q_i k_ji|, xabs = max_j |x_j|, and per frame the key count N, the tile count T, lwmax = max |lw| and lw16 = max |lw - fp16(lw)|.
    A frame without sources has out = 0, lse = mx = -inf, L = 0."""
    BF, H, Nq, d = p.BF, p.heads, p.Nq, p.d
    q, k, v = p.qref(), p.k16().astype(np.float64), p.v16().astype(np.float64)
    cs = 1.0 / math.sqrt(d) * LOG2E
    z = lambda *s: np.zeros(s)
    r = SimpleNamespace(out=z(BF, H, Nq, d), lse=np.full((BF, H, Nq), -np.inf), mx=np.full((BF, H, Nq), -np.inf), L=z(BF, H, Nq), A=z(BF, H, Nq, d),
                        absv=z(BF, H, Nq, d), vsum=z(BF, H, 1, d), qk=z(BF, H, Nq), xabs=z(BF, H, Nq), N=np.zeros(BF), T=np.zeros(BF), lwmax=np.zeros(BF),
                        lw16=np.zeros(BF))
    for bf in range(BF):
        srcs = p.sources(bf) if frames is None else frames[bf]
        if not srcs:
            continue
        kk = np.concatenate([k[s] for s, _ in srcs], axis=1)               # [H, N, d]
        vv = np.concatenate([v[s] for s, _ in srcs], axis=1)
        lw = np.concatenate([np.full(p.Nkv, w) for _, w in srcs])
        x = q[bf] @ kk.transpose(0, 2, 1) * cs + lw                         # [H, Nq, N] log2 units
        mx = x.max(-1)
        e = np.exp2(x - mx[..., None])
        L = e.sum(-1)
        s = e / L[..., None]
        out = s @ vv
        r.out[bf], r.mx[bf], r.L[bf], r.lse[bf] = out, mx, L, mx + np.log2(L)
        r.N[bf], r.T[bf] = kk.shape[1], len(srcs) * ((p.Nkv + KT - 1) // KT)
        r.lwmax[bf] = max(abs(w) for _, w in srcs)
        r.lw16[bf] = max(abs(w - float(np.float16(w))) for _, w in srcs)
        if detail:
            r.absv[bf] = s @ np.abs(vv)
            r.vsum[bf] = np.abs(vv).sum(1, keepdims=True)
            r.qk[bf] = (np.abs(q[bf]) @ np.abs(kk).transpose(0, 2, 1)).max(-1) * cs
            r.xabs[bf] = np.abs(x).max(-1)
            step = max(8, (1 << 22) // (kk.shape[1] * d * H))               # sum_j s_j |v_j - out_i|: [H, step, N, d] at a time
            for i0 in range(0, Nq, step):
                sl = slice(i0, min(i0 + step, Nq))
                r.A[bf][:, sl] = (s[:, sl, :, None] * np.abs(vv[:, None] - out[:, sl, None])).sum(2)
    for name in ("out", "A", "absv"):
        setattr(r, name, _rows(getattr(r, name)))
    r.vsum = np.broadcast_to(_rows(np.broadcast_to(r.vsum, (BF, H, Nq, d))), (BF, Nq, H * d))
    return r


def _percol(p, x):
    """[BF, heads, Nq] -> [BF, Nq, C]"""
    return _rows(np.broadcast_to(x[..., None], x.shape + (p.d,)))


def _perframe(x):
    return np.asarray(x, dtype=np.float64)[:, None, None]


def store_bound(ref_out):
    return 2.0 ** -11 * np.abs(ref_out) + 2.0 ** -25


def rho(p, r, tr):
    """relative error of one probability against float64, [BF, heads, Nq] (test_gpu_attention.py: scores)"""
    span = r.qk + r.xabs + DEFER + r.lwmax[:, None, None]
    return LN2 * U * (tr.ks + 5) * span + 2.0 ** -22 + (LN2 * r.lw16[:, None, None] if tr.lw16 else 0.0)


def launch_terms(p, r, tr, centre=None):
    """the bound of one launch without its store; centre: the rows the packed-probability term is taken around (default: the launch's own
    result; the merge of a two-phase attention passes the rows over the union)"""
    A = r.A if centre is None else r.A + np.abs(r.out - centre)
    T, N = _perframe(r.T), _perframe(r.N)
    L = np.maximum(_percol(p, r.L), 1e-300)
    pack = 2.0 ** -10 * A if tr.matched else 2.0 ** -11 * r.absv
    score = _percol(p, rho(p, r, tr)) * A
    acc = U * ((7 * T + 3) * r.absv + (21 * T + 6) * np.abs(r.out))
    drop = 2.0 ** -24 * 1.01 * (r.vsum + N * np.abs(r.out)) / L
    return np.where(N > 0, pack + score + acc + drop, 0.0)


def bound(p, r, tr):
    """one launch, rows against reference(p): [BF, Nq, C]"""
    return launch_terms(p, r, tr) + store_bound(r.out)


def state_bound(p, r, tr):
    """|m + log2(l) - lse| of a first phase, [BF, heads, Nq] (frames without sources are checked for l == 0 instead)"""
    T, N = _perframe(r.T), _perframe(r.N)
    rel = (2.0 ** -10 if tr.matched else 0.0) + rho(p, r, tr) + U * (21 * T + 6) + 2.0 ** -24 * 1.01 * N / np.maximum(r.L, 1e-300)
    return rel / LN2 + 4 * U * (np.abs(np.where(np.isfinite(r.lse), r.lse, 0.0)) + r.xabs + DEFER + r.lwmax[:, None, None])


def merge_weights(p, r1, r2):
    """float64 weights of the two phases in the union, [BF, heads, Nq] each, and the rows over the union [BF, Nq, C]"""
    m = np.maximum(r1.lse, r2.lse)
    m = np.where(np.isfinite(m), m, 0.0)
    a1, a2 = np.exp2(r1.lse - m), np.exp2(r2.lse - m)
    den = np.maximum(a1 + a2, 1e-300)
    w1, w2 = a1 / den, a2 / den
    return w1, w2, _percol(p, w1) * r1.out + _percol(p, w2) * r2.out


def merge_bound(p, r1, r2, tr2, phase1_terms=None):
    """rows after the merge launch against the float64 rows over the union.  phase1_terms None: `out` held the float64 phase-1 rows rounded
    to fp16 and the state came from float64 (a synthetic first phase); else the bound of the first launch without its store."""
    w1, w2, want = merge_weights(p, r1, r2)
    W1, W2 = _percol(p, w1), _percol(p, w2)
    span = np.abs(np.where(np.isfinite(r1.lse), r1.lse, 0.0)) + np.abs(np.where(np.isfinite(r2.lse), r2.lse, 0.0)) + 2 * DEFER
    merge = (2.0 ** -21 + LN2 * U * _percol(p, span)) * (W1 * np.abs(r1.out) + W2 * np.abs(r2.out))
    first = W1 * (store_bound(r1.out) + (0.0 if phase1_terms is None else phase1_terms))
    b = first + W2 * launch_terms(p, r2, tr2, centre=want) + merge + store_bound(want)
    # a frame whose merge launch has no sources keeps its rows bit for bit: the test asserts that, the bound is not used there
    return want, b


def chained_bound(p, r1, r2, union, tr1, tr2):
    """two real launches against float64 over the union: every key's probability is packed once, in whichever launch, so the one-launch terms
    over the union hold (the looser of the two kernels' packing terms), plus the fp16 rounding of the phase-1 rows the merge re-reads"""
    w1, _, _ = merge_weights(p, r1, r2)
    terms = np.maximum(launch_terms(p, union, tr1), launch_terms(p, union, tr2))
    span = np.abs(np.where(np.isfinite(union.lse), union.lse, 0.0)) + 2 * DEFER
    merge = (2.0 ** -21 + LN2 * U * _percol(p, span)) * union.absv
    return terms + _percol(p, w1) * store_bound(r1.out) + merge + store_bound(union.out)


def synthetic_state(r1, shift=0.0):
    """(m, l) float32 [BF, heads, Nq, 2] with m + log2(l) = the float64 log-sum-exp: m = the row maximum + shift; l = 0 where there is no source"""
    has = np.isfinite(r1.lse)
    m = np.where(has, r1.mx + shift, 0.0).astype(np.float32)
    l = np.where(has, np.exp2(np.where(has, r1.lse, 0.0) - m.astype(np.float64)), 0.0).astype(np.float32)
    return np.stack([m, l], axis=-1)


# ------------------------------------------------------------------------------------------------ emulation
def _pack(e, rtz):
    """float32 -> fp16 as v_cvt_pkrtz_f16_f32 (toward zero) or as the (half_t) cast (to nearest), returned as float32"""
    with np.errstate(over="ignore"):
        h = e.astype(np.float16)
    if rtz:
        h = np.where(np.isinf(h), np.float16(65504.0), h)
        over = h.astype(np.float32) > e
        h = np.where(over, np.nextafter(h, np.float16(0.0)), h)
    return h.astype(np.float32)


def emulate(p, tr, phase=0, state_in=None, out_in=None, defect=None):
    """The launch in float32 / fp16.  phase 0: rows fp16 [BF, Nq, C]; phase 1: (rows, state float32 [BF, heads, Nq, 2]); phase 2: rows merged
    with out_in (fp16 rows) and state_in.  defect: one of DEFECTS."""
    assert defect in (None,) + DEFECTS
    f32 = np.float32
    BF, H, Nq, d = p.BF, p.heads, p.Nq, p.d
    q, k, v = p.q16().astype(f32), p.k16().astype(f32), p.v16().astype(f32)
    c = f32(1.0) if p.pre else f32(p.c)
    out = np.zeros((BF, H, Nq, d), dtype=np.float16)
    state = np.zeros((BF, H, Nq, 2), dtype=f32)
    prev = None if out_in is None else out_in.reshape(BF, Nq, H, d).transpose(0, 2, 1, 3)
    for bf in range(BF):
        row = bf ^ 1 if defect == "other_frame_row" and BF > 1 else bf
        srcs = p.sources(row, src_cnt=None if defect != "no_cnt" or p.src_cnt is None else np.full(BF, p.nsrc))
        if defect == "no_logw":
            srcs = [(s, 0.0) for s, _ in srcs]
        if not srcs:
            if phase == 2:
                out[bf] = prev[bf]
            continue
        M = np.zeros((H, Nq), dtype=f32)
        l = np.zeros((H, Nq), dtype=f32)
        o = np.zeros((H, Nq, d), dtype=f32)
        first, skipped, last_e = True, False, None
        for si, (s, lw) in enumerate(srcs):
            lw = f32(np.float16(lw)) if tr.lw16 else f32(lw)
            nkv = p.Nkv - 1 if defect == "drop_last_key" and si == 0 and p.Nkv > 1 else p.Nkv
            for t0 in range(0, nkv, KT):
                kt, vt = k[s][:, t0:min(t0 + KT, nkv)], v[s][:, t0:min(t0 + KT, nkv)]
                x = (q[bf] @ kt.transpose(0, 2, 1)).astype(f32) * c + lw            # [H, Nq, keys]
                mx = x.max(-1)
                move = np.full(mx.shape, True) if first else (mx - M > f32(DEFER))
                mnew = mx if first else np.maximum(M, mx)
                if tr.quant:
                    mnew = (np.floor(mnew * f32(64.0) + f32(0.5)) * f32(1.0 / 64.0)).astype(f32)
                mnew = np.where(move, mnew, M).astype(f32)
                if not first:
                    alpha = np.exp2(M - mnew).astype(f32)
                    if defect == "skip_rescale" and not skipped and move.any():
                        skipped = True                                              # this tile: the reference moves, O^T and l keep their scale
                    else:
                        o *= alpha[..., None]
                        l *= alpha
                M, first = mnew, False
                e = np.exp2((x - M[..., None]).astype(f32)).astype(f32)
                pk = _pack(e, tr.matched)
                o += (pk @ vt).astype(f32)
                l += (pk if tr.matched else e).sum(-1, dtype=f32)
                last_e = pk[..., -1] if tr.matched else e[..., -1]
        if defect == "swap_heads" and H > 1:
            o, l, M = o[::-1], l[::-1], M[::-1]
        if phase == 1:
            state[bf, ..., 0] = M
            state[bf, ..., 1] = l - last_e if defect == "state_l_off" else l
        if phase == 2:
            m1, l1 = state_in[bf, ..., 0].astype(f32), state_in[bf, ..., 1].astype(f32)
            has1 = l1 > 0
            m = np.where(has1, np.maximum(m1, M), M)
            a1 = np.where(has1, l1 * np.exp2(np.where(has1, m1 - m, 0)).astype(f32), f32(0))
            a2 = np.exp2(M - m).astype(f32)
            inv = (f32(1.0) / (a1 + l * a2)).astype(f32)
            w1, w2 = a1 * inv, a2 * inv
            out[bf] = (prev[bf].astype(f32) * w1[..., None] + o * w2[..., None]).astype(np.float16)
        else:
            out[bf] = (o * (f32(1.0) / l)[..., None]).astype(np.float16)
    rows = _rows(out)
    return (rows, state) if phase == 1 else rows
