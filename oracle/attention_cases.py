"""The cases of tests/test_gpu_attention.py: for every kernel of the attention launch table (csrc/attention.hip: ATTN_KERNELS) the smallest
problem that selects it and still leaves a ragged tail in every tiling the kernel has, and three data families per case.

Shapes.  BF = 2 frames, 2 heads (head-major block order and per-frame source rows can both go wrong visibly), four source blocks of which
the source tables name three, in an order that is not the identity; q, k, v are column slices of ONE fused buffer (ldq = ldkv = 3C) and the
output has ldo = C + 8.  Queries:
70 (one 64-row block + 6 rows), 520 (4 x 128 + 8), 2088 (8 x 256 + 40), 1064 / 200 (the d = 64 pipelined kernel), 257 (the text kernel).
Keys: 141 per source in two sources (two 64-key tiles + 13 keys: the tail mask runs once per source); 13 and 80 for the text kernel (inside
its first key fragment, the end of its last); 81, 100, 128 in one source and 77 weighted by src_logw for the register-staged d = 40 kernel;
per body one case of three sources with src_cnt = (1, 3) and multiplicities, and one of a single key.

Families (build(case, family)):
  random   seeded normal q, k, v; source block 2's K x 2.5 (peaked scores); per frame one key of the last tile set to 4 q[i] (a late, large
           reference jump) and one query to -16 k[j] (strongly negative scores); where a source has 64 keys or more, its first 32 keys equal and
           a query at -16 times that key (a strongly negative FIRST reference);
  uniform  q = 0: every score is 0, every probability 2^lw (multiplicities 1, 2, 4 here: exact in fp16), V small integers: the float64 mean is
           what the kernel must give to one store rounding;
  onehot   k rows are +-a sign patterns (16 columns spread over the head) that spell the key's number, q[i] = the pattern of ONE key chosen by
           a fixed permutation over all sources, tiles, tail positions and heads: its score beats every other by 2 a^2 c > 40 log2 units, so
           the output is that key's V row (integers 1 .. 2047 with alternating signs, exact in fp16) bit for bit."""
import functools
import math
from types import SimpleNamespace

import numpy as np

from oracle import attention_ref as ar

BF, HEADS, S = 2, 2, 4                     # source blocks 0..2 are named by the tables, block 3 by none: no launch may read it
PAD = 8                                   # ldo = C + PAD
SRC_IDX = {1: [[2], [1]], 2: [[2, 0], [1, 2]], 3: [[2, 0, 1], [1, 2, 0]]}
MERGE_IDX = {1: [[0], [2]], 2: [[1, 2], [0, 1]]}        # the source table of a second launch (two-phase tests)
LOGW_RANDOM = [[math.log2(3.0), 0.0, 1.0], [1.0, math.log2(3.0), 0.0]]
LOGW_EXACT = [[1.0, 0.0, 2.0], [2.0, 1.0, 0.0]]
PLAN_SRC_LOGW = 1
FAMILIES = ("random", "uniform", "onehot")
DPAD = {16: (32, 1), 32: (32, 2), 40: (64, 3), 64: (64, 4), 80: (96, 5), 160: (160, 10)}


def _case(name, sym, Nq, Nkv, nsrc, d, pre, phase=0, logw=False, cnt=None):
    return SimpleNamespace(name=name, sym=sym, BF=BF, heads=HEADS, Nq=Nq, Nkv=Nkv, nsrc=nsrc, d=d, pre=pre, phase=phase, logw=logw, cnt=cnt)


def _make():
    cs = []
    for tp in (0, 1, 2):
        for d, (dpad, dv16) in DPAD.items():
            for cf in ((False, True) if dpad >= 96 else (False,)):
                t = "true" if cf else "false"
                big = "attn_kernel" if dpad == 160 else "attn_kernel_occ3"
                cs.append(_case(f"body_d{d}_q70_{t}_tp{tp}", f"attn_kernel<{dpad},{dv16},1,{t},{tp}>", 70, 141, 2, d, cf, tp))
                cs.append(_case(f"body_d{d}_q520_{t}_tp{tp}", f"{big}<{dpad},{dv16},2,{t},{tp}>", 520, 141, 2, d, cf, tp))
        cs.append(_case(f"pp40_tp{tp}", f"attn_pp40_kernel<0,1,true,{tp}>", 2088, 141, 2, 40, True, tp))
        cs.append(_case(f"pp64_q1064_tp{tp}", f"attn_pp64_kernel<0,{tp}>", 1064, 141, 2, 64, True, tp))
    cs.append(_case("pp64_q200_tp2", "attn_pp64_kernel<0,2>", 200, 141, 2, 64, True, 2))
    for d in (16, 32, 40, 64):
        dpad, dv16 = DPAD[d]
        cs.append(_case(f"occ2_d{d}", f"attn_kernel_occ2<{dpad},{dv16},4>", 2088, 141, 2, d, False))
    for d in (40, 80):
        for nkv in (13, 80):
            cs.append(_case(f"text_d{d}_k{nkv}", f"attn_text_kernel<{d}>", 257, nkv, 1, d, d == 40))
    for nkv in (81, 100, 128):
        cs.append(_case(f"pp40reg_k{nkv}", "attn_pp40_kernel<1,0,false,0>", 2088, nkv, 1, 40, True))
    cs.append(_case("pp40reg_k77_logw", "attn_pp40_kernel<1,0,false,0>", 2088, 77, 1, 40, True, logw=True))
    # per body: three sources with src_cnt = (1, 3) and multiplicities; a single key
    cs.append(_case("body_d16_3src", "attn_kernel<32,1,1,false,0>", 70, 141, 3, 16, False, logw=True, cnt=(1, 3)))
    cs.append(_case("body_d40_3src", "attn_kernel<64,3,1,false,0>", 70, 141, 3, 40, False, logw=True, cnt=(1, 3)))
    cs.append(_case("body_d80_3src_cf", "attn_kernel_occ3<96,5,2,true,0>", 520, 141, 3, 80, True, logw=True, cnt=(1, 3)))
    cs.append(_case("pp40_3src", "attn_pp40_kernel<0,1,true,0>", 2088, 141, 3, 40, True, logw=True, cnt=(1, 3)))
    cs.append(_case("pp64_3src", "attn_pp64_kernel<0,0>", 1064, 141, 3, 64, True, logw=True, cnt=(1, 3)))
    cs.append(_case("body_d32_1key", "attn_kernel<32,2,1,false,0>", 70, 1, 1, 32, False))
    cs.append(_case("pp40reg_1key", "attn_pp40_kernel<1,0,false,0>", 2088, 1, 1, 40, True, logw=True))
    cs.append(_case("pp64_1key", "attn_pp64_kernel<0,0>", 1064, 1, 1, 64, True))
    return {c.name: c for c in cs}


CASES = _make()
PHASE_CNT = {"full": (2, 1), "empty": (0, 2)}        # src_cnt of a two-phase launch: every frame with sources / frame 0 without any


def of_phase(phase):
    return [n for n, c in CASES.items() if c.phase == phase]


def plan_args(c, phase=None):
    """the arguments of univst_debug_attention_plan"""
    return (c.BF, c.heads, c.Nq, c.Nkv, c.nsrc, c.d, int(c.pre), PLAN_SRC_LOGW if c.logw else 0, c.phase if phase is None else phase)


def _logw(c, family):
    if not c.logw:
        return None
    return np.asarray(LOGW_EXACT if family == "uniform" else LOGW_RANDOM, dtype=np.float32)[:, :c.nsrc]


def _half(x):
    with np.errstate(over="raise"):
        return x.astype(np.float16)


def _key_of_query(c, bf, h, i, ntot):
    """onehot: the key (position in the frame's concatenated sources) query i of (bf, h) selects — the first queries take the last key of the
    last and of the first source, both sides of each tile boundary and the first key; the rest walk the keys with a stride coprime to them"""
    fixed = [ntot - 1, c.Nkv - 1, min(63, ntot - 1), min(64, ntot - 1), 0, min(c.Nkv, ntot - 1), min(127, ntot - 1), min(128, ntot - 1)]
    if i < len(fixed):
        return fixed[(i + h + bf) % len(fixed)]
    return (i * 37 + h * 11 + bf * 5) % ntot


def onehot_amplitude(d):
    """|k| = |q| of the 16 columns that carry the pattern: two keys differ in at least one of them, so the selected key leads by 2 a^2 c > 40
    log2 units, while the scores stay small enough (16 a^2 c < 1100) that a float32 rounding of the reference is far below half an fp16 step"""
    return 8.0 if 128.0 * ar.scale_log2e(d) > 41.0 else 16.0


def _pattern(code, d):
    """[d]: the low 12 bits of `code` as +-1 in 16 columns spread over the head (bits 0..3 twice), 0 elsewhere"""
    out = np.zeros(d)
    out[(np.arange(16) * d) // 16] = 2.0 * ((code >> (np.arange(16) % 12)) & 1) - 1.0
    return out


@functools.lru_cache(maxsize=None)
def build(name, family, cnt_key=None):
    """-> Problem (oracle/attention_ref.py) with .case, .family, .select (onehot: [BF, heads, Nq] the (source block, key) each query selects).
    cnt_key: a key of PHASE_CNT instead of the case's own src_cnt (two-phase launches need one)."""
    c = CASES[name]
    C, d = c.heads * c.d, c.d
    rows = max(c.BF * c.Nq, S * c.Nkv)
    cnt = c.cnt if cnt_key is None else PHASE_CNT[cnt_key]
    if cnt is not None:
        cnt = tuple(min(n, c.nsrc) for n in cnt)
    rng = np.random.default_rng(abs(hash_name(name)) % (2 ** 31))
    buf = rng.standard_normal((rows, 3 * C))
    q = buf[:c.BF * c.Nq, :C].reshape(c.BF, c.Nq, C)
    k = buf[:S * c.Nkv, C:2 * C].reshape(S, c.Nkv, C)
    v = buf[:S * c.Nkv, 2 * C:].reshape(S, c.Nkv, C)
    src = np.asarray(SRC_IDX[c.nsrc], dtype=np.int32)
    select = None
    if family == "random":
        k[2] *= 2.5
        for bf in range(c.BF):
            n = c.nsrc if cnt is None else cnt[bf]
            if n == 0 or c.Nkv < 4:
                continue
            first, last = int(src[bf, 0]), int(src[bf, n - 1])
            if c.Nkv >= 64:
                k[first, :32] = k[first, 3]
                q[bf, 7 + bf] = -16.0 * _half(k[first, 3]).astype(np.float64) / (2.5 if first == 2 else 1.0)
            q[bf, 9 + bf] = -16.0 * _half(k[first, c.Nkv // 2]).astype(np.float64) / (2.5 if first == 2 else 1.0)
            k[last, c.Nkv - 1 - bf] = 4.0 * q[bf, 5 + bf]          # frame 0: the very last key of the tail
    elif family == "uniform":
        q[:] = 0.0
        g = np.arange(S * c.Nkv)[:, None]
        col = np.arange(C)[None, :]
        v[:] = (((g * 7 + col * 3 + (col // d) * 5) % 17) - 8 + 3 * (g // c.Nkv)).reshape(S, c.Nkv, C)
    else:
        g = np.arange(S * c.Nkv)
        for h in range(c.heads):
            pat = np.stack([_pattern(int(i) * 2 + h + 1, d) for i in g])                     # [S * Nkv, d], distinct rows
            k[:, :, h * d:(h + 1) * d] = onehot_amplitude(d) * pat.reshape(S, c.Nkv, d)
        col = np.arange(C)[None, :]
        n = 1 + ((g[:, None] * C + col) * 5) % 2047
        v[:] = (n * np.where((g[:, None] + col) % 2 == 0, 1.0, -1.0)).reshape(S, c.Nkv, C)
        select = np.zeros((c.BF, c.heads, c.Nq, 2), dtype=np.int64)
        q[:] = 0.0
        for bf in range(c.BF):
            n_src = c.nsrc if cnt is None else cnt[bf]
            for h in range(c.heads):
                for i in range(c.Nq):
                    if n_src == 0:
                        continue
                    j = _key_of_query(c, bf, h, i, n_src * c.Nkv)
                    blk, key = int(src[bf, j // c.Nkv]), j % c.Nkv
                    select[bf, h, i] = (blk, key)
                    q[bf, i, h * d:(h + 1) * d] = k[blk, key, h * d:(h + 1) * d]
    buf16 = _half(buf)
    if c.pre:                              # q' = fp16(q c): rounded once, as the folded to_q weights give it; the reference sees q' / c
        q16 = buf16[:c.BF * c.Nq, :C].astype(np.float64)
        buf16[:c.BF * c.Nq, :C] = _half(q16 * ar.scale_log2e(d))
    p = ar.Problem(buf16, c.BF, c.heads, c.Nq, c.Nkv, S, d, c.pre, src, None if cnt is None else np.asarray(cnt, dtype=np.int32), _logw(c, family))
    p.case, p.family, p.select = c, family, select
    return p


def hash_name(name):
    h = 0
    for ch in name:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def merge_problem(p, cnt_key):
    """the same operands as the SECOND launch of a two-phase attention sees them: another source table, its own src_cnt"""
    c = p.case
    cnt = tuple(min(n, c.nsrc) for n in PHASE_CNT[cnt_key])
    m = ar.Problem(p.buf, c.BF, c.heads, c.Nq, c.Nkv, S, c.d, c.pre, MERGE_IDX[c.nsrc], np.asarray(cnt, dtype=np.int32), p.src_logw)
    m.case, m.family, m.select = c, p.family, None
    return m


def used_rows(p):
    """boolean masks over the rows of the fused buffer: (rows whose q columns a launch reads, rows whose k | v columns one reads)"""
    c = p.case
    rows = p.buf.shape[0]
    qrows = np.arange(rows) < c.BF * c.Nq
    kv = np.zeros(rows, dtype=bool)
    for bf in range(c.BF):
        for blk, _ in p.sources(bf):
            kv[blk * c.Nkv:(blk + 1) * c.Nkv] = True
    return qrows, kv


def poisoned(p):
    """a copy of the fused buffer with NaN in every element no launch may read: q columns of rows past BF * Nq, k | v columns of rows past
    the source blocks and of source blocks that no src_idx row names"""
    qrows, kv = used_rows(p)
    buf = p.buf.copy()
    buf[~qrows, :p.C] = np.nan
    buf[~kv, p.C:] = np.nan
    return buf


def uniform_bound(p, r):
    """uniform family: integer numerators and denominators are exact in fp32 (the multiplicities are powers of two); 1 / l, the product and
    the store remain"""
    return ar.store_bound(r.out) + 4 * ar.U * np.abs(r.out)


def selected_rows(p):
    """onehot: the V rows the queries select, fp16 [BF, Nq, C] (zero rows for a frame without sources)"""
    c, v = p.case, p.v16()
    want = np.zeros((c.BF, c.Nq, p.C), dtype=np.float16)
    for bf in range(c.BF):
        if not p.sources(bf):
            continue
        for h in range(c.heads):
            want[bf, :, h * c.d:(h + 1) * c.d] = v[p.select[bf, h, :, 0], h, p.select[bf, h, :, 1]]
    return want


def chain_first_symbol(c):
    """the kernel the first launch of case c's shape takes (the plan tree of uv_attention_plan for phase 1, restated for the shapes of the
    cases; tests/test_attention_cases.py holds the library to it)"""
    if c.d == 40 and c.pre and c.Nq >= 2048:
        return "attn_pp40_kernel<0,1,true,1>"
    if c.d == 64 and c.pre and c.Nq >= 1024:
        return "attn_pp64_kernel<0,1>"
    dpad, dv16 = DPAD[c.d]
    qb = 2 if c.Nq >= 512 else 1
    cf = "true" if dpad >= 96 and c.pre else "false"
    return f"{'attn_kernel_occ3' if qb == 2 and dpad <= 96 else 'attn_kernel'}<{dpad},{dv16},{qb},{cf},1>"
