"""Designed inputs for tests/test_gpu_rownorm.py (layernorm_kernel of csrc/norm.hip and the operators of csrc/sd3.hip through the C ABI), the
path each takes through the kernels, and the bounds their outputs are held to (derivation: tests/test_gpu_rownorm.py).

The kernels have no plan read-out: which template instance, slot, lane and wave an element falls into is a few lines of integer arithmetic,
restated here in plain Python (layernorm_path, adaln_path, rms_path, flat_path) next to the kernel lines it mirrors.  Every case names the
path values it is there for (EXPECT); tests/test_rownorm_cases.py holds the restatement to them without a GPU, shows that a float32
emulation in the kernels' own order meets the bounds, and that the defects the sentinels are there for move the float64 reference by more
than 8 bounds.

Base data: every row has its own mean and sigma (every (row, head) its own sigma for the RMS cases, every batch row its own modulation),
so a row, head or batch mix-up shows in the values; the last row's sigma is 4x the others'.  On top of them SENTINEL elements carry
+ 32 sigma: elements 0 and 7 of the 16-byte chunks that a loop boundary owns — chunk 63, 64, 127, 128, .. (the last lane of a slot and the
first of the next) and the last chunk nch - 1 — in every row of every case with more than one chunk.  The scalar RMS kernel has elements
where the others have chunks: 63, 64, 127, 128, 191, 192 and d - 1."""
import math
from collections import namedtuple
from functools import lru_cache
from types import SimpleNamespace

import torch

from oracle import rownorm_ref as rr

SENTINEL = 32.0
U = 2.0 ** -24                                         # one float32 rounding (relative)
LN_EPS, ADALN_EPS, RMS_EPS = 1e-5, 1e-6, 1e-6


def _store(ref):
    """`(half_t)(...)`: round to nearest fp16, half the smallest subnormal step absolute"""
    return 2.0 ** -11 * ref.abs() + 2.0 ** -25


def fp16_step(v):
    """spacing of the fp16 numbers at |v| (float64 tensor)"""
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -14)))
    return 2.0 ** (e - 10)


def sentinel_chunks(nch8):
    """the chunks a loop boundary owns: ch = lane + 64 i turns from lane 63 of slot i to lane 0 of slot i + 1; the last chunk"""
    if nch8 <= 1:
        return []
    s = {nch8 - 1}
    for k in range(64, nch8, 64):
        s |= {k - 1, k}
    if nch8 >= 64:
        s.add(63)
    return sorted(s)


def sentinel_cols(C):
    return [8 * ch + e for ch in sentinel_chunks(C // 8) for e in (0, 7)]


def _rows_data(g, rows, C, mean=None, sigma=None, sentinels=True):
    """-> x float32 [rows, C], per-row sigma [rows, 1]"""
    m = torch.randn(rows, 1, generator=g) if mean is None else torch.full((rows, 1), float(mean))
    s = 0.5 + 1.5 * torch.rand(rows, 1, generator=g) if sigma is None else torch.full((rows, 1), float(sigma))
    if sigma is None:
        s[-1] *= 4.0
    x = m + s * torch.randn(rows, C, generator=g)
    if sentinels:
        for col in sentinel_cols(C):
            x[:, col] += SENTINEL * s[:, 0]
    return x, s


# ------------------------------------------------------------------------------------------------ layernorm
LnCase = namedtuple("LnCase", "name rows C values")
LN_GEOMETRY = [LnCase(n, r, c, "normal") for n, r, c in (
    ("n1_c8_one_lane", 1, 8), ("n2_c320_partial_wave", 37, 320), ("n3_c512_last_of_1x4", 19, 512), ("n4_c520_first_of_2x2", 19, 520),
    ("n5_c1024_last_of_2x2", 9, 1024), ("n6_c1032_first_of_4x1", 7, 1032), ("n7_c768_clip", 7, 768), ("n8_c1280", 7, 1280),
    ("n9_c2048_cap", 5, 2048))]
LN_VALUES = [LnCase(f"v_{tag}_c{c}", 5, c, tag) for tag in ("mean300", "mean_m2000") for c in (320, 1280)]
LN_CASES = {c.name: c for c in LN_GEOMETRY + LN_VALUES}
LN_MEANS = {"mean300": (300.0, 0.5), "mean_m2000": (-2000.0, 3.0)}
LN_CONST_CASE, LN_CONST_ROWS = "n2_c320_partial_wave", ((3, 0.75), (36, -1.5))       # row 36: the one row of the partial wave


def layernorm_path(rows, C):
    """uv_launch_layernorm: nch = (C / 8 + 63) / 64 picks <1, 4>, <2, 2> or <4, 1>; a block is 4 waves of RPW rows"""
    nch8 = C // 8                                      # const int nch = C / 8  (kernel): chunk ch = lane + 64 * i < nch
    slots = (nch8 + 63) // 64                          # const int nch = (C / 8 + 63) / 64  (launcher)
    maxch, rpw = (1, 4) if slots <= 1 else (2, 2) if slots == 2 else (4, 1)
    per_block = 4 * rpw
    blocks = (rows + per_block - 1) // per_block       # dim3((rows + 15) / 16) | (rows + 7) / 8 | (rows + 3) / 4
    rem = rows - (blocks - 1) * per_block              # rows of the last block: row0 = (blockIdx.x * 4 + wave) * RPW
    full, part = rem // rpw, rem % rpw
    return dict(inst=(maxch, rpw), slots=slots, lanes_last=nch8 - 64 * (slots - 1), empty_slots=maxch - slots, blocks=blocks,
                last_full_waves=full, last_partial_rows=part, last_empty_waves=4 - full - (part > 0), adds_per_lane=8 * slots)


LN_EXPECT = {
    "n1_c8_one_lane": dict(inst=(1, 4), lanes_last=1, blocks=1, last_full_waves=0, last_partial_rows=1, last_empty_waves=3),
    "n2_c320_partial_wave": dict(inst=(1, 4), lanes_last=40, blocks=3, last_full_waves=1, last_partial_rows=1, last_empty_waves=2),
    "n3_c512_last_of_1x4": dict(inst=(1, 4), slots=1, lanes_last=64, blocks=2, last_full_waves=0, last_partial_rows=3),
    "n4_c520_first_of_2x2": dict(inst=(2, 2), slots=2, lanes_last=1, blocks=3, last_full_waves=1, last_partial_rows=1, last_empty_waves=2),
    "n5_c1024_last_of_2x2": dict(inst=(2, 2), slots=2, lanes_last=64, blocks=2, last_full_waves=0, last_partial_rows=1),
    "n6_c1032_first_of_4x1": dict(inst=(4, 1), slots=3, lanes_last=1, empty_slots=1, blocks=2, last_full_waves=3, last_empty_waves=1),
    "n7_c768_clip": dict(inst=(2, 2), slots=2, lanes_last=32, blocks=1, last_full_waves=3, last_partial_rows=1),
    "n8_c1280": dict(inst=(4, 1), slots=3, lanes_last=32, empty_slots=1, blocks=2),
    "n9_c2048_cap": dict(inst=(4, 1), slots=4, lanes_last=64, empty_slots=0, blocks=2, last_full_waves=1, last_empty_waves=3),
}
for _v in LN_VALUES:
    LN_EXPECT[_v.name] = dict(inst=(1, 4) if _v.C == 320 else (4, 1), blocks=1 if _v.C == 320 else 2)


def _seed(table, name):
    return 3000 + sorted(table).index(name)


@lru_cache(maxsize=None)
def build_ln(name):
    c = LN_CASES[name]
    g = torch.Generator().manual_seed(_seed(LN_CASES, name))
    if c.values == "normal":
        x, _ = _rows_data(g, c.rows, c.C)
    else:
        x, _ = _rows_data(g, c.rows, c.C, *LN_MEANS[c.values], sentinels=False)
    if name == LN_CONST_CASE:
        for r, v in LN_CONST_ROWS:
            x[r] = v
    x = x.half()
    gamma = (1.0 + 0.1 * torch.randn(c.C, generator=g)).half()
    beta = (0.1 * torch.randn(c.C, generator=g)).half()
    return SimpleNamespace(case=c, x=x, gamma=gamma, beta=beta, path=layernorm_path(c.rows, c.C), ref=rr.layernorm_ref(x, gamma, beta, LN_EPS),
                           sentinels=sentinel_chunks(c.C // 8) if c.values == "normal" else [])


def rowln_bound(x, ref, adds_per_lane):
    """[|x - mean| r |g| + |b|] 8 u + mean_row |x| r |g| K u + |z - b| K u + 2^-11 |z| + 2^-25,  K = 8 + adds_per_lane + 6"""
    K = 8 + adds_per_lane + 6
    xd = x.double()
    g = ref.g.abs()
    return (((xd - ref.mean).abs() * ref.r * g + ref.b.abs()) * 8 * U + xd.abs().mean(dim=1, keepdim=True) * ref.r * g * K * U
            + (ref.out - ref.b).abs() * K * U + _store(ref.out))


def ln_bound(b, ref=None):
    return rowln_bound(b.x, b.ref if ref is None else ref, b.path["adds_per_lane"])


# ------------------------------------------------------------------------------------------------ adaln_modulate
AdaCase = namedtuple("AdaCase", "name C two values")
ADA_B, ADA_N = 3, 5                                    # 15 rows: 4 blocks of 4 waves, the last with 3; b steps at rows 5 and 10
ADA_CASES = {c.name: c for c in
             [AdaCase(f"a_c{C}", C, False, "normal") for C in (8, 128, 512, 520, 1536, 2432, 4088, 4096)]
             + [AdaCase(f"a2_c{C}_two_outputs", C, True, "normal") for C in (128, 1536, 4096)]
             + [AdaCase("av_mean300_c1536", 1536, False, "mean300")]}


def adaln_path(rows, rows_per_batch, C, two):
    """adaln_modulate_kernel: one wave per row, r = blockIdx.x * 4 + wave, chunk c / 8 = lane + 64 i for i < 8, b = r / rows_per_batch"""
    nch8 = C // 8
    slots = (nch8 + 63) // 64                          # slots i with `c < C` for some lane
    blocks = (rows + 3) // 4                           # dim3((rows + 3) / 4)
    return dict(slots=slots, lanes_last=nch8 - 64 * (slots - 1), blocks=blocks, last_block_rows=rows - 4 * (blocks - 1),
                batch_steps=tuple(range(rows_per_batch, rows, rows_per_batch)), outputs=2 if two else 1, adds_per_lane=8 * slots)


_ADA_COMMON = dict(blocks=4, last_block_rows=3, batch_steps=(5, 10))
ADA_EXPECT = {
    "a_c8": dict(slots=1, lanes_last=1, outputs=1), "a_c128": dict(slots=1, lanes_last=16, outputs=1),
    "a_c512": dict(slots=1, lanes_last=64), "a_c520": dict(slots=2, lanes_last=1),
    "a_c1536": dict(slots=3, lanes_last=64), "a_c2432": dict(slots=5, lanes_last=48),
    "a_c4088": dict(slots=8, lanes_last=63), "a_c4096": dict(slots=8, lanes_last=64),
    "a2_c128_two_outputs": dict(slots=1, outputs=2), "a2_c1536_two_outputs": dict(slots=3, outputs=2),
    "a2_c4096_two_outputs": dict(slots=8, lanes_last=64, outputs=2), "av_mean300_c1536": dict(slots=3, outputs=1),
}
for _e in ADA_EXPECT.values():
    _e.update(_ADA_COMMON)


@lru_cache(maxsize=None)
def build_ada(name):
    """scale / shift are chunk views of one [B, 6C] matrix (chunks 1 / 0, transformer_3D_model.py), of a [B, 9C] one with the second pair
    in chunks 7 / 6 for the two-output form (AdaLayerNormZeroX)"""
    c = ADA_CASES[name]
    g = torch.Generator().manual_seed(_seed(ADA_CASES, name))
    rows, C = ADA_B * ADA_N, c.C
    if c.values == "normal":
        x, _ = _rows_data(g, rows, C)
    else:
        x, _ = _rows_data(g, rows, C, 300.0, 0.5, sentinels=False)
    x = x.half()
    mod = (0.5 * torch.randn(ADA_B, (9 if c.two else 6) * C, generator=g)).half()
    ch = lambda k: mod[:, k * C:(k + 1) * C]
    b = SimpleNamespace(case=c, x=x, mod=mod, scale=ch(1), shift=ch(0), path=adaln_path(rows, ADA_N, C, c.two),
                        sentinels=sentinel_chunks(C // 8) if c.values == "normal" else [])
    b.ref = rr.adaln_ref(x, b.scale, b.shift, ADA_N, ADALN_EPS)
    if c.two:
        b.scale2, b.shift2 = ch(7), ch(6)
        b.ref2 = rr.adaln_ref(x, b.scale2, b.shift2, ADA_N, ADALN_EPS)
    return b


def ada_bound(b, ref=None):
    return rowln_bound(b.x, b.ref if ref is None else ref, b.path["adds_per_lane"])


# ------------------------------------------------------------------------------------------------ rmsnorm_heads
RmsCase = namedtuple("RmsCase", "name d heads rows pad ptr_off family")      # ld = heads * d + pad; the base pointer is ptr_off halfs in
RMS_VEC = [RmsCase(f"vec_d{d}_h{h}_r{r}_pad{p}", d, h, r, p, 0, "vec") for d in (32, 64, 128) for h in (1, 3, 24) for r in (1, 5, 11) for p in (0, 8)]
RMS_SCALAR = [RmsCase(f"scalar_d{d}_h{h}_r{r}", d, h, r, 0, 0, "scalar") for d in (2, 40, 72, 96, 192, 256) for h in (1, 3) for r in (1, 5, 9)]
RMS_FORCED = [RmsCase("scalar_d64_ld_plus_2", 64, 3, 5, 2, 0, "scalar"), RmsCase("scalar_d64_pointer_plus_2", 64, 3, 5, 0, 2, "scalar")]
RMS_CASES = {c.name: c for c in RMS_VEC + RMS_SCALAR + RMS_FORCED}
PairCase = namedtuple("PairCase", "name d heads rows pad family")              # a fused [rows, 3C + pad] buffer, c0 = 0, c1 = C
PAIR_CASES = {c.name: c for c in
              [PairCase(f"pair_vec_d{d}_h{h}_r{r}_pad{p}", d, h, r, p, "vec") for d in (64, 128) for h in (2, 24) for r in (1, 7) for p in (0, 8)]
              + [PairCase(f"pair_scalar_d40_h8_r{r}_pad{p}", 40, 8, r, p, "scalar") for r in (1, 7) for p in (0, 8)]}


def rms_path(rows, heads, d, ld, c0=0, c1=None, ptr_off=0):
    """launch_rms_pair: the vec eligibility test, then the grid of the kernel it launches"""
    two = c1 is not None
    vec = d in (32, 64, 128) and ld % 8 == 0 and c0 % 8 == 0 and (not two or c1 % 8 == 0) and (2 * ptr_off) % 16 == 0      # x | w0 | w1 & 15
    if vec:
        n = rows * heads * (d // 8) * (2 if two else 1)                 # one thread per 16-byte piece
        return dict(kernel="vec", LPH=d // 8, launches=1, blocks=(n + 255) // 256, ragged=n % 256 != 0, adds_per_lane=8)
    units = rows * heads                                                # one wave per (row, head), 4 per block
    return dict(kernel="scalar", LPH=0, launches=2 if two else 1, blocks=(units + 3) // 4, ragged=units % 4 != 0, slots=(d + 63) // 64,
                lanes_last=d - 64 * ((d - 1) // 64), adds_per_lane=4)


def rms_expect(c):
    """what the case's family says: the vec kernel with LPH = d / 8 in one launch, or the scalar kernel (two launches for a pair)"""
    if c.family == "vec":
        return dict(kernel="vec", LPH=c.d // 8, launches=1)
    return dict(kernel="scalar", LPH=0, launches=2 if isinstance(c, PairCase) else 1)


def rms_sentinels(d, vec):
    if vec:
        return [d - 8, d - 1]                                           # elements 0 and 7 of the head's last chunk (lane LPH - 1)
    return sorted({e for e in (63, 64, 127, 128, 191, 192, d - 1) if 0 <= e < d})


def _heads_data(g, rows, heads, d, vec):
    s = 0.5 * (1.0 + (7 * torch.arange(rows)[:, None] + torch.arange(heads)[None]) % 5).float()[..., None]      # neighbours differ by 1.2x at least
    s[-1] *= 4.0
    x = s * torch.randn(rows, heads, d, generator=g)
    for e in rms_sentinels(d, vec):
        x[..., e] += SENTINEL * s[..., 0]
    return x.half()


@lru_cache(maxsize=None)
def build_rms(name):
    c = RMS_CASES[name]
    g = torch.Generator().manual_seed(_seed(RMS_CASES, name))
    path = rms_path(c.rows, c.heads, c.d, c.heads * c.d + c.pad, ptr_off=c.ptr_off)
    x = _heads_data(g, c.rows, c.heads, c.d, path["kernel"] == "vec")
    w = (1.0 + 0.2 * torch.randn(c.d, generator=g)).half()
    return SimpleNamespace(case=c, x=x, w=w, path=path, ref=rr.rms_ref(x, w, RMS_EPS), sentinels=rms_sentinels(c.d, path["kernel"] == "vec"))


def pair_scale0(d):
    """log2(e) / sqrt(d) as the float32 the entry is given"""
    return float(torch.tensor(math.log2(math.e) / math.sqrt(d), dtype=torch.float32))


@lru_cache(maxsize=None)
def build_pair(name):
    c = PAIR_CASES[name]
    g = torch.Generator().manual_seed(_seed(PAIR_CASES, name))
    C = c.heads * c.d
    path = rms_path(c.rows, c.heads, c.d, 3 * C + c.pad, 0, C)
    vec = path["kernel"] == "vec"
    qkv = torch.cat([_heads_data(g, c.rows, c.heads, c.d, vec).reshape(c.rows, C) for _ in range(3)], dim=1)
    w0 = (1.0 + 0.2 * torch.randn(c.d, generator=g)).half()
    w1 = (0.7 + 0.2 * torch.randn(c.d, generator=g)).half()
    return SimpleNamespace(case=c, qkv=qkv, w0=w0, w1=w1, C=C, scale0=pair_scale0(c.d), path=path,
                           ref=rr.rms_pair_ref(qkv, c.heads, c.d, 0, w0, C, w1, RMS_EPS, pair_scale0(c.d)))


def rms_bound(ref_out, adds_per_lane):
    """|ref| K u + 2^-11 |ref| + 2^-25,  K = 8 + adds_per_lane + 6"""
    return ref_out.abs() * (8 + adds_per_lane + 6) * U + _store(ref_out)


# ------------------------------------------------------------------------------------------------ elementwise
def flat_path(n_threads, block=256):
    """one thread per 16-byte piece (gate_residual, activation), per (b, j) (timestep_embedding) or per element (patch_kernel)"""
    return dict(threads=n_threads, blocks=(n_threads + block - 1) // block, ragged=n_threads % block != 0)


GATE_C = (8, 64, 1536)
GATE_EXPECT = {8: dict(threads=15, blocks=1, ragged=True), 64: dict(threads=120, blocks=1, ragged=True), 1536: dict(threads=2880, blocks=12, ragged=True)}


@lru_cache(maxsize=None)
def build_gate(C):
    g = torch.Generator().manual_seed(3500 + C)
    rows = ADA_B * ADA_N
    x, _ = _rows_data(g, rows, C, sentinels=False)
    y, _ = _rows_data(g, rows, C, sentinels=False)
    mod = (0.5 * torch.randn(ADA_B, 6 * C, generator=g)).half()
    x, y, gate = x.half(), y.half(), mod[:, 2 * C:3 * C]
    return SimpleNamespace(C=C, x=x, y=y, mod=mod, gate=gate, path=flat_path(rows * (C // 8)), ref=rr.gate_residual_ref(x, gate, y, ADA_N))


def gate_bound(ref):
    """one fmaf: the store plus one float32 rounding"""
    return _store(ref) + ref.abs() * U


def all_finite_fp16():
    """the 63 488 finite fp16 values, -0 and the subnormals included"""
    v = torch.arange(0, 65536, dtype=torch.int32).to(torch.int16).view(torch.float16)
    v = v[torch.isfinite(v)]
    assert v.numel() == 63488
    return v


ACT_SILU, ACT_GELU_TANH = 0, 1
ACT_INPUTS = ("all_finite", "n8")


@lru_cache(maxsize=None)
def build_act(which):
    x = all_finite_fp16() if which == "all_finite" else torch.tensor([-5.16, -0.75, -0.0, 0.0, 6.1e-5, 1.0, 3.3, 11.0]).half()
    return SimpleNamespace(x=x, path=flat_path(x.numel() // 8), ref={ACT_SILU: rr.silu_ref(x), ACT_GELU_TANH: rr.gelu_tanh_ref(x)})


ACT_EXPECT = {"all_finite": dict(threads=7936, blocks=31, ragged=False), "n8": dict(threads=1, blocks=1, ragged=True)}


def act_bound(x, ref, act):
    """SiLU: 2^-11 |ref| + 2^-25 + |ref| 8 u;  GELU(tanh): the same + 0.5 |x| 4 u  (1 + tanhf(u) cancels to about one float32 ulp)"""
    bnd = _store(ref) + ref.abs() * 8 * U
    return bnd + 0.5 * x.double().abs() * 4 * U if act == ACT_GELU_TANH else bnd


TS_VALUES = (0.0, 0.5, 1.0, 437.0, 981.25, 999.0, 1000.0)
TsCase = namedtuple("TsCase", "name B dim shift flip t")
TS_CASES = {}
for _i, (_dim, _shift) in enumerate(((2, 0.0), (6, 0.0), (256, 0.0), (320, 0.0), (320, 1.0))):
    for _flip in (0, 1):
        _k = 2 * _i + _flip
        _t1 = (TS_VALUES[(3 + _k) % 7],)                                           # B = 1: 437, 981.25, 999, 1000, 0, 0.5, 1, 437, ..
        _t5 = tuple(TS_VALUES[(_k + s) % 7] for s in range(5))                      # B = 5: five consecutive values of the list
        for _t in (_t1, _t5):
            _n = f"t_b{len(_t)}_dim{_dim}_shift{int(_shift)}_flip{_flip}"
            TS_CASES[_n] = TsCase(_n, len(_t), _dim, _shift, _flip, _t)


@lru_cache(maxsize=None)
def build_ts(name):
    c = TS_CASES[name]
    t = torch.tensor(c.t, dtype=torch.float32)
    ref, a, ex = rr.timestep_embedding_ref(t, c.dim, c.flip, c.shift)
    return SimpleNamespace(case=c, t=t, ref=ref, a=a, ex=ex, path=flat_path(c.B * (c.dim // 2), 128))


def ts_bound(b):
    """2^-11 |ref| + 2^-25 + a (ex + 4) 2^-23 + 2^-22,  a = t freq, ex = ln(P) j / (half - shift): the rounding of the argument moves sin / cos by
    as much as it moves a"""
    arg = b.a * (b.ex[None] + 4.0) * 2.0 ** -23 + 2.0 ** -22
    return _store(b.ref) + torch.cat([arg, arg], dim=1)


PATCH_SHAPE = (3, 16, 8, 12)                           # B, C, H, W
PATCHES = (1, 2, 4)


@lru_cache(maxsize=None)
def build_patch(p):
    B, C, H, W = PATCH_SHAPE
    g = torch.Generator().manual_seed(3600 + p)
    lat = torch.randn(B, C, H, W, generator=g).half()
    rows = torch.randn(B * (H // p) * (W // p), p * p * C, generator=g).half()
    return SimpleNamespace(p=p, lat=lat, rows=rows, path=flat_path(B * C * H * W), want_rows=rr.patchify_ref(lat, p), want_lat=rr.unpatchify_ref(rows, B, C, H, W, p))
