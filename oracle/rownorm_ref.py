"""Float64 references, on the fp16 inputs, of the row-wise normalisations and the MM-DiT elementwise operators (csrc/norm.hip:
layernorm_kernel; csrc/sd3.hip: adaln_modulate_kernel, rms_heads_kernel, rms_heads_vec_kernel, gate_residual_kernel, act_kernel,
timestep_embed_kernel, patch_kernel), and next to each a float32 emulation in the kernel's own order of operations: per-lane sums over the
slots i and the 8 elements e of a 16-byte chunk, the xor butterfly over 64 (or LPH) lanes, then the expression of the store line.

The references take optional weights on the terms of the statistics (1: as is, 0: left out of the sum, 2: counted twice) so that
tests/test_rownorm_cases.py can show what a dropped or doubled chunk does to the result.  The emulations use plain float32 torch
arithmetic (no fused multiply-add where the compiler may contract one: the bounds hold for either)."""
import math
from types import SimpleNamespace

import torch

F32 = torch.float32
_LANE = torch.arange(64)


def _f(v):
    return torch.tensor(float(v), dtype=F32)


def _h(x):
    """the store: one rounding to fp16, returned as float64"""
    return x.half().double()


# ------------------------------------------------------------------------------------------------ LayerNorm / adaLN
def rowln_ref(x, g, b, eps, col_weight=None):
    """x fp16 [rows, C]; g, b float64 [rows or 1, C]  ->  out = (x - mean) r g + b with mean, var over the row (biased), r = 1 / sqrt(var + eps).
    col_weight [C] or [rows, C]: the weight of each element in the two sums (the divisor stays C)."""
    xd = x.double()
    C = xd.shape[1]
    w = torch.ones_like(xd) if col_weight is None else col_weight.double().expand_as(xd)
    mean = (w * xd).sum(dim=1, keepdim=True) / C
    var = (w * (xd - mean) ** 2).sum(dim=1, keepdim=True) / C
    r = 1.0 / torch.sqrt(var + eps)
    return SimpleNamespace(out=(xd - mean) * r * g + b, mean=mean, var=var, r=r, g=g.expand_as(xd), b=b.expand_as(xd))


def layernorm_ref(x, gamma, beta, eps, col_weight=None):
    return rowln_ref(x, gamma.double()[None], beta.double()[None], eps, col_weight)


def batch_of_row(rows, rows_per_batch, shift_rows=0):
    """b = r / rows_per_batch; shift_rows = +1 / -1: every row takes the batch of its neighbour (a defect, clamped to the valid range)"""
    r = (torch.arange(rows) + shift_rows).clamp(0, rows - 1)
    return r // rows_per_batch


def adaln_ref(x, scale, shift, rows_per_batch, eps, col_weight=None, shift_rows=0):
    """x fp16 [rows, C], scale / shift fp16 [B, C] (views allowed) -> LayerNorm(x; no affine) (1 + scale[b]) + shift[b]"""
    bi = batch_of_row(x.shape[0], rows_per_batch, shift_rows)
    return rowln_ref(x, 1.0 + scale.double()[bi], shift.double()[bi], eps, col_weight)


def xor_sum(v, offsets):
    """v += shfl_xor(v, o) for o in offsets, on the last axis (64 lanes), float32"""
    for o in offsets:
        v = v + v[..., _LANE ^ o]
    return v


WAVE = (32, 16, 8, 4, 2, 1)                            # wave_sum of csrc/common.h


def _lane_layout(x, C):
    """[rows, C] float32 -> [rows, slots, 64, 8] (chunk ch = lane + 64 i, zero filled) and the mask of live (slot, lane)"""
    rows = x.shape[0]
    nch8 = C // 8
    slots = (nch8 + 63) // 64
    xp = torch.zeros(rows, slots * 512, dtype=F32)
    xp[:, :C] = x
    return xp.reshape(rows, slots, 64, 8), (torch.arange(slots * 64).reshape(slots, 64) < nch8), slots


def emu_rowln(x, g, b, eps):
    """layernorm_kernel / adaln_modulate_kernel in float32 on x fp16 [rows, C], g, b float32 [rows or 1, C] -> float64 (the fp16 result)"""
    rows, C = x.shape
    xf = x.float()
    xp, ok, slots = _lane_layout(xf, C)
    s = torch.zeros(rows, 64, dtype=F32)
    for i in range(slots):
        for e in range(8):
            s = s + xp[:, i, :, e]                                       # idle lanes add 0.f: the same value
    mean = (xor_sum(s, WAVE) / _f(C))[:, :1]
    q = torch.zeros(rows, 64, dtype=F32)
    for i in range(slots):
        for e in range(8):
            d = (xp[:, i, :, e] - mean) * ok[i][None]
            q = q + d * d
    rstd = 1.0 / torch.sqrt(xor_sum(q, WAVE)[:, :1] / _f(C) + _f(eps))
    return _h((xf - mean) * rstd * g + b)


def emu_layernorm(x, gamma, beta, eps):
    return emu_rowln(x, gamma.float()[None], beta.float()[None], eps)


def emu_adaln(x, scale, shift, rows_per_batch, eps):
    bi = batch_of_row(x.shape[0], rows_per_batch)
    return emu_rowln(x, _f(1.0) + scale.float()[bi], shift.float()[bi], eps)


# ------------------------------------------------------------------------------------------------ per-head RMSNorm
def rms_ref(x, w, eps, scale=1.0, elem_weight=None):
    """x fp16 [rows, heads, d], w fp16 [d] -> x / sqrt(mean_e x^2 + eps) w scale (float64).  elem_weight [d] or [rows, heads, d] weighs the
    squares in the sum (the divisor stays d)."""
    xd = x.double()
    ew = torch.ones_like(xd) if elem_weight is None else elem_weight.double().expand_as(xd)
    r = 1.0 / torch.sqrt((ew * xd * xd).sum(dim=-1, keepdim=True) / xd.shape[-1] + eps)
    return SimpleNamespace(out=xd * r * w.double() * scale, r=r)


def rms_pair_ref(buf, heads, d, c0, w0, c1, w1, eps, scale0):
    """the q | k pass on a [rows, ld] buffer: block c0 with w0 and scale0, block c1 with w1; every other column as it is -> float64 [rows, ld]"""
    rows, C = buf.shape[0], heads * d
    out = buf.double().clone()
    out[:, c0:c0 + C] = rms_ref(buf[:, c0:c0 + C].reshape(rows, heads, d), w0, eps, scale0).out.reshape(rows, C)
    out[:, c1:c1 + C] = rms_ref(buf[:, c1:c1 + C].reshape(rows, heads, d), w1, eps).out.reshape(rows, C)
    return out


def emu_rms_vec(x, w, eps, scale=1.0):
    """rms_heads_vec_kernel<LPH = d / 8>: fmaf over the lane's 8 elements (a square of an fp16 value is exact in float32, so the fused and
    the plain form agree), xor butterfly o = 1 .. LPH / 2, r_ = rsqrt(ss / D + eps) * scl0, (float)v * r_ * (float)w"""
    rows, heads, d = x.shape
    lph = d // 8
    xf = x.float().reshape(rows, heads, lph, 8)
    ss = torch.zeros(rows, heads, lph, dtype=F32)
    for e in range(8):
        ss = ss + xf[..., e] * xf[..., e]
    o = 1
    idx = torch.arange(lph)
    while o < lph:
        ss = ss + ss[..., idx ^ o]
        o <<= 1
    r_ = (1.0 / torch.sqrt(ss[..., :1] / _f(d) + _f(eps))) * _f(scale)
    return _h((xf * r_[..., None] * w.float().reshape(lph, 8)).reshape(rows, heads, d))


def emu_rms_scalar(x, w, eps, scale=1.0):
    """rms_heads_kernel: lane l holds e = l + 64 i, i < 4 (0.f past d), ss += v * v, wave_sum, v * r_ * w * scl"""
    rows, heads, d = x.shape
    xp = torch.zeros(rows, heads, 256, dtype=F32)
    xp[..., :d] = x.float()
    xp = xp.reshape(rows, heads, 4, 64)
    ss = torch.zeros(rows, heads, 64, dtype=F32)
    for i in range(4):
        ss = ss + xp[:, :, i] * xp[:, :, i]
    r_ = 1.0 / torch.sqrt(xor_sum(ss, WAVE)[..., :1] / _f(d) + _f(eps))
    return _h(x.float() * r_ * w.float() * _f(scale))


# ------------------------------------------------------------------------------------------------ elementwise
def gate_residual_ref(x, gate, y, rows_per_batch, shift_rows=0):
    """x, y fp16 [rows, C], gate fp16 [B, C] -> x + gate[b] y"""
    bi = batch_of_row(x.shape[0], rows_per_batch, shift_rows)
    return x.double() + gate.double()[bi] * y.double()


def emu_gate_residual(x, gate, y, rows_per_batch):
    """fmaf(g, y, x): one rounding to float32 of the exact value (the product of two fp16 values is exact in float64), then the store"""
    return _h(gate_residual_ref(x, gate, y, rows_per_batch).float())


GELU_C = math.sqrt(2.0 / math.pi)


def silu_ref(x):
    xd = x.double()
    return xd / (1.0 + torch.exp(-xd))


def gelu_tanh_ref(x):
    xd = x.double()
    return 0.5 * xd * (1.0 + torch.tanh(GELU_C * (xd + 0.044715 * xd ** 3)))


def emu_silu(x):
    t = x.float()
    return _h(t / (_f(1.0) + torch.exp(-t)))


def emu_gelu_tanh(x):
    """u = 0.7978845608028654f * fmaf(0.044715f * t * t, t, t); 0.5f * t * (1.f + tanhf(u))"""
    t = x.float()
    k = _f(0.044715) * t * t
    inner = (k.double() * t.double() + t.double()).float()              # the fmaf: one rounding
    u = _f(0.7978845608028654) * inner
    return _h(_f(0.5) * t * (_f(1.0) + torch.tanh(u)))


def timestep_embedding_ref(t, dim, flip, shift, max_period=10000.0):
    """diffusers get_timestep_embedding (scale 1) on the float32 t, in float64 -> (out [B, dim], a = t freq [B, half], ex = ln(P) j / (half - shift))"""
    half = dim // 2
    ex = math.log(max_period) * torch.arange(half, dtype=torch.float64) / (half - shift)
    a = t.double()[:, None] * torch.exp(-ex)[None]
    sn, cs = torch.sin(a), torch.cos(a)
    return torch.cat([cs, sn] if flip else [sn, cs], dim=1), a, ex


def emu_timestep_embedding(t, dim, flip, shift, max_period=10000.0):
    """freq = expf(-logf(P) * (float)j / ((float)half - shift)); a = t * freq; sinf, cosf; the store"""
    half = dim // 2
    j = torch.arange(half, dtype=F32)
    freq = torch.exp(-torch.log(_f(max_period)) * j / (_f(half) - _f(shift)))
    a = t.float()[:, None] * freq[None]
    sn, cs = torch.sin(a), torch.cos(a)
    return _h(torch.cat([cs, sn] if flip else [sn, cs], dim=1))


def patchify_ref(lat, p):
    """[B, C, H, W] -> rows[(b, i, j)][(c p + u) p + v] = lat[b, c, i p + u, j p + v]"""
    B, C, H, W = lat.shape
    return lat.reshape(B, C, H // p, p, W // p, p).permute(0, 2, 4, 1, 3, 5).reshape(B * (H // p) * (W // p), C * p * p)


def unpatchify_ref(rows, B, C, H, W, p):
    """rows[(b, i, j)][(u p + v) C + c] -> lat[b, c, i p + u, j p + v]"""
    return rows.reshape(B, H // p, W // p, p, p, C).permute(0, 5, 1, 3, 2, 4).reshape(B, C, H, W)
