"""The MX-fp8 quantisation rule of include/univst.h (univst_mxfp8_quantize), restated in float64 with no fp8 dtype of torch involved.

Format: OCP MX, e4m3fn elements, blocks of 32 consecutive elements along K, one E8M0 scale byte per block.
  block scale  e = floor(log2(amax)) - 8, and e += 1 when amax * 2^-e > 448; amax == 0 -> e = 0; scale byte = e + 127
  elements     x * 2^-e (exact) rounded to e4m3 to nearest even; the clamp to +-448 is a guard that the scale rule never lets fire
"""
import torch

BLOCK = 32
E4M3_MAX = 448.0


def e4m3_decode_table():
    """float64 [256]: the value of every e4m3fn byte (0x7f / 0xff are NaN)"""
    out = torch.empty(256, dtype=torch.float64)
    for b in range(256):
        sign = -1.0 if b & 0x80 else 1.0
        ex, man = (b >> 3) & 0xF, b & 7
        if ex == 0xF and man == 7:
            v = float("nan")
        elif ex == 0:
            v = man * 2.0 ** -9
        else:
            v = (8 + man) * 2.0 ** (ex - 7 - 3)
        out[b] = sign * v
    return out


def e4m3_encode(v):
    """float64 tensor, |v| <= 448 -> uint8 e4m3fn bytes, round to nearest even (torch.round is half-to-even; every quotient below is exact)"""
    v = v.to(torch.float64)
    a = v.abs().clamp(max=E4M3_MAX)
    ex = torch.floor(torch.log2(a.clamp(min=2.0 ** -20))).clamp(min=-6.0)            # subnormals share the exponent of the smallest normal
    # log2 of a float64 just below a power of two can round up to it: fix the exponent with exact comparisons
    ex = torch.where(torch.pow(2.0, ex) > a, ex - 1, ex).clamp(min=-6.0)
    ex = torch.where(torch.pow(2.0, ex + 1) <= a, ex + 1, ex)
    m = torch.round(a / torch.pow(2.0, ex - 3))                                      # 0..16 in units of the exponent's step
    up = m >= 16
    ex = torch.where(up, ex + 1, ex)
    m = torch.where(up, torch.full_like(m, 8.0), m)
    normal = m >= 8
    code = torch.where(normal, (ex + 7) * 8 + (m - 8), m).to(torch.int64)            # subnormal: exponent field 0, m = 0..7
    code = code | (torch.signbit(v).to(torch.int64) << 7)
    return code.to(torch.uint8)


def block_exponent(amax):
    """float64 tensor of block maxima -> int64 e of the rule above"""
    amax = amax.to(torch.float64)
    safe = torch.where(amax > 0, amax, torch.ones_like(amax))
    fl = torch.floor(torch.log2(safe))
    fl = torch.where(torch.pow(2.0, fl) > safe, fl - 1, fl)
    fl = torch.where(torch.pow(2.0, fl + 1) <= safe, fl + 1, fl)
    e = fl - 8
    e = torch.where(safe * torch.pow(2.0, -e) > E4M3_MAX, e + 1, e)
    return torch.where(amax > 0, e, torch.zeros_like(e)).to(torch.int64)


def quantize(x):
    """x fp16 [rows, K] (K % 32 == 0) -> (e4m3fn bytes uint8 [rows, K], E8M0 bytes uint8 [rows, K/32])"""
    assert x.dtype == torch.float16 and x.dim() == 2 and x.shape[1] % BLOCK == 0
    rows, K = x.shape
    xb = x.to(torch.float64).reshape(rows, K // BLOCK, BLOCK)
    e = block_exponent(xb.abs().amax(dim=2))
    scaled = xb * torch.pow(2.0, -e.to(torch.float64)).unsqueeze(2)
    q = e4m3_encode(scaled).reshape(rows, K)
    return q, (e + 127).to(torch.uint8)


def dequantize(q, s):
    """-> float64 [rows, K]"""
    rows, K = q.shape
    v = e4m3_decode_table()[q.long()].reshape(rows, K // BLOCK, BLOCK)
    return (v * torch.pow(2.0, s.to(torch.float64) - 127).unsqueeze(2)).reshape(rows, K)


def fake_quantize(x):
    """fp16 -> the dequantised values, which are exactly representable in fp16 (asserted)"""
    d = dequantize(*quantize(x))
    h = d.to(torch.float16)
    assert torch.equal(h.to(torch.float64), d)
    return h
