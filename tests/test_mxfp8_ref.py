"""CPU: tests/mxfp8_ref.py, the float64 restatement of the MX-fp8 quantisation rule (include/univst.h univst_mxfp8_quantize), against torch's own
float8_e4m3fn cast and against the rule's edge cases.  The GPU tests compare the kernels with this restatement byte for byte."""
import pytest
import torch

import mxfp8_ref as R


def _draw(rows, K, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(rows, K, generator=g) * scale).to(torch.float16)


def test_decode_table_and_encode_agree_with_torch_e4m3fn():
    tab = R.e4m3_decode_table()
    ok = ~torch.isnan(tab)
    assert int(ok.sum()) == 254 and float(tab[ok].abs().max()) == 448.0
    tt = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64)
    assert torch.equal(tab[ok], tt[ok])
    # every byte round-trips; midpoints between neighbours go to the even one, as torch's cast does
    assert torch.equal(R.e4m3_encode(tab[ok]), torch.arange(256, dtype=torch.uint8)[ok])
    pos = torch.sort(tab[:0x7f]).values
    mid = (pos[:-1] + pos[1:]) / 2
    v = torch.cat([mid, -mid, mid * (1 + 2.0 ** -20), mid * (1 - 2.0 ** -20)])
    assert torch.equal(R.e4m3_encode(v), v.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8))
    g = torch.Generator().manual_seed(0)
    v = (torch.rand(20000, generator=g, dtype=torch.float64) * 2 - 1) * 448
    v = torch.cat([v, v * 2.0 ** -8, v * 2.0 ** -14]).to(torch.float32).to(torch.float64)
    assert torch.equal(R.e4m3_encode(v), v.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_quantize_equals_torch_cast_of_the_scaled_values_and_never_saturates(scale):
    x = _draw(256, 1536, scale, 1)
    q, s = R.quantize(x)
    e = s.to(torch.float64) - 127
    scaled = (x.to(torch.float64).reshape(256, -1, 32) * torch.pow(2.0, -e).unsqueeze(2)).reshape(256, 1536)
    assert float(scaled.abs().max()) <= 448.0, "an element saturates"
    assert torch.equal(q, scaled.to(torch.float32).to(torch.float8_e4m3fn).view(torch.uint8))
    # every block uses the top binade pair of e4m3: its maximum lands in (224, 448]
    top = scaled.abs().reshape(256, -1, 32).amax(dim=2)
    assert float(top.min()) > 224.0
    d = R.dequantize(q, s)
    assert torch.equal(d.to(torch.float16).to(torch.float64), d), "a dequantised value is not an fp16 value"
    assert torch.equal(R.fake_quantize(x).to(torch.float64), d)


def test_plain_ocp_rule_would_saturate_where_this_one_does_not():
    """the +1 step is what the rule adds to OCP's floor(log2(amax)) - 8: without it block maxima in (448, 512) * 2^e clamp"""
    x = _draw(256, 1536, 1.0, 2)
    amax = x.to(torch.float64).abs().reshape(256, -1, 32).amax(dim=2)
    plain = torch.floor(torch.log2(amax)) - 8
    frac_blocks = float((amax * torch.pow(2.0, -plain) > 448).double().mean())
    assert 0.0 < frac_blocks < 0.5
    e = R.block_exponent(amax).to(torch.float64)
    assert bool((amax * torch.pow(2.0, -e) <= 448).all())


@pytest.mark.parametrize("e", [-20, -3, 0, 5])
def test_scale_byte_at_block_maxima_around_448(e):
    """amax = 448 * 2^e is the last maximum that keeps floor(log2) - 8; the next fp16 value above it takes the +1 step"""
    at = 448.0 * 2.0 ** e                    # floor(log2) = e + 8; the fp16 values around it are 0.25 * 2^e apart
    x = torch.zeros(3, 32, dtype=torch.float64)
    x[0, 3] = at
    x[1, 5] = -(at + 2.0 ** e)              # 449 * 2^e
    x[2, 7] = at + 0.25 * 2.0 ** e          # the next fp16 value above 448 * 2^e
    assert torch.equal(x.to(torch.float16).to(torch.float64), x)
    x = x.to(torch.float16)
    q, s = R.quantize(x)
    assert s[:, 0].tolist() == [e + 127, e + 128, e + 128]
    assert q[0, 3] == 0x7E and q[1, 5] == (0x80 | 0x76) and q[2, 7] == 0x76      # 448; 224.5 and 224.125 round to 224 = 1.75 * 2^7
    # a power-of-two maximum sits at 256 after scaling
    p = torch.zeros(1, 32, dtype=torch.float16)
    p[0, 0] = 2.0 ** (e + 8)
    q, s = R.quantize(p)
    assert int(s[0, 0]) == e + 127 and int(q[0, 0]) == 0x78 and float(R.dequantize(q, s)[0, 0]) == 2.0 ** (e + 8)


def test_zero_block_and_fp16_subnormal_blocks():
    x = torch.zeros(2, 96, dtype=torch.float16)
    x[0, 40] = 1.5                                # blocks 0 and 2 of row 0 are all zero
    x[1, :32] = torch.arange(32, dtype=torch.float64).mul(2.0 ** -24).to(torch.float16)       # subnormals 0 .. 31 * 2^-24
    x[1, 64] = 2.0 ** -24                         # the smallest fp16 value alone
    x[1, 65] = -0.0
    q, s = R.quantize(x)
    assert s[0].tolist() == [127, 127 - 8, 127] and int(q[0].count_nonzero()) == 1 and int(q[0, 40]) == 0x7C      # 1.5 * 2^8 = 384
    assert s[1].tolist() == [127 - 27, 127, 127 - 32]          # 31 * 2^-24 * 2^28 = 496 > 448: the +1 step; 2^-24 * 2^32 = 256
    assert int(q[1, 64]) == 0x78 and int(q[1, 65]) == 0x80
    d = R.dequantize(q, s)
    # 31 * 2^-24 scales to 248: 0 .. 31 become 0, 8, .. 248, all e4m3 values up to 128, then every second one (ties to even above)
    want = torch.tensor([R.e4m3_decode_table()[int(b)] for b in R.e4m3_encode(torch.arange(32, dtype=torch.float64) * 8)]) * 2.0 ** -27
    assert torch.equal(d[1, :32], want) and torch.equal(d[1, :17], x[1, :17].to(torch.float64))
    assert torch.equal(d.to(torch.float16).to(torch.float64), d)


def test_product_error_of_the_format_is_a_few_percent():
    """activations N(0,1) [256, 1536] x weights N(0, 1/K) [512, 1536]: the relative rms error of the MX product is the format's, about 3.7 %"""
    x, w = _draw(256, 1536, 1.0, 3), _draw(512, 1536, 1536 ** -0.5, 4)
    exact = x.to(torch.float64) @ w.to(torch.float64).T
    mx = R.dequantize(*R.quantize(x)) @ R.dequantize(*R.quantize(w)).T
    rel = float((mx - exact).pow(2).mean().sqrt() / exact.pow(2).mean().sqrt())
    print(f"relative rms error of the MX-fp8 product: {rel:.4f}")
    assert 0.02 < rel < 0.06
