"""GPU: the upsampler conv (3x3 over the nearest x2 upsampled input) as four 2x2-tap phase convs inside conv_patch_kernel
(univst_conv_up2_phase_weights / univst_conv3x3_up2_phase; GemmParams::W4).

Output pixel (2y+a, 2x+b) reads source rows {y-1, y} (a = 0) / {y, y+1} (a = 1), columns alike, so phase (a, b) is a 2x2-tap conv over the SOURCE
image whose weights are sums of the original taps: per axis {k0}, {k1+k2} for phase 0 and {k0+k1}, {k2} for phase 1.

Bound of the operator test (every element, none exempt).  The reference is the fp64 conv of the same fp16 inputs with the UNROUNDED weight sums;
A is the fp64 conv of |x| with |summed weights| (+ |bias|).  The kernel rounds each summed weight to fp16 once (relative error <= 2^-11 each, so
<= 2^-11 A in the result), accumulates 4 Cin products and the bias in fp32 (<= (4 Cin + 2) 2^-24 A) and rounds the result to fp16 once
(<= 2^-11 |y|):    |got - y64| <= 2^-11 |y64| + (2^-11 + (4 Cin + 2) 2^-24) A.
A swapped tap or phase is off by about 60x this bound at these K.  Worst error / bound ratio measured on MI355X: see DESIGN.md §4."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (imgs, Cin, Cout, Hs, Ws): 49 152 output rows each — the smallest size at which the LDS-patch kernel is chosen (>= 150 tiles)
CASES = [(48, 64, 320, 16, 16),     # 192-row tiles straddling images; the smallest legal patch ring (2 slabs)
         (48, 192, 640, 16, 16),    # 6 slabs: the patch ring wraps; two column tiles
         (12, 64, 320, 32, 32),     # tiles inside an image, halo rows from the neighbouring tiles
         (192, 64, 320, 8, 8),      # two image rows per 16-pixel fragment, three images per tile
         (96, 64, 320, 8, 16)]      # non-square source
ROWS = {0: ([0], [1, 2]), 1: ([0, 1], [2])}      # original taps of one axis on the two source pixels of phase 0 / 1


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def phase_sums(w64):
    """[Co, Ci, 3, 3] fp64 -> {(a, b): [Co, Ci, 2, 2]} unrounded"""
    out = {}
    for a in (0, 1):
        for b in (0, 1):
            s = torch.zeros(w64.shape[0], w64.shape[1], 2, 2, dtype=torch.float64)
            for i in (0, 1):
                for j in (0, 1):
                    s[:, :, i, j] = w64[:, :, ROWS[a][i], :][:, :, :, ROWS[b][j]].sum((2, 3))
            out[(a, b)] = s
    return out


def phase_conv64(x64, sums, bias64):
    """the four 2x2-tap convs over the zero-padded source, interleaved into [imgs, Co, 2Hs, 2Ws] (fp64, CPU)"""
    imgs, _, Hs, Ws = x64.shape
    Co = sums[(0, 0)].shape[0]
    y = torch.empty(imgs, Co, 2 * Hs, 2 * Ws, dtype=torch.float64)
    xp = F.pad(x64, (1, 1, 1, 1))
    for (a, b), s in sums.items():
        full = F.conv2d(xp, s, bias64)                  # [.., Hs + 1, Ws + 1]: element (y + a, x + b) reads source rows y - 1 + a .. y + a
        y[:, :, a::2, b::2] = full[:, :, a:a + Hs, b:b + Ws]
    return y


@pytest.fixture(scope="module")
def cases(nat):
    """inputs, the operator's result with its statistics and the fp64 reference with its bound, computed once per case"""
    made = {}

    def get(case):
        if case not in made:
            imgs, Ci, Co, Hs, Ws = case
            g = torch.Generator().manual_seed(17 + Ci + Hs)
            x = torch.randn(imgs, Ci, Hs, Ws, generator=g).half()
            w = (torch.randn(Co, Ci, 3, 3, generator=g) / (9 * Ci) ** 0.5).half()
            b = torch.randn(Co, generator=g).half()
            w4 = nat.conv_up2_phase_weights(w.cuda())
            got, gst = nat.conv3x3_up2_phase(nhwc(x.cuda()), w4, bias=b.cuda(), gn_group_width=10)
            torch.cuda.synchronize()
            sums = phase_sums(w.double())
            y64 = phase_conv64(x.double(), sums, b.double())
            A = phase_conv64(x.double().abs(), {k: v.abs() for k, v in sums.items()}, b.double().abs())
            bound = 2.0 ** -11 * y64.abs() + (2.0 ** -11 + (4 * Ci + 2) * 2.0 ** -24) * A
            made[case] = dict(x=x, w=w, b=b, w4=w4.cpu(), got=got.cpu(), gst=gst.cpu(), y64=nhwc(y64), bound=nhwc(bound))
        return made[case]
    return get


@pytest.mark.parametrize("case", CASES)
def test_phase_weights_are_the_rounded_tap_sums(cases, case):
    """[4][Co][Ci/32][4][32]: fp32 sums of fp16 taps, one fp16 rounding (the fp64 sum rounds the same way: <= 4 addends of 11-bit significands)"""
    c = cases(case)
    Co, Ci = c["w"].shape[:2]
    sums = phase_sums(c["w"].double())
    for (a, b), s in sums.items():
        want = s.reshape(Co, Ci // 32, 32, 4).permute(0, 1, 3, 2).float().half()
        assert torch.equal(c["w4"][2 * a + b], want), (a, b)


@pytest.mark.parametrize("case", CASES)
def test_phase_conv_within_the_fp64_rounding_bound(cases, case):
    c = cases(case)
    err = (c["got"].double() - c["y64"]).abs()
    ratio = (err / c["bound"]).max().item()
    print(f"conv phase {case}: worst error / bound = {ratio:.3f}, max err {err.max().item():.3e}, max |ref| {c['y64'].abs().max().item():.3e}")
    bad = err > c["bound"]
    assert not bad.any(), f"{int(bad.sum())} elements over the bound, worst ratio {ratio:.3f}"


@pytest.mark.parametrize("case", CASES)
def test_phase_conv_statistics_are_those_of_the_stored_rows(cases, case):
    """gn_out[sub-group][slot][2] with slot 4 s + phase: over every range of whole images the slots' sums equal the sum and sum of squares of the
    stored fp16 rows (fp32 summation error: 16 rows x 10 channels per slot in fp32, then fp64 here)"""
    c = cases(case)
    imgs, Ci, Co, Hs, Ws = case
    got = c["got"].double().reshape(imgs, 4 * Hs * Ws, Co // 10, 10)
    s1 = got.sum((1, 3))                                             # [imgs, Co / 10]
    s2 = (got * got).sum((1, 3))
    a2 = (got * got).sum((1, 3))
    a1 = got.abs().sum((1, 3))
    slots = c["gst"].double().reshape(Co // 10, imgs, 4 * Hs * Ws // 16, 2).sum(2)      # an image's slots are one contiguous range
    tol = 160 * 2.0 ** -24
    assert ((slots[..., 0].T - s1).abs() <= tol * a1 + 1e-30).all()
    assert ((slots[..., 1].T - s2).abs() <= tol * a2 + 1e-30).all()
    # and every slot is one 16-row fragment of ONE phase: slot 4 s + ph holds source pixels 16 s .. 16 s + 15 of phase ph
    rows = c["got"].double().reshape(imgs, Hs, 2, Ws, 2, Co)         # [img, y, a, x, b, c]
    for ph in range(4):
        frag = rows[:, :, ph >> 1, :, ph & 1, :].reshape(imgs * Hs * Ws // 16, 16, Co // 10, 10)
        want = frag.sum((1, 3)).T                                    # [Co / 10, source fragments]
        have = c["gst"][:, ph::4, 0].double()
        assert ((have - want).abs() <= tol * frag.abs().sum((1, 3)).T + 1e-30).all(), ph


@pytest.mark.parametrize("case", [CASES[0], CASES[2]])
def test_phase_conv_exact_on_small_integers(nat, case):
    """x in {-2 .. 2}, w in {-1, 0, 1}, integer bias: |y| <= 1 152 and every sum (weights, products, result) is exact in fp16 / fp32, so the phase form
    must equal the conv over the upsampled image bit for bit"""
    imgs, Ci, Co, Hs, Ws = case
    g = torch.Generator().manual_seed(5)
    x = torch.randint(-2, 3, (imgs, Ci, Hs, Ws), generator=g).half()
    w = torch.randint(-1, 2, (Co, Ci, 3, 3), generator=g).half()
    b = torch.randint(-4, 5, (Co,), generator=g).half()
    ref = F.conv2d(F.interpolate(x.double(), scale_factor=2.0, mode="nearest"), w.double(), b.double(), padding=1)
    assert ref.abs().max().item() <= 1152 + 4
    got = nat.conv3x3_up2_phase(nhwc(x.cuda()), nat.conv_up2_phase_weights(w.cuda()), bias=b.cuda())
    assert torch.equal(got.cpu(), nhwc(ref).half())


def test_phase_conv_refuses_ineligible_problems(nat):
    """too few tiles for the LDS-patch kernel, and a source width that does not divide the tile: an error, never another path"""
    for imgs, Hs, Ws in [(6, 16, 16), (48, 16, 24)]:
        x = torch.zeros(imgs, Hs, Ws, 64, dtype=torch.float16, device="cuda")
        w4 = torch.zeros(4, 320, 2, 4, 32, dtype=torch.float16, device="cuda")
        with pytest.raises(RuntimeError, match="not eligible"):
            nat.conv3x3_up2_phase(x, w4)
