"""GPU parity of every stand-alone HIP operator, called through the C ABI (univst_amd._native), against
the oracle / a plain torch fp32 restatement of the same op on the same seeded inputs.

Tolerances (fp16 storage, fp32 accumulation): outputs are compared with the fp32 result computed from the SAME
fp16-rounded inputs; allowed error = 2 fp16 ulp of the output magnitude + accumulation noise, expressed as
|err| <= atol + rtol*|ref| with rtol = 2e-3 (2 ulp of fp16 = 2*2^-11 ~ 1e-3) unless stated otherwise.
Integer / index outputs (masks, warped uint8 frames) must be bit-exact.
"""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from oracle import unet_ref, maskprop_ref, flow_ref, synth_inputs as si  # noqa: E402


@pytest.fixture(scope="module")
def nat():
    from univst_amd import _native
    _native.load()
    assert torch.cuda.is_available(), "gpu tests need a GPU"
    return _native


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half().cuda()


def close(got, ref, rtol=2e-3, atol=None):
    got = got.float()
    ref = ref.float().to(got.device)
    if atol is None:
        atol = 2e-3 * ref.abs().max().item() + 1e-6
    err = (got - ref).abs()
    bad = err > (atol + rtol * ref.abs())
    assert not bad.any(), f"max err {err.max().item():.4e} (ref max {ref.abs().max().item():.3e}), {int(bad.sum())} bad"


def test_tr16_probe(nat):
    """ds_read_b64_tr_b16 semantics the attention kernel relies on: lane (g, l15), element j reads
    row g*4+j, column l15 of a row-major [16][16] fp16 image."""
    out = nat.debug_tr16().cpu().view(64, 4)
    for lane in range(64):
        g, l15 = lane >> 4, lane & 15
        for j in range(4):
            assert out[lane, j].item() == (g * 4 + j) * 16 + l15, (lane, j, out[lane].tolist())


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (300, 320, 320), (129, 96, 72), (4096, 960, 320), (77 * 3, 64, 32),
                                   (1000, 4, 2880)])
def test_linear(nat, M, N, K):
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    b, r = rnd(N, seed=3), rnd(M, N, seed=4)
    close(nat.linear(x, w), x.float() @ w.float().T)
    close(nat.linear(x, w, bias=b, residual=r), x.float() @ w.float().T + b.float() + r.float())


def test_linear_geglu(nat):
    M, C = 520, 64
    x, w, b = rnd(M, C, seed=1), rnd(8 * C, C, seed=2, scale=1 / 8), rnd(8 * C, seed=3)
    h = x.float() @ w.float().T + b.float()
    a, gate = h.chunk(2, dim=-1)
    ref = a * F.gelu(gate)
    # interleave rows: [16 x | 16 gate] blocks
    idx = []
    for q in range(4 * C // 16):
        idx += list(range(16 * q, 16 * q + 16)) + list(range(4 * C + 16 * q, 4 * C + 16 * q + 16))
    idx = torch.tensor(idx).cuda()
    close(nat.linear(x, w[idx].contiguous(), bias=b[idx].contiguous(), geglu=True), ref)


def _xres_source_rows(N):
    """row n of the X-resident GEGLU order <- row of the [x rows | gate rows] weight (include/univst.h, univst_geglu_xres_permute)"""
    n = torch.arange(N)
    nt, wn, i, g, r = n // 256, (n % 256) // 64, (n % 64) // 16, (n % 16) // 4, n % 4
    h = nt * 128 + wn * 32 + i * 8 + g * 2 + (r & 1)
    return torch.where(r < 2, h, N // 2 + h)


@pytest.mark.parametrize("M,N", [(4096 + 37, 2560), (24576, 2560), (100, 256), (65536, 512)])
def test_linear_geglu_x_resident(nat, M, N):
    """geglu = 2: the K = 320 projection on the kernel that keeps a block's 128 activation rows in LDS and streams the weights once per
    row block (weight rows interleaved [x0 x1 g0 g1 ...] by univst_geglu_xres_permute).  Reference: torch fp32 linear -> x * gelu(gate);
    ragged M, a single column tile, the row count of one frame-shard rank and the FF1 width of the 64x64 level."""
    K = 320
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K)), rnd(N, seed=3)
    src = _xres_source_rows(N).cuda()
    wp, bp = nat.geglu_xres_permute(w), nat.geglu_xres_permute(b)
    assert torch.equal(wp, w[src]) and torch.equal(bp, b[src]), "the permutation kernel and the documented row order differ"
    h = x.float() @ w.float().T + b.float()
    a, gate = h.chunk(2, dim=-1)
    close(nat.linear(x, wp, bias=bp, geglu=2), a * F.gelu(gate))
    close(nat.linear(x, wp, geglu=2), (x.float() @ w.float().T).chunk(2, dim=-1)[0] * F.gelu((x.float() @ w.float().T).chunk(2, dim=-1)[1]))
    # same values as the 256x320 / 128-wide GEGLU kernels up to fp16 rounding of identical fp32 math: compare directly as well
    idx = []
    for q in range(N // 32):
        idx += list(range(16 * q, 16 * q + 16)) + list(range(N // 2 + 16 * q, N // 2 + 16 * q + 16))
    idx = torch.tensor(idx).cuda()
    other = nat.linear(x, w[idx].contiguous(), bias=b[idx].contiguous(), geglu=True)
    assert (nat.linear(x, wp, bias=bp, geglu=2).float() - other.float()).abs().max().item() <= 2e-3 * other.float().abs().max().item()


def test_linear_geglu_x_resident_rejects_other_shapes(nat):
    x, w = rnd(512, 640, seed=1), rnd(2560, 640, seed=2)
    with pytest.raises(RuntimeError, match="K = 320"):
        nat.linear(x, w, geglu=2)


def test_linear_big_tile_path(nat):
    """shapes that dispatch to the 256x320 GLDS kernel (>= 150 tiles), incl. M tail, K tail, bias+residual, GEGLU."""
    M = 131072 + 77
    for N, K in ((320, 320), (640, 72)):
        x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
        b, r = rnd(N, seed=3), rnd(M, N, seed=4)
        close(nat.linear(x, w, bias=b, residual=r), x.float() @ w.float().T + b.float() + r.float())
    C = 80
    x, w, b = rnd(M, C, seed=1), rnd(8 * C, C, seed=2, scale=1 / 8), rnd(8 * C, seed=3)
    h = x.float() @ w.float().T + b.float()
    a, gate = h.chunk(2, dim=-1)
    idx = []
    for q in range(4 * C // 16):
        idx += list(range(16 * q, 16 * q + 16)) + list(range(4 * C + 16 * q, 4 * C + 16 * q + 16))
    idx = torch.tensor(idx).cuda()
    close(nat.linear(x, w[idx].contiguous(), bias=b[idx].contiguous(), geglu=True), a * F.gelu(gate))


def test_linear_big_tile_ragged_last_column_tile(nat):
    """N not a multiple of 320 on the 256 x 320 tile (the MM-DiT widths of the SD3 path: 1536 = 4.8 tiles; also 648 = 2 tiles + 8
    columns): weight rows >= N come from the zero page, both epilogues (LDS transpose with aligned rows, per-row otherwise) skip the
    columns >= N, nothing is written past a row's N columns (canary columns in a wider output buffer)."""
    for M, N, K, wide in ((40000 + 13, 1536, 192, 0), (50000, 648, 64, 0), (40000, 1536, 64, 1544)):
        x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
        b, r = rnd(N, seed=3), rnd(M, N, seed=4)
        ref = x.float() @ w.float().T + b.float() + r.float()
        if not wide:
            close(nat.linear(x, w, bias=b, residual=r), ref)
            close(nat.linear(x, w), x.float() @ w.float().T)
            continue
        from univst_amd import _native
        out = torch.full((M, wide), 7.0, device="cuda", dtype=torch.float16)
        _native.check(_native.load().univst_linear(x.data_ptr(), K, w.data_ptr(), b.data_ptr(), r.data_ptr(), N, out.data_ptr(), wide, M, N, K, 0,
                                                   _native.stream_ptr()), "linear")
        close(out[:, :N], ref)
        assert bool((out[:, N:] == 7.0).all()), "columns past N were written"


def test_conv_big_tile_path(nat):
    imgs, C1, C2, Co, H = 48, 32, 16, 320, 56        # 150528 output rows -> 588 tiles of 256x320
    x1, x2 = rnd(imgs, C1, H, H, seed=1), rnd(imgs, C2, H, H, seed=2)
    w = rnd(Co, C1 + C2, 3, 3, seed=3, scale=0.05)
    b, rb, res = rnd(Co, seed=4), rnd(3, Co, seed=5), rnd(imgs, Co, H, H, seed=6)
    ref = F.conv2d(torch.cat([x1, x2], 1).float(), w.float(), b.float(), padding=1)
    ref = ref + rb.float().repeat_interleave(16, 0)[:, :, None, None] + res.float()
    got = nat.conv_nhwc(nhwc(x1), conv_w(w), bias=b, x2=nhwc(x2), rowbias=rb, rows_per_rowbias=16 * H * H, residual=nhwc(res))
    close(got, nhwc(ref))
    x = rnd(imgs, 32, 32, 32, seed=7)
    w = rnd(Co, 32, 3, 3, seed=8, scale=0.06)
    ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
    close(nat.conv_nhwc(nhwc(x), conv_w(w), bias=b, upsample=True), nhwc(ref))


def test_split_k_paths(nat):
    """few output tiles, long reduction: fp32 partials [splits][M][N] + splitk_reduce_kernel (which runs the epilogue), on the
    128-row tiles (any N) and on the 256x320 tile (K >= 8192, 8..149 tiles)."""
    # small tiles: M tail, N not a multiple of the tile, bias + residual in the reduction kernel
    M, N, K = 517, 96, 4096
    x, w = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=1 / math.sqrt(K))
    b, r = rnd(N, seed=3), rnd(M, N, seed=4)
    close(nat.linear(x, w, bias=b, residual=r), x.float() @ w.float().T + b.float() + r.float())
    # 256x320 tile, linear: 9 x 4 tiles, K = 8192 -> 5 splits
    M, N, K = 2048 + 5, 1280, 8192
    x, w = rnd(M, K, seed=5), rnd(N, K, seed=6, scale=1 / math.sqrt(K))
    b, r = rnd(N, seed=7), rnd(M, N, seed=8)
    close(nat.linear(x, w, bias=b, residual=r), x.float() @ w.float().T + b.float() + r.float())
    # 256x320 tile, tap-inner conv over a virtual concat (K = 9 * 960), per-branch row bias + residual
    imgs, C1, C2, Co, H = 32, 640, 320, 320, 16          # 32 tiles x 5 splits
    x1, x2 = rnd(imgs, C1, H, H, seed=9), rnd(imgs, C2, H, H, seed=10)
    wc = rnd(Co, C1 + C2, 3, 3, seed=11, scale=1 / math.sqrt(9 * (C1 + C2)))
    bc, rb, res = rnd(Co, seed=12), rnd(16, Co, seed=13), rnd(imgs, Co, H, H, seed=14)
    ref = F.conv2d(torch.cat([x1, x2], 1).float(), wc.float(), bc.float(), padding=1)
    ref = ref + rb.float().repeat_interleave(2, 0)[:, :, None, None] + res.float()
    got = nat.conv_nhwc_tapinner(nhwc(x1), conv_w_ti(wc), bias=bc, x2=nhwc(x2), rowbias=rb, rows_per_rowbias=2 * H * H, residual=nhwc(res))
    close(got, nhwc(ref))


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_w(w):   # [Co,Ci,3,3] -> [Co,9,Ci]
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1, w.shape[1]).contiguous()


@pytest.mark.parametrize("Ci,Co,H,stride,up", [(32, 64, 16, 1, False), (64, 32, 16, 2, False), (32, 32, 8, 1, True),
                                               (8, 32, 16, 1, False), (320, 320, 16, 1, False), (96, 160, 12, 1, False)])
def test_conv3x3(nat, Ci, Co, H, stride, up):
    imgs = 6
    x = rnd(imgs, Ci, H, H, seed=1)
    w = rnd(Co, Ci, 3, 3, seed=2, scale=1 / math.sqrt(9 * Ci))
    b = rnd(Co, seed=3)
    xin = F.interpolate(x.float(), scale_factor=2.0, mode="nearest") if up else x.float()
    ref = F.conv2d(xin, w.float(), b.float(), stride=stride, padding=1)
    got = nat.conv_nhwc(nhwc(x), conv_w(w), bias=b, upsample=up, stride=stride)
    close(got, nhwc(ref))


def conv_w_ti(w):   # [Co,Ci,3,3] -> [Co,Ci/64,9,64]
    Co, Ci = w.shape[:2]
    return w.reshape(Co, Ci // 64, 64, 9).permute(0, 1, 3, 2).contiguous()


@pytest.mark.parametrize("C1,C2,Co,H,imgs,stride,up", [(64, 0, 64, 16, 6, 1, False), (128, 64, 96, 12, 6, 2, False),
                                                         (64, 64, 320, 56, 48, 1, False), (64, 0, 320, 28, 48, 1, True),
                                                         (64, 64, 320, 56, 48, 2, False),      # stride 2 on the 192-row tile (uniform-delta im2col)
                                                         (128, 0, 640, 30, 48, 1, False)])     # odd image width, 2 column tiles
def test_conv3x3_tap_inner_order(nat, C1, C2, Co, H, imgs, stride, up):
    x1 = rnd(imgs, C1, H, H, seed=1)
    x2 = rnd(imgs, C2, H, H, seed=2) if C2 else None
    w = rnd(Co, C1 + C2, 3, 3, seed=3, scale=1 / math.sqrt(9 * (C1 + C2)))
    b = rnd(Co, seed=4)
    xin = torch.cat([x1, x2], 1).float() if C2 else x1.float()
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.float(), b.float(), stride=stride, padding=1)
    got = nat.conv_nhwc_tapinner(nhwc(x1), conv_w_ti(w), bias=b, x2=None if x2 is None else nhwc(x2), upsample=up, stride=stride)
    close(got, nhwc(ref))


def conv_w_t32(w):   # [Co,Ci,3,3] -> [Co,Ci/32,9,32]
    Co, Ci = w.shape[:2]
    return w.reshape(Co, Ci // 32, 32, 9).permute(0, 1, 3, 2).contiguous()


@pytest.mark.parametrize("C1,C2,Co,H,imgs", [(320, 0, 320, 64, 12),      # 64x64 level, 192-row tiles (3 image rows): tiles straddle images
                                              (96, 32, 640, 32, 48),     # virtual concat (3 + 1 slabs: the ring crosses sources), 2 column tiles, 6-row tiles straddling
                                              (128, 0, 320, 16, 192),    # 16x16 level on 192-row tiles: 12 rows, every other tile straddles
                                              (32, 32, 320, 48, 21),     # 48-wide images, 4-row tiles aligned with the image
                                              (64, 0, 320, 64, 15),      # 256-row tiles (4 image rows)
                                              (64, 0, 320, 16, 240)])    # 256-row tiles = one whole 16x16 image each
def test_conv3x3_lds_patch(nat, C1, C2, Co, H, imgs):
    """conv_patch_kernel (input patch in LDS, k order [Cin/32][9][32]) vs F.conv2d: image borders (zero halo in the patch),
    tiles that start / end at an image boundary, tiles that straddle two images (the inserted zero row), virtual concat with
    the slab ring crossing from source 1 to source 2, per-branch row bias + residual epilogue."""
    x1 = rnd(imgs, C1, H, H, seed=1)
    x2 = rnd(imgs, C2, H, H, seed=2) if C2 else None
    w = rnd(Co, C1 + C2, 3, 3, seed=3, scale=1 / math.sqrt(9 * (C1 + C2)))
    b, rb, res = rnd(Co, seed=4), rnd(3, Co, seed=5), rnd(imgs, Co, H, H, seed=6)
    xin = torch.cat([x1, x2], 1).float() if C2 else x1.float()
    ref = F.conv2d(xin, w.float(), b.float(), padding=1)
    close(nat.conv3x3_patch(nhwc(x1), conv_w_t32(w), bias=b, x2=None if x2 is None else nhwc(x2)), nhwc(ref))
    ref2 = ref + rb.float().repeat_interleave(imgs // 3, 0)[:, :, None, None] + res.float()
    got2 = nat.conv3x3_patch(nhwc(x1), conv_w_t32(w), bias=b, x2=None if x2 is None else nhwc(x2), rowbias=rb,
                             rows_per_rowbias=(imgs // 3) * H * H, residual=nhwc(res))
    close(got2, nhwc(ref2))


def test_conv3x3_lds_patch_fused_upsample(nat):
    """UpsamplePseudo3D (resnet.py:123-175): nearest x2 folded into the patch addressing (source pixel = (y >> 1, x >> 1))."""
    imgs, Ci, Co, H = 48, 64, 320, 16                  # -> 32x32 outputs, 49152 rows: 192-row tiles straddling images
    x = rnd(imgs, Ci, H, H, seed=1)
    w = rnd(Co, Ci, 3, 3, seed=2, scale=1 / math.sqrt(9 * Ci))
    b = rnd(Co, seed=3)
    ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
    close(nat.conv3x3_patch(nhwc(x), conv_w_t32(w), bias=b, upsample=True), nhwc(ref))


@pytest.mark.parametrize("C1,C2,Co,H,imgs", [(1280, 0, 640, 16, 12),      # 24 tiles x 5 splits over 64-channel slab pairs
                                              (640, 640, 640, 16, 12),     # virtual concat, 24 tiles
                                              (64, 0, 320, 64, 20)])       # M tail: 81920 rows = 426.67 tiles of 192
def test_conv3x3_lds_patch_split_k_and_tail(nat, C1, C2, Co, H, imgs):
    """few tiles + long reduction (single-branch / frame-shard shapes): split-K over 64-channel slab pairs with fp32 partials
    and the epilogue in splitk_reduce_kernel; and a row count that is not a multiple of the tile height."""
    x1 = rnd(imgs, C1, H, H, seed=1)
    x2 = rnd(imgs, C2, H, H, seed=2) if C2 else None
    w = rnd(Co, C1 + C2, 3, 3, seed=3, scale=1 / math.sqrt(9 * (C1 + C2)))
    b, res = rnd(Co, seed=4), rnd(imgs, Co, H, H, seed=6)
    xin = torch.cat([x1, x2], 1).float() if C2 else x1.float()
    ref = F.conv2d(xin, w.float(), b.float(), padding=1) + res.float()
    got = nat.conv3x3_patch(nhwc(x1), conv_w_t32(w), bias=b, x2=None if x2 is None else nhwc(x2), residual=nhwc(res))
    close(got, nhwc(ref))


@pytest.mark.parametrize("C1,C2,Co,H,imgs", [(1280, 0, 1280, 8, 48),      # the 8x8 level: 4 (256-row) whole images per tile, split-K over slab pairs
                                              (1280, 1280, 1280, 8, 48),   # up-path concat at 8x8
                                              (64, 0, 320, 8, 800)])       # 8x8 images without split-K (200 tiles): 3 separators per 192-row tile
def test_conv3x3_lds_patch_small_images(nat, C1, C2, Co, H, imgs):
    """image width 8 (two image rows per 16-pixel MFMA fragment) and tiles that hold several whole images: one zero row between
    every two images of the patch."""
    x1 = rnd(imgs, C1, H, H, seed=1)
    x2 = rnd(imgs, C2, H, H, seed=2) if C2 else None
    w = rnd(Co, C1 + C2, 3, 3, seed=3, scale=1 / math.sqrt(9 * (C1 + C2)))
    b, res = rnd(Co, seed=4), rnd(imgs, Co, H, H, seed=6)
    xin = torch.cat([x1, x2], 1).float() if C2 else x1.float()
    ref = F.conv2d(xin, w.float(), b.float(), padding=1) + res.float()
    got = nat.conv3x3_patch(nhwc(x1), conv_w_t32(w), bias=b, x2=None if x2 is None else nhwc(x2), residual=nhwc(res))
    close(got, nhwc(ref))


def test_conv3x3_lds_patch_rejects_ineligible(nat):
    x = rnd(6, 32, 4, 4, seed=1)
    w = rnd(320, 32, 3, 3, seed=2)
    with pytest.raises(RuntimeError, match="not eligible"):
        nat.conv3x3_patch(nhwc(x), conv_w_t32(w))


def test_conv_concat_rowbias_residual(nat):
    imgs, Fr, C1, C2, Co, H = 6, 2, 64, 32, 64, 8      # 3 "branches" x 2 frames
    x1, x2 = rnd(imgs, C1, H, H, seed=1), rnd(imgs, C2, H, H, seed=2)
    w = rnd(Co, C1 + C2, 3, 3, seed=3, scale=0.05)
    b, rb, res = rnd(Co, seed=4), rnd(imgs // Fr, Co, seed=5), rnd(imgs, Co, H, H, seed=6)
    ref = F.conv2d(torch.cat([x1, x2], 1).float(), w.float(), b.float(), padding=1)
    ref = ref + rb.float().repeat_interleave(Fr, 0)[:, :, None, None] + res.float()
    got = nat.conv_nhwc(nhwc(x1), conv_w(w), bias=b, x2=nhwc(x2), rowbias=rb, rows_per_rowbias=Fr * H * H, residual=nhwc(res))
    close(got, nhwc(ref))
    # 1x1 shortcut over the virtual concat
    w1 = rnd(Co, C1 + C2, 1, 1, seed=7, scale=0.1)
    ref1 = F.conv2d(torch.cat([x1, x2], 1).float(), w1.float(), b.float())
    close(nat.conv_nhwc(nhwc(x1), conv_w(w1), bias=b, x2=nhwc(x2)), nhwc(ref1))


@pytest.mark.parametrize("C1,C2,G,H", [(32, 0, 8, 8), (64, 32, 8, 8), (640, 320, 32, 8), (320, 0, 32, 16), (1280, 1280, 32, 8)])
def test_groupnorm_5d_and_per_frame(nat, C1, C2, G, H):
    B, Fr = 3, 4
    x1 = rnd(B * Fr, C1, H, H, seed=1) * 2 + 0.5
    x2 = rnd(B * Fr, C2, H, H, seed=2) if C2 else None
    C = C1 + C2
    gam, bet = rnd(C, seed=3) * 0.1 + 1, rnd(C, seed=4) * 0.1
    full = torch.cat([x1, x2], 1) if C2 else x1
    x5 = full.float().view(B, Fr, C, H, H).permute(0, 2, 1, 3, 4)
    ref5 = F.silu(F.group_norm(x5, G, gam.float(), bet.float(), 1e-5)).permute(0, 2, 1, 3, 4).reshape(B * Fr, C, H, H)
    got5 = nat.groupnorm_nhwc(nhwc(x1), gam, bet, G, 1e-5, Fr * H * H, silu=True, x2=None if x2 is None else nhwc(x2))
    close(got5, nhwc(ref5))
    ref4 = F.group_norm(full.float(), G, gam.float(), bet.float(), 1e-6)
    got4 = nat.groupnorm_nhwc(nhwc(x1), gam, bet, G, 1e-6, H * H, silu=False, x2=None if x2 is None else nhwc(x2))
    close(got4, nhwc(ref4))


def test_groupnorm_large_mean(nat):
    """|mean| >> std in every group (real SD checkpoints have such channel groups; random-init activations do not): a raw
    one-pass E[x^2] - mean^2 in fp32 cancels here.  fp16 inputs 200 +- 0.25 (the fp16 grid is 0.125 there, so the spread is a
    few grid steps): the normalised output must still match the fp32 two-pass reference to 2e-3 of its range."""
    B, Fr, C, G, H = 3, 4, 320, 32, 32
    g = torch.Generator().manual_seed(9)
    x = (200.0 + 0.25 * torch.randn(B * Fr, C, H, H, generator=g) + 3.0 * torch.randn(1, C, 1, 1, generator=g)).half().cuda()
    gam, bet = rnd(C, seed=3) * 0.1 + 1, rnd(C, seed=4) * 0.1
    x5 = x.float().view(B, Fr, C, H, H).permute(0, 2, 1, 3, 4)
    ref5 = F.group_norm(x5.double(), G, gam.double(), bet.double(), 1e-5).float().permute(0, 2, 1, 3, 4).reshape(B * Fr, C, H, H)
    got5 = nat.groupnorm_nhwc(nhwc(x), gam, bet, G, 1e-5, Fr * H * H, silu=False)
    close(got5, nhwc(ref5))


@pytest.mark.parametrize("C", [32, 320, 640, 1280])
def test_layernorm(nat, C):
    x = rnd(777, C, seed=1) * 3 + 1
    g, b = rnd(C, seed=2) * 0.1 + 1, rnd(C, seed=3) * 0.1
    close(nat.layernorm(x, g, b), F.layer_norm(x.float(), (C,), g.float(), b.float(), 1e-5))


def sdpa_ref(q, k, v, heads):
    return unet_ref.sdpa(q.float(), k.float(), v.float(), heads)


def prescaled(q, d):
    """(q', q'/c): q multiplied by c = log2(e)/sqrt(d) and rounded to fp16 once — what the UNet graph's folded to_q weights
    produce — and the fp32 tensor the oracle must see so that both sides start from the SAME rounded values."""
    c = 1.4426950408889634 / math.sqrt(d)
    qp = (q.float() * c).to(torch.float16)
    return qp, qp.float() / c


@pytest.mark.parametrize("heads,d,N,Fr,mode,pre", [(2, 40, 2048 + 40, 2, "stock", 1), (8, 40, 2304, 1, "pnp", 1), (2, 40, 2048 + 40, 2, "stock", 0),
                                                    (2, 16, 64, 3, "stock", 0), (2, 32, 256, 4, "pnp", 0), (8, 40, 576, 2, "stock", 0), (8, 40, 576, 2, "stock", 1),
                                                    (8, 80, 128, 3, "pnp", 0), (8, 160, 64, 2, "stock", 0), (8, 80, 1024, 3, "stock", 1), (4, 80, 512 + 40, 2, "pnp", 1), (4, 160, 256, 2, "stock", 1), (2, 160, 640, 2, "pnp", 1), (4, 80, 200, 3, "stock", 1), (4, 64, 200, 2, "stock", 0)])
def test_attention_sparse_causal(nat, heads, d, N, Fr, mode, pre):
    """fused-QKV layout, K/V gathered by pointer from {prev, (cur), first} frames of the same branch.  pre: q carries
    log2(e)/sqrt(d) already (head_dim 40, Nq >= 2048 then runs the software-pipelined kernel)."""
    B, C = 3, heads * d
    qkv = rnd(B * Fr, N, 3 * C, seed=1)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    qref = q
    if pre:
        qp, qref = prescaled(q, d)
        qkv[..., :C] = qp
    index = [-1, 0, "first"] if mode == "stock" else [-1, "first"]
    kk = unet_ref.sparse_causal_gather(k.float().contiguous().cpu(), Fr, index).cuda()
    vv = unet_ref.sparse_causal_gather(v.float().contiguous().cpu(), Fr, index).cuda()
    ref = sdpa_ref(qref.contiguous(), kk, vv, heads)
    rows = []
    for b in range(B):
        for f in range(Fr):
            prev, first = b * Fr + max(f - 1, 0), b * Fr
            rows.append([prev, b * Fr + f, first] if mode == "stock" else [prev, first])
    src = torch.tensor(rows, dtype=torch.int32).cuda()
    got = nat.attention(q, k, v, src, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, q_prescaled=bool(pre))
    close(got, ref, rtol=4e-3)


@pytest.mark.parametrize("heads,d,N,Fl,mode,pre", [(8, 40, 2048 + 40, 2, "stock", 1), (8, 40, 2304, 2, "pnp", 1), (2, 40, 2048, 4, "pnp", 1), (8, 40, 576, 2, "stock", 0),
                                                    (4, 80, 1024, 2, "stock", 1), (4, 80, 512 + 40, 4, "pnp", 1), (4, 80, 200, 2, "pnp", 0), (4, 160, 256, 2, "stock", 1),
                                                    (2, 160, 64, 4, "pnp", 1), (2, 160, 640, 2, "pnp", 0), (4, 64, 200, 2, "stock", 0), (2, 32, 256, 1, "pnp", 0)])
def test_attention_two_phase_local_then_halo(nat, heads, d, N, Fl, mode, pre):
    """TWO-PHASE attention (univst_attention_phase; round 6): a rank of the frame shard holds Fl frames per branch plus two halo frames per branch (the frame
    before its first one and the clip's frame 0).  Launch 1 consumes the key frames the rank holds and leaves (m, l) per query; launch 2 continues over the
    halo frames and merges.  Against the oracle's gather + SDPA over the FULL key set of attention.py:384-413 (stock: [-1, 0, 'first']) / pnp_utils.py:59-84
    (PnP: [-1, 'first'] — the first local frame then has NO local source: phase 1 leaves it empty), both source tables, head_dim 40 (pipelined kernel from
    2048 queries on) / 80 / 160 / 64 / 32, Fl = 1, 2 and 4 local frames, a spiky halo frame (the merge must rescale the local part)."""
    B, C = 3, heads * d
    # a clip of Fl + 2 frames per branch stands in for (first, ..., prev | local frames): clip frame 0 = 'first', frame 1 = prev of the first local frame
    Fc = Fl + 2
    qkv = rnd(B * Fc, N, 3 * C, seed=7)
    qkv[Fc + 1, :, C:2 * C] *= 2.5                    # branch 1's halo (prev) frame: peaked scores in the second phase
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    qref = q
    if pre:
        qp, qref = prescaled(q, d)
        qkv[..., :C] = qp
    # reference: the reference's own index list on the clip (frame, 'first' = clip frame 0), rows of the local frames only
    index = [-1, 0, "first"] if mode == "stock" else [-1, "first"]
    kk = unet_ref.sparse_causal_gather(k.float().contiguous().cpu(), Fc, index).cuda()
    vv = unet_ref.sparse_causal_gather(v.float().contiguous().cpu(), Fc, index).cuda()
    ref = sdpa_ref(qref.contiguous(), kk, vv, heads).view(B, Fc, N, C)[:, 2:].reshape(B * Fl, N, C)
    # the rank's buffers: local frames first, then [B prev | B first] halo frames (the UNet graph's layout)
    view = qkv.view(B, Fc, N, 3 * C)
    buf = torch.cat([view[:, 2:].reshape(B * Fl, N, 3 * C), view[:, 1], view[:, 0]]).contiguous()
    ql, kl, vl = buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    loc, rem, c1, c2 = [], [], [], []
    for b in range(B):
        for f in range(Fl):
            prev_halo, first_halo = B * Fl + b, B * Fl + B + b
            if mode == "stock":
                l_ = [b * Fl + f] if f == 0 else [b * Fl + f - 1, b * Fl + f]
            else:
                l_ = [] if f == 0 else [b * Fl + f - 1]
            r_ = [prev_halo, first_halo] if f == 0 else [first_halo]
            c1.append(len(l_)); c2.append(len(r_))
            loc.append((l_ + [0, 0])[:2]); rem.append((r_ + [0, 0])[:2])
    loc, rem = torch.tensor(loc, dtype=torch.int32).cuda(), torch.tensor(rem, dtype=torch.int32).cuda()
    c1, c2 = torch.tensor(c1, dtype=torch.int32).cuda(), torch.tensor(c2, dtype=torch.int32).cuda()
    qq = ql[:B * Fl]
    out, st = nat.attention_phase(qq, kl, vl, loc, c1, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, q_prescaled=bool(pre))
    if mode == "pnp":          # the first local frame of every branch had no local source: empty phase
        assert float(st.view(B, Fl, heads, N, 2)[:, 0, :, :, 1].abs().max()) == 0.0 and float(out.view(B, Fl, N, C)[:, 0].abs().max()) == 0.0
    got = nat.attention_phase(qq, kl, vl, rem, c2, heads, out=out, state_in=st, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, q_prescaled=bool(pre))
    close(got, ref, rtol=4e-3)
    # and the split is invisible: one launch over the union of the sources gives the same rows up to the fp16 rounding of the phase-1 rows
    rows, cnt = [], []
    for i in range(B * Fl):
        u = loc[i, :int(c1[i])].tolist() + rem[i, :int(c2[i])].tolist()
        cnt.append(len(u)); rows.append((u + [0] * 4)[:4])
    one = nat.attention(qq, kl, vl, torch.tensor(rows, dtype=torch.int32).cuda(), heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C,
                        src_cnt=torch.tensor(cnt, dtype=torch.int32).cuda(), q_prescaled=bool(pre))
    close(got, one, rtol=2e-3)


@pytest.mark.parametrize("heads,d,N,Fl,mode,pre", [(8, 40, 1024, 2, "stock", 0), (8, 40, 1024, 2, "stock", 1), (8, 40, 512, 4, "pnp", 0), (8, 80, 1024, 2, "stock", 0),
                                                    (8, 80, 1024, 4, "pnp", 1), (8, 160, 512, 2, "stock", 1), (8, 64, 1024, 2, "stock", 0), (8, 40, 4096, 2, "pnp", 1),
                                                    (8, 64, 1024, 2, "stock", 1), (8, 64, 2048, 2, "pnp", 1)])      # d = 64 prescaled: the pipelined kernel's two-phase forms
def test_attention_two_phase_error_is_rounding_level(nat, heads, d, N, Fl, mode, pre):
    """The two-phase attention against an fp32 softmax over the full key set with a ROUNDING-LEVEL bound (rms 6e-4 of the rms, max 2.5e-3 of the max; the
    one-launch kernel measures 3.0e-4 / 5e-4, the split 3.3e-4) on launches of MORE blocks than the chip has CUs.  Round 6: with one kernel serving both
    phases through run-time branches, the 128-query-row bodies at head_dim 40 / 80 left sporadic x * 0 elements in the first phase's rows whenever blocks were
    co-resident on a CU — 0.2 of the maximum, invisible to `close`'s 2e-3-of-the-maximum absolute floor at the sizes tested then.  Also checks the state:
    m + log2(l) of phase 1 is the log-sum-exp of its scores."""
    B, C = 3, heads * d
    g = torch.Generator().manual_seed(3)
    buf = torch.randn(B * Fl + 2 * B, N, 3 * C, generator=g).half().cuda()
    q, k, v = buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    loc, rem, full = [], [], []
    for b in range(B):
        for f in range(Fl):
            ph, fh = B * Fl + b, B * Fl + B + b
            l_ = ([b * Fl + f] if f == 0 else [b * Fl + f - 1, b * Fl + f]) if mode == "stock" else ([] if f == 0 else [b * Fl + f - 1])
            r_ = [ph, fh] if f == 0 else [fh]
            loc.append(l_); rem.append(r_); full.append(l_ + r_)
    qq = q[:B * Fl]
    c = 1.4426950408889634 / d ** 0.5

    qf = [qq.float()]               # the queries the reference uses (fp32): the raw ones, or the prescaled ones the kernel sees divided by the factor

    def ref(rows, want_lse=False):
        out = torch.zeros(B * Fl, N, C, device="cuda")
        lse = torch.full((B * Fl, heads, N), float("nan"), device="cuda")
        for i, srcs in enumerate(rows):
            if not srcs:
                continue
            kk = torch.cat([k[s_] for s_ in srcs]).float().view(-1, heads, d).transpose(0, 1)
            vv = torch.cat([v[s_] for s_ in srcs]).float().view(-1, heads, d).transpose(0, 1)
            sc = qf[0][i].view(N, heads, d).transpose(0, 1) @ kk.transpose(1, 2) / d ** 0.5
            lse[i] = torch.logsumexp(sc, -1) * 1.4426950408889634
            out[i] = (torch.softmax(sc, -1) @ vv).transpose(0, 1).reshape(N, C)
        return (out, lse) if want_lse else out
    if pre:
        buf[:B * Fl, :, :C] = (qq.float() * c).half()
        qf[0] = buf[:B * Fl, :, :C].float() / c
    want = ref(full)
    want1, lse1 = ref(loc, True)
    ti = lambda a, w: torch.tensor([(r + [0] * w)[:w] for r in a], dtype=torch.int32).cuda()
    tc = lambda a: torch.tensor([len(r) for r in a], dtype=torch.int32).cuda()
    W = 3 if mode == "stock" else 2
    tl, tc1, tr, tc2 = ti(loc, W), tc(loc), ti(rem, W), tc(rem)                # (kept alive over the launches)
    out, st = nat.attention_phase(qq, k, v, tl, tc1, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, q_prescaled=bool(pre))
    o1 = out.clone().float()
    ok = ~torch.isnan(lse1)
    assert float((st[..., 0] + torch.log2(st[..., 1]) - lse1)[ok].abs().max()) < 5e-3
    got = nat.attention_phase(qq, k, v, tr, tc2, heads, out=out, state_in=st, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, q_prescaled=bool(pre)).float()
    torch.cuda.synchronize()
    for name, a, b in (("phase 1", o1, want1), ("merged", got, want)):
        rms, mx = float((a - b).pow(2).mean().sqrt() / b.pow(2).mean().sqrt()), float((a - b).abs().max() / b.abs().max())
        assert rms < 6e-4 and mx < 2.5e-3, (name, rms, mx)


def test_attention_merged_duplicate_sources(nat):
    """a source listed m times == the source once with log2(m) added to its scores (what the UNet graph does for the
    duplicated frame 0 at f = 0, 1)."""
    heads, d, N = 8, 40, 320
    C = heads * d
    qkv = rnd(3, N, 3 * C, seed=1)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    dup = torch.tensor([[0, 0, 0], [0, 1, 0], [1, 2, 0]], dtype=torch.int32).cuda()
    # the oracle sees the reference's key set: every listed source concatenated, duplicates included
    kk = torch.stack([torch.cat([k[j] for j in row]) for row in dup.tolist()]).float()
    vv = torch.stack([torch.cat([v[j] for j in row]) for row in dup.tolist()]).float()
    ref = sdpa_ref(q.contiguous(), kk, vv, heads)
    close(nat.attention(q, k, v, dup, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C), ref, rtol=4e-3)      # duplicates read as listed
    uniq = torch.tensor([[0, 0, 0], [0, 1, 0], [1, 2, 0]], dtype=torch.int32).cuda()
    cnt = torch.tensor([1, 2, 3], dtype=torch.int32).cuda()
    lw = torch.tensor([[math.log2(3), 0, 0], [1.0, 0, 0], [0, 0, 0]], dtype=torch.float32).cuda()
    got = nat.attention(q, k, v, uniq, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, src_cnt=cnt, src_logw=lw)
    close(got, ref, rtol=4e-3)                                                                          # merged: once + log2 multiplicity


def test_attention_cross_77(nat):
    heads, d, N, BF, B = 8, 40, 300, 6, 3
    C = heads * d
    q = rnd(BF, N, C, seed=1)
    kv = rnd(B, 77, 2 * C, seed=2)
    k, v = kv[..., :C], kv[..., C:]
    src = torch.tensor([[i // 2] for i in range(BF)], dtype=torch.int32).cuda()
    ref = sdpa_ref(q, k.float().repeat_interleave(2, 0), v.float().repeat_interleave(2, 0), heads)
    got = nat.attention(q, k, v, src, heads, ldkv=2 * C, Nkv=77, C_=C)
    close(got, ref, rtol=4e-3)


@pytest.mark.parametrize("heads,d,N,Nkv,pre", [(8, 40, 4096, 77, 1), (8, 40, 1000, 77, 0), (8, 80, 1024, 77, 0), (4, 80, 300, 80, 1),
                                               (8, 40, 257, 13, 0), (2, 80, 2048 + 31, 64, 0), (8, 40, 640, 65, 1)])
def test_attention_text_register_kernel(nat, heads, d, N, Nkv, pre):
    """attn_text_kernel (one source of <= 80 keys, head_dim 40 / 80, K / V held in registers): ragged query counts (tails inside a
    32-row wave tile, a 1024-row block chunk and the 128-row iteration), key counts that end inside any of the five key fragments,
    prescaled and plain q, strided q / kv rows as the UNet graph passes them.  fp16 tolerance 4e-3 of the output scale."""
    BF, B = 6, 3
    C = heads * d
    qbuf = rnd(BF, N, C + 64, seed=1)                 # row stride wider than C
    q = qbuf[..., :C]
    kv = rnd(B, Nkv, 2 * C, seed=2)
    kv[1] *= 3.0                                       # one branch with peaked scores
    k, v = kv[..., :C], kv[..., C:]
    src = torch.tensor([[i // 2] for i in range(BF)], dtype=torch.int32).cuda()
    if pre:
        qp, qref = prescaled(q, d)
        qpb = torch.zeros_like(qbuf)
        qpb[..., :C] = qp
        got = nat.attention(qpb[..., :C], k, v, src, heads, ldq=C + 64, ldkv=2 * C, Nkv=Nkv, C_=C, q_prescaled=True)
    else:
        qref = q
        got = nat.attention(q, k, v, src, heads, ldq=C + 64, ldkv=2 * C, Nkv=Nkv, C_=C)
    ref = sdpa_ref(qref, k.float().repeat_interleave(2, 0), v.float().repeat_interleave(2, 0), heads)
    close(got, ref, rtol=4e-3)


def test_attention_softmax_spike(nat):
    """force large running-max jumps between key tiles (online-softmax rescale path)."""
    heads, d, N = 2, 32, 256
    C = heads * d
    q, k, v = rnd(1, N, C, seed=1), rnd(1, N, C, seed=2), rnd(1, N, C, seed=3)
    k[0, 200] = q[0, 5] * 6           # a spike in the 4th tile for query 5
    k[0, 70] = q[0, 9] * 5
    src = torch.zeros(1, 1, dtype=torch.int32).cuda()
    close(nat.attention(q, k, v, src, heads), sdpa_ref(q, k, v, heads), rtol=4e-3)


# ---- the software-pipelined head_dim-40 kernel (Nq >= 2048): scale / running reference folded into the QK^T MFMA ----------
def test_attention_d40_long_reference_jumps(nat):
    """large, late, positive AND negative score excursions: the quantised (multiple-of-8 + remainder) reference is rewritten
    mid-stream, pending scores are shifted, O^T rescaled once; ragged key count (tail tile) on top."""
    heads, d, N = 2, 40, 2048 + 72
    C = heads * d
    q, k, v = rnd(1, N, C, seed=1) * 2, rnd(1, N, C, seed=2), rnd(1, N, C, seed=3)
    k[0, 1500] = q[0, 5] * 6            # raw score ~ 6*|q|^2: hundreds of log2 units above the rest, in a late tile
    k[0, 70] = q[0, 9] * 5
    k[0, 2100] = q[0, 2000] * 4         # inside the tail tile
    q[0, 300] = -k[0, :64].mean(0) * 30  # a query whose early scores are all strongly negative (negative first reference)
    k[0, :32] = k[0, 3]                  # ... and one whose first 32 scores are all about -145 in log2 units (2^145 overflows fp32)
    q[0, 400] = -k[0, 3] * 16
    src = torch.zeros(1, 1, dtype=torch.int32).cuda()
    qp, qref = prescaled(q, d)
    close(nat.attention(qp, k, v, src, heads, q_prescaled=True), sdpa_ref(qref, k, v, heads), rtol=4e-3)
    close(nat.attention(q, k, v, src, heads), sdpa_ref(q, k, v, heads), rtol=4e-3)      # plain q: attn_body


def test_attention_d40_long_merged_sources_and_text(nat):
    heads, d, N = 8, 40, 2048
    C = heads * d
    qkv = rnd(3, N, 3 * C, seed=1)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    qp, qref = prescaled(q, d)
    qkv[..., :C] = qp
    dup = torch.tensor([[0, 0, 0], [0, 1, 0], [1, 2, 0]], dtype=torch.int32).cuda()
    kk = torch.stack([torch.cat([k[j] for j in row]) for row in dup.tolist()]).float()
    vv = torch.stack([torch.cat([v[j] for j in row]) for row in dup.tolist()]).float()
    ref = sdpa_ref(qref.contiguous(), kk, vv, heads)
    cnt = torch.tensor([1, 2, 3], dtype=torch.int32).cuda()
    lw = torch.tensor([[math.log2(3), 0, 0], [1.0, 0, 0], [0, 0, 0]], dtype=torch.float32).cuda()
    got = nat.attention(q, k, v, dup, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, src_cnt=cnt, src_logw=lw, q_prescaled=True)
    close(got, ref, rtol=4e-3)
    # 77 text tokens against 2304 queries: one unweighted source of at most 80 keys goes to attn_text_kernel<40> (K/V in registers, no key tiles);
    # the register-staged attn_pp40_kernel<1,0,false,0> and its tail tile are held by tests/test_gpu_attention.py
    qx = rnd(2, 2304, C, seed=4)
    kv = rnd(2, 77, 2 * C, seed=5)
    kt, vt = kv[..., :C], kv[..., C:]
    src = torch.tensor([[0], [1]], dtype=torch.int32).cuda()
    qxp, qxref = prescaled(qx, d)
    close(nat.attention(qxp, kt, vt, src, heads, ldkv=2 * C, Nkv=77, C_=C, q_prescaled=True), sdpa_ref(qxref, kt, vt, heads), rtol=4e-3)


# ---- the software-pipelined head_dim-64 kernel (prescaled q, Nq >= 1024): reference in the MFMA accumulator, dot2 row sums --------
@pytest.mark.parametrize("d", [64, 80])
def test_attention_d64_long_reference_jumps(nat, d):
    """the d = 40 kernel's torture cases at head_dim 64 and 80 (attn_pp64_kernel<64, 4> / <80, 2>: the latter with a half-padded third k
    step and 32 query rows per wave): late large positive excursions, strongly negative first scores, ragged key and query counts; the
    same inputs with plain q (generic body) for comparison."""
    heads, N = 2, 1024 + 200
    C = heads * d
    q, k, v = rnd(1, N, C, seed=1) * 2, rnd(1, N, C, seed=2), rnd(1, N, C, seed=3)
    k[0, 900] = q[0, 5] * 6
    k[0, 70] = q[0, 9] * 5
    k[0, 1200] = q[0, 1000] * 4          # inside the tail tile
    q[0, 300] = -k[0, :64].mean(0) * 30
    k[0, :32] = k[0, 3]
    q[0, 400] = -k[0, 3] * 16
    src = torch.zeros(1, 1, dtype=torch.int32).cuda()
    qp, qref = prescaled(q, d)
    close(nat.attention(qp, k, v, src, heads, q_prescaled=True), sdpa_ref(qref, k, v, heads), rtol=4e-3)
    close(nat.attention(q, k, v, src, heads), sdpa_ref(q, k, v, heads), rtol=4e-3)


@pytest.mark.parametrize("d", [64, 80])
def test_attention_d64_long_merged_sources(nat, d):
    heads, N = 4, 1088
    C = heads * d
    qkv = rnd(3, N, 3 * C, seed=1)
    q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    qp, qref = prescaled(q, d)
    qkv[..., :C] = qp
    dup = torch.tensor([[0, 0, 0], [0, 1, 0], [1, 2, 0]], dtype=torch.int32).cuda()
    kk = torch.stack([torch.cat([k[j] for j in row]) for row in dup.tolist()]).float()
    vv = torch.stack([torch.cat([v[j] for j in row]) for row in dup.tolist()]).float()
    ref = sdpa_ref(qref.contiguous(), kk, vv, heads)
    cnt = torch.tensor([1, 2, 3], dtype=torch.int32).cuda()
    lw = torch.tensor([[math.log2(3), 0, 0], [1.0, 0, 0], [0, 0, 0]], dtype=torch.float32).cuda()
    got = nat.attention(q, k, v, dup, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, src_cnt=cnt, src_logw=lw, q_prescaled=True)
    close(got, ref, rtol=4e-3)
    # un-merged (three explicit sources) gives the same
    got2 = nat.attention(q, k, v, dup, heads, ldq=3 * C, ldkv=3 * C, Nkv=N, C_=C, q_prescaled=True)
    close(got2, ref, rtol=4e-3)


@pytest.mark.parametrize("C,N,Fr,idx", [(64, 64, 4, 0), (320, 256, 3, 13), (1280, 64, 2, 25)])
def test_attention_adain_shift(nat, C, N, Fr, idx):
    qkv = (rnd(3 * Fr * N, 3 * C, seed=1) * 1.5 + 0.2)
    q, k, v = (qkv[:, i * C:(i + 1) * C].float().cpu().view(3 * Fr, N, C) for i in range(3))
    rq, rk, rv = unet_ref.pnp_shift(q, k, v, idx)
    beta = unet_ref.pnp_beta(idx)
    got = nat.attention_adain_shift_(qkv.clone(), Fr, N, C, 0.65, beta, 3.0).float().cpu()
    ref = torch.cat([rq.reshape(-1, C), rk.reshape(-1, C), rv.reshape(-1, C)], 1)
    close(got, ref, rtol=3e-3)
    assert torch.equal(got[:2 * Fr * N], qkv[:2 * Fr * N].float().cpu()), "content/style rows must be untouched"


def test_attention_adain_shift_large_mean(nat):
    """style K / V columns with |mean| >> std — mean 200, std 0.25, about the most extreme ratio fp16 inputs can carry (ulp 0.125 at
    200): a one-pass fp32 E[x^2] - mean^2 keeps ~4 significant bits of the variance there.  colstats takes its sums about a pivot
    and merges the row phases in double, so the per-(frame, channel) statistics must match torch's float64 ones to 1e-4 relative."""
    C, N, Fr, idx = 320, 4096, 2, 13
    g = torch.Generator().manual_seed(5)
    qkv = (torch.randn(3 * Fr * N, 3 * C, generator=g) * 0.25 + 200.0).half().cuda()
    q, k, v = (qkv[:, i * C:(i + 1) * C].float().cpu().view(3 * Fr, N, C) for i in range(3))
    rq, rk, rv = unet_ref.pnp_shift(q, k, v, idx)
    out, mean, std = nat.attention_adain_shift_(qkv.clone(), Fr, N, C, 0.65, unet_ref.pnp_beta(idx), 3.0, return_stats=True)
    sty = torch.cat([k[Fr:2 * Fr], v[Fr:2 * Fr]], -1).double()                 # style branch, [Fr, N, 2C]
    assert ((mean.cpu().double() - sty.mean(1)).abs() / 200.0).max().item() < 1e-6
    assert (std.cpu().double() / sty.std(1) - 1).abs().max().item() < 1e-4
    got = out.float().cpu()
    ref = torch.cat([rq.reshape(-1, C), rk.reshape(-1, C), rv.reshape(-1, C)], 1)
    err = (got[2 * Fr * N:, C:] - ref[2 * Fr * N:, C:]).abs().max().item()
    assert err <= 2 * 0.125 + 1e-6, err                       # K / V outputs: 2 fp16 ulps at 200


def test_latent_adain_and_elementwise(nat, golden):
    g = golden("g1_latent_adain")
    got = nat.latent_adain(g["cnt"].half().cuda(), g["sty"].half().cuda())
    close(got, unet_ref.latent_adain(g["cnt"].half().float(), g["sty"].half().float()), rtol=3e-3)
    c, s = rnd(1, 4, 16, 64, 64, seed=1), rnd(1, 4, 16, 64, 64, seed=2) * 0.7 + 0.1
    close(nat.latent_adain(c, s), unet_ref.latent_adain(c.float(), s.float()), rtol=3e-3)
    close(nat.axpby(c, s, 0.97, -0.13), 0.97 * c.float() - 0.13 * s.float())
    m = (torch.rand(16, 64, 64) > 0.5).half().cuda()
    close(nat.mask_blend(c, s, m), (1 - m.float()) * c.float() + m.float() * s.float())
    close(nat.mask_blend(c, s, None), c.float())


def test_mask_resize(nat):
    m = torch.from_numpy((si.disc_masks(16, 512, 512) > 0).astype(np.uint8)).cuda()
    ref = F.interpolate(m[None].float(), size=(64, 64), mode="bilinear", align_corners=False)[0]
    got = nat.mask_resize(m, 64, 64)
    assert torch.equal(got.float(), ref), "mask resize values {0,.25,.5,.75,1} must be exact"


@pytest.mark.parametrize("M,C,Nf,geglu,res,row_mean", [(49152, 320, 960, False, False, 0.7), (49152, 320, 320, False, True, 0.7),
                                                       (49152, 640, 5120, True, False, 0.7), (40000, 1280, 1280, False, False, 0.7),
                                                       (49152, 320, 960, False, False, 30.0),
                                                       # the levels of one rank of an 8-GPU frame shard: producer (and, but for the first, consumer) on the
                                                       # 128-wide kernel — 160-, 128-column tiles of 128 rows and 128-column tiles of 64 rows; a ragged M
                                                       (24576, 320, 960, False, False, 0.7), (24576, 320, 320, False, True, 0.7), (6144, 640, 640, False, True, 0.7),
                                                       (6144, 640, 1920, False, False, 0.7), (6100, 640, 640, False, False, 30.0)])
def test_linear_layernorm_fold(nat, M, C, Nf, geglu, res, row_mean):
    """univst_linear_ln: a producer linear leaves (sum, sumsq) per row and 160-column slot; the consumer runs on the raw rows with
    gamma folded into the weight and applies rstd * (acc - mean * wsum) + lnb.  Reference: torch fp32 LayerNorm -> linear
    (-> GEGLU / + residual) on the producer's fp16 output.  fp16 tolerance: 2e-3 of the output scale (max), 5e-4 rms."""
    g = torch.Generator().manual_seed(M + C + Nf)
    x0 = torch.randn(M, C, generator=g).half().cuda()
    wp = (torch.randn(C, C, generator=g) / math.sqrt(C)).half().cuda()
    # rows with a mean well away from 0 (the statistics are one-pass sums in fp32: E[x^2] - mean^2 loses log2(1 + mean^2/var) bits;
    # the last case has mean = 30 std, far beyond what a residual stream shows, and still has to hold the tolerance)
    bp = (row_mean + 0.3 * torch.randn(C, generator=g)).half().cuda()
    stats = torch.full((M, C // 160, 2), float("nan"), device="cuda", dtype=torch.float32)
    x = nat.linear_ln(x0, wp, bias=bp, stats_out=stats)
    assert torch.equal(x, nat.linear(x0, wp, bias=bp)), "emitting the statistics must not change the output"
    xf = x.float()
    want_st = torch.stack([xf.view(M, C // 160, 160).sum(-1), (xf * xf).view(M, C // 160, 160).sum(-1)], -1)
    assert torch.allclose(stats, want_st, rtol=2e-5, atol=1e-3), (stats - want_st).abs().max().item()
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).half().cuda()
    beta = (0.2 * torch.randn(C, generator=g)).half().cuda()
    w = (torch.randn(Nf, C, generator=g) / math.sqrt(C)).half().cuda()
    b = (0.1 * torch.randn(Nf, generator=g)).half().cuda()
    r = torch.randn(M, Nf, generator=g).half().cuda() if res else None
    wref, bref = w, b
    if geglu:          # rows interleaved [16 x | 16 gate] as the kernel expects
        idx = []
        for q in range(Nf // 32):
            idx += list(range(16 * q, 16 * q + 16)) + list(range(Nf // 2 + 16 * q, Nf // 2 + 16 * q + 16))
        idx = torch.tensor(idx).cuda()
        w, b = w[idx].contiguous(), b[idx].contiguous()
    wl = (w.float() * gamma.float()[None]).half()
    wsum = wl.float().sum(1).contiguous()
    lnb = (b.float() + w.float() @ beta.float()).contiguous()
    got = nat.linear_ln(x, wl, residual=r, geglu=geglu, ln=(stats, wsum, lnb)).float()
    xn = torch.nn.functional.layer_norm(xf, (C,), gamma.float(), beta.float(), 1e-5)
    y = xn @ wref.float().t() + bref.float()
    if geglu:
        a, gate = y.chunk(2, dim=-1)
        y = a * F.gelu(gate)
    if res:
        y = y + r.float()
    scale = y.abs().max().item()
    mx = (got - y).abs().max().item() / scale
    rms = ((got - y).pow(2).mean().sqrt() / y.pow(2).mean().sqrt()).item()
    assert mx < 2e-3 and rms < 5e-4, (mx, rms)


@pytest.mark.parametrize("M,row_mean", [(49152, 0.7), (6144 + 5, 30.0)])
def test_linear_geglu_x_resident_layernorm_fold(nat, M, row_mean):
    """norm3 folded into the X-resident GEGLU projection (K = 320): statistics from a producer linear, gamma folded into the permuted
    weight, wsum / lnb in the permuted row order.  Same reference and bars as test_linear_layernorm_fold."""
    C, Nf = 320, 2560
    g = torch.Generator().manual_seed(M)
    x0 = torch.randn(M, C, generator=g).half().cuda()
    wp_ = (torch.randn(C, C, generator=g) / math.sqrt(C)).half().cuda()
    bp_ = (row_mean + 0.3 * torch.randn(C, generator=g)).half().cuda()
    stats = torch.zeros(M, C // 160, 2, device="cuda", dtype=torch.float32)
    x = nat.linear_ln(x0, wp_, bias=bp_, stats_out=stats)
    gamma = (1.0 + 0.3 * torch.randn(C, generator=g)).half().cuda()
    beta = (0.2 * torch.randn(C, generator=g)).half().cuda()
    w = (torch.randn(Nf, C, generator=g) / math.sqrt(C)).half().cuda()
    b = (0.1 * torch.randn(Nf, generator=g)).half().cuda()
    src = _xres_source_rows(Nf).cuda()
    wx, bx = w[src].contiguous(), b[src].contiguous()
    wl = (wx.float() * gamma.float()[None]).half()
    wsum = wl.float().sum(1).contiguous()
    lnb = (bx.float() + wx.float() @ beta.float()).contiguous()
    got = nat.linear_ln(x, wl, geglu=2, ln=(stats, wsum, lnb)).float()
    xn = torch.nn.functional.layer_norm(x.float(), (C,), gamma.float(), beta.float(), 1e-5)
    a, gate = (xn @ w.float().t() + b.float()).chunk(2, dim=-1)
    y = a * F.gelu(gate)
    mx = (got - y).abs().max().item() / y.abs().max().item()
    rms = ((got - y).pow(2).mean().sqrt() / y.pow(2).mean().sqrt()).item()
    assert mx < 2e-3 and rms < 5e-4, (mx, rms)


def test_linear_layernorm_fold_rejects_split_k_problems(nat):
    """a problem the launcher runs with split-K (few tiles, long reduction: the 16x16 level of a frame shard) has its epilogue in the
    reduction kernel: no statistics, no fold — refused loudly instead of silently skipped"""
    x = torch.randn(1536, 1280).half().cuda()
    w = torch.randn(1280, 1280).half().cuda()
    with pytest.raises(RuntimeError, match="not taken by the direct"):
        nat.linear_ln(x, w, stats_out=torch.empty(1536, 8, 2, device="cuda"))
    st = torch.zeros(1536, 8, 2, device="cuda")
    with pytest.raises(RuntimeError, match="not taken by the direct"):
        nat.linear_ln(x, w, ln=(st, torch.zeros(1280, device="cuda"), torch.zeros(1280, device="cuda")))


@pytest.mark.parametrize("Ci,Co,H,imgs,up", [(256, 256, 64, 16, False), (512, 512, 32, 16, False), (512, 256, 64, 8, False), (256, 256, 32, 16, True)])
def test_conv_big_tile_ragged_width(nat, Ci, Co, H, imgs, up):
    """3x3 convs whose width is not a multiple of the 320-column tile (the temporal VAE: 256, 512) on the 256x320 tile with a partly filled last
    column tile (round 5), tap-inner and plain k order, with and without the fused nearest x2: vs torch fp32 on the same fp16 inputs"""
    x = rnd(imgs, H, H, Ci, seed=1)
    w = rnd(Co, Ci, 3, 3, seed=2, scale=1 / math.sqrt(9 * Ci))
    b, r = rnd(Co, seed=3), rnd(imgs, H * (2 if up else 1), H * (2 if up else 1), Co, seed=4)
    xin = x.float().permute(0, 3, 1, 2)
    if up:
        xin = F.interpolate(xin, scale_factor=2.0, mode="nearest")
    ref = F.conv2d(xin, w.float(), b.float(), padding=1).permute(0, 2, 3, 1) + r.float()
    wn = w.permute(0, 2, 3, 1).reshape(Co, 9, Ci).contiguous()
    close(nat.conv_nhwc(x, wn, bias=b, residual=r, upsample=up), ref)
    if not up:
        wti = w.reshape(Co, Ci // 64, 64, 9).permute(0, 1, 3, 2).contiguous()
        close(nat.conv_nhwc_tapinner(x, wti, bias=b, residual=r), ref)
