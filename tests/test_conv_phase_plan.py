"""CPU: the phase form of the upsampler convs (GemmParams::W4, announced to univst_debug_gemm_plan by UNIVST_PLAN_W4) is a run-time mode of the existing
conv_patch_kernel instantiations — a plan queried with the phase copy names the same symbol and grid as without it, and problems that are not eligible
for the phase form keep today's line."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "dispatch_plan.txt")
NCU = 256
BIAS, RES, ROWBIAS, W32_ONLY, W32, GN_OUT, WORKSPACE, W4 = 1, 2, 4, 128, 256, 512, 4096, 8192
GRAPH = BIAS | W32 | GN_OUT | WORKSPACE          # what the UNet graph passes for an upsampler conv


@pytest.fixture(scope="module")
def lib():
    from univst_amd import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native.load()


def conv_line(lib, imgs, N, C1, Hs, Ws, flags, up=1, C2=0, ncu=NCU):
    buf = C.create_string_buffer(8192)
    rc = lib.univst_debug_gemm_plan(ncu, 1, imgs, N, 0, 0, flags, 0, C1, C2, Hs, Ws, up, 1, 9, 0, buf, 8192)
    return rc, buf.value.decode()


def test_flag_value_matches_the_header():
    src = open(os.path.join(ROOT, "include", "univst.h")).read()
    assert int(re.search(r"#define UNIVST_PLAN_W4 (\d+)", src).group(1)) == W4


@pytest.mark.parametrize("imgs,C,Hs,Ws,sym,grid", [(48, 640, 32, 32, "conv_patch_kernel<4>", 1536), (48, 1280, 16, 16, "conv_patch_kernel<4>", 768),
                                                   (48, 1280, 8, 8, "conv_patch_kernel<3>", 256)])
def test_unet_upsampler_shapes_keep_symbol_and_grid(lib, imgs, C, Hs, Ws, sym, grid):
    """the three upsampler convs of the 16 x 512 x 512 three-branch step: 4 phases x a quarter of the row tiles = the 9-tap grid"""
    rc0, without = conv_line(lib, imgs, C, C, Hs, Ws, GRAPH)
    rc1, with_w4 = conv_line(lib, imgs, C, C, Hs, Ws, GRAPH | W4)
    assert rc0 == 0 and rc1 == 0 and with_w4 == without
    assert without.startswith(f"{sym} grid={grid} block=512 splits=1 ")


def test_recorded_upsample_rows_give_their_line_with_the_phase_copy(lib):
    """every recorded conv row with upsample = 1: the same line with UNIVST_PLAN_W4 added to its flags (patch rows take the phase form or not — symbol,
    grid and splits are the same either way; rows on other kernels are untouched by the flag)"""
    n = patch = 0
    for line in open(TABLE):
        if not line.startswith("gemm "):
            continue
        left, want = line.rstrip("\n").split(" | ", 1)
        a = [int(v) for v in left.split()[1:]]
        if a[1] != 1 or a[12] != 1:
            continue
        a[6] |= W4
        buf = C.create_string_buffer(8192)
        rc = lib.univst_debug_gemm_plan(*a, buf, 8192)
        assert buf.value.decode() == want and (rc == 0) == (" grid=" in want), (left, buf.value.decode())
        n += 1
        patch += want.startswith("conv_patch_kernel")
    assert n >= 8 and patch >= 3


def test_ineligible_problems_keep_todays_line(lib):
    cases = [
        (6, 1280, 1280, 8, 8, GRAPH),               # a frame-shard rank: split-K
        (12, 640, 1280, 16, 16, GRAPH),             # few tiles, long reduction: split-K
        (48, 320, 64, 24, 24, GRAPH),               # source width 24: 16-pixel fragments would straddle source rows
        (48, 640, 640, 32, 32, GRAPH | RES),        # a residual indexes output rows
        (48, 640, 640, 32, 32, GRAPH | ROWBIAS),
        (48, 640, 320, 32, 32, BIAS | W32 | WORKSPACE),      # C2 below: virtual concat
    ]
    for imgs, N, C1, Hs, Ws, flags in cases:
        rc0, without = conv_line(lib, imgs, N, C1, Hs, Ws, flags)
        rc1, with_w4 = conv_line(lib, imgs, N, C1, Hs, Ws, flags | W4)
        assert (rc0, without) == (rc1, with_w4), (imgs, N, C1, Hs, Ws, flags)
    rc0, without = conv_line(lib, 48, 640, 320, 32, 32, BIAS | W32 | WORKSPACE, C2=320)
    rc1, with_w4 = conv_line(lib, 48, 640, 320, 32, 32, BIAS | W32 | WORKSPACE | W4, C2=320)
    assert rc0 == 0 and (rc0, without) == (rc1, with_w4)
    assert "splits=1" not in conv_line(lib, 6, 1280, 1280, 8, 8, GRAPH | W4)[1]


def test_only_the_phase_copy(lib):
    """no plain weight copy (UNIVST_PLAN_W32_ONLY clears it): an eligible problem plans on the LDS-patch kernel in either form, a problem that kernel does
    not take is an error — never another kernel, which would have no weights"""
    rc, line = conv_line(lib, 48, 320, 64, 16, 16, BIAS | W32_ONLY | W4)
    assert rc == 0 and line.startswith("conv_patch_kernel<3> grid=256 ")
    rc, line = conv_line(lib, 48, 320, 64, 16, 24, BIAS | W32_ONLY | W4)
    assert rc == 0 and line.startswith("conv_patch_kernel")       # 9-tap form through the [Cin/32][9][32] copy: the width 24 is not phase-eligible
    rc, line = conv_line(lib, 6, 320, 64, 16, 16, BIAS | W32_ONLY | W4)
    assert rc != 0 and "not eligible" in line
