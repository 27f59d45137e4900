"""CPU: the option table of the UNet handle (abi.hip kUNetOptions).  univst_unet_create touches no device, so defaults, accepted ranges, environment
seeds and the read-back through univst_unet_query are all checked without a GPU."""
import ctypes as C
import os
import re

import pytest

from univst_amd import _native

ARG = -1
# name -> (default, lowest accepted, highest accepted); None: a 0 / 1 switch that takes any int as != 0
OPTIONS = {"ln_fold": (2, 0, 2), "gn_producer": (1, None, None), "chain_bands": (1, 0, 64), "gn_fold": (1, None, None), "attn2_fused": (2, 0, 2),
           "kv_overlap": (1, None, None), "emu_wire_gbps": (0, 0, 10000), "emu_wire_lat_us": (3, 0, 100000), "kcat_fold": (3, 0, 3)}
SEEDS = [("UNIVST_LN_FOLD", "7", "ln_fold", 2), ("UNIVST_LN_FOLD", "-1", "ln_fold", 0), ("UNIVST_KCAT_FOLD", "9", "kcat_fold", 3),
         ("UNIVST_ATTN2_PRE", "0", "attn2_fused", 1), ("UNIVST_ATTN2_PRE", "1", "attn2_fused", 2), ("UNIVST_CHAIN_BANDS", "100", "chain_bands", 100),
         ("UNIVST_CHAIN_BANDS", "-5", "chain_bands", 0), ("UNIVST_GN_PRODUCER", "0", "gn_producer", 0), ("UNIVST_GN_FOLD", "0", "gn_fold", 0),
         ("UNIVST_KV_OVERLAP", "0", "kv_overlap", 0)]
ENV_NAMES = sorted({s[0] for s in SEEDS})


def _cfg():
    return _native.UnetCfg(4, 4, (C.c_int * 4)(320, 640, 1280, 1280), 2, 768, (C.c_int * 4)(8, 8, 8, 8), 32, 1e-5, 1, 0.0)


@pytest.fixture
def lib(monkeypatch):
    for n in ENV_NAMES:      # the defaults are what a handle has without seeds
        monkeypatch.delenv(n, raising=False)
    return _native.load()


@pytest.fixture
def handle(lib):
    h, cfg = C.c_void_p(), _cfg()
    assert lib.univst_unet_create(C.byref(cfg), C.byref(h)) == 0, lib.univst_last_error().decode()
    yield h
    lib.univst_unet_destroy(h)


@pytest.fixture
def ad_handle(lib):
    h, cfg = C.c_void_p(), _cfg()
    ad = _native.AnimateDiffCfg(1, 15, 1, _native.MotionCfg(0, 8, 1, 2, 32, 24, 1, 1e-6, 1e-5))
    assert lib.univst_unet_create_animatediff(C.byref(cfg), C.byref(ad), C.byref(h)) == 0, lib.univst_last_error().decode()
    yield h
    lib.univst_unet_destroy(h)


def query(lib, h, name):
    out = C.c_double(-7)
    rc = lib.univst_unet_query(h, name.encode(), C.byref(out))
    return rc, out.value


def test_the_table_has_the_options_the_header_lists():
    """the option list of include/univst.h: a comment block of lines ' *   "name" (default ...' in front of univst_unet_set_option"""
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "univst.h")).read()
    block = text[text.index("/* tuning switches of a handle"):text.index("int univst_unet_set_option")]
    listed = set()
    for line in re.findall(r'^ \*   ("[^(]*)\(', block, flags=re.M):
        listed.update(re.findall(r'"(\w+)"', line))
    assert listed == set(OPTIONS)


@pytest.mark.parametrize("name", sorted(OPTIONS))
def test_default_range_and_read_back(lib, handle, name):
    default, lo, hi = OPTIONS[name]
    assert query(lib, handle, name) == (0, default)
    if lo is None:
        for v, want in ((0, 0), (1, 1), (-3, 1), (17, 1), (0, 0)):
            assert lib.univst_unet_set_option(handle, name.encode(), v) == 0
            assert query(lib, handle, name) == (0, want)
        return
    for v in range(lo, hi + 1):
        assert lib.univst_unet_set_option(handle, name.encode(), v) == 0, (name, v)
        assert query(lib, handle, name) == (0, v)
    for bad in (lo - 1, hi + 1):
        assert lib.univst_unet_set_option(handle, name.encode(), bad) == ARG, (name, bad)
        assert name in lib.univst_last_error().decode()
        assert query(lib, handle, name) == (0, hi), "a refused value leaves the option as it was"


@pytest.mark.parametrize("env,value,name,want", SEEDS)
def test_environment_seed(lib, monkeypatch, env, value, name, want):
    monkeypatch.setenv(env, value)
    h, cfg = C.c_void_p(), _cfg()
    assert lib.univst_unet_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert query(lib, h, name) == (0, want)
        for other, (default, _, _) in OPTIONS.items():
            if other != name:
                assert query(lib, h, other) == (0, default), "a seed moves its own option only"
    finally:
        lib.univst_unet_destroy(h)


def test_the_wire_emulation_has_no_seed(lib, monkeypatch):
    for env in ("UNIVST_EMU_WIRE_GBPS", "UNIVST_EMU_WIRE_LAT_US"):
        monkeypatch.setenv(env, "50")
    h, cfg = C.c_void_p(), _cfg()
    assert lib.univst_unet_create(C.byref(cfg), C.byref(h)) == 0
    try:
        assert query(lib, h, "emu_wire_gbps") == (0, 0) and query(lib, h, "emu_wire_lat_us") == (0, 3)
    finally:
        lib.univst_unet_destroy(h)


def test_unknown_names_and_motion_fold(lib, handle, ad_handle):
    assert lib.univst_unet_set_option(handle, b"no_such_option", 1) == ARG and "no_such_option" in lib.univst_last_error().decode()
    rc, v = query(lib, handle, "no_such_option")
    assert rc == ARG and v == -7 and "no_such_option" in lib.univst_last_error().decode()
    assert query(lib, handle, "motion_fold")[0] == ARG, "the SD handle has no such option"
    assert lib.univst_unet_set_option(handle, b"motion_fold", 0) == ARG
    assert query(lib, ad_handle, "motion_fold") == (0, 0)
    assert lib.univst_unet_set_option(ad_handle, b"motion_fold", 1) == -3 and query(lib, ad_handle, "motion_fold") == (0, 0)
    for name, (default, _, _) in OPTIONS.items():
        assert query(lib, ad_handle, name) == (0, default), "the AnimateDiff handle has the SD handle's options too"
