"""CPU: kernel selection of the GEMM / conv launcher and of the attention launcher, read out through the host-only entries
univst_debug_gemm_plan / univst_debug_attention_plan (uv_gemm_plan / uv_attention_plan in csrc/gemm.hip, csrc/attention.hip).

 - the recorded table tests/data/dispatch_plan.txt: what the launchers launched for the shapes the project runs BEFORE the plan functions
   existed (recorded from that commit), row for row; every kernel of the two launch tables is produced by at least one row;
 - the predicates the UNet graph acts on never promise a path the plan then refuses;
 - the plan errors the GPU tests provoke come out of the debug entries with the same text."""
import ctypes as C
import itertools
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "data", "dispatch_plan.txt")
NCU = 256
BIAS, RES, ROWBIAS, LN_STATS, STATS_OUT, ACT, GATE, W32_ONLY, W32, GN_OUT, TAPINNER, Y_UNALIGNED, WORKSPACE, W4, LDY_ODD = (1 << i for i in range(15))


@pytest.fixture(scope="module")
def lib():
    from univst_amd import _native
    if not os.path.exists(_native.lib_path()):
        import __graft_entry__
        __graft_entry__.build()
    return _native.load()


def _call(fn, args, n=8192):
    buf = C.create_string_buffer(n)
    rc = fn(*args, buf, n)
    return rc, buf.value.decode()


def gemm_line(lib, M, N, K, geglu=0, flags=0, sets=0, ncu=NCU):
    return _call(lib.univst_debug_gemm_plan, (ncu, 0, M, N, K, geglu, flags, sets, 0, 0, 0, 0, 0, 1, 1, 0))


def _rows():
    for line in open(TABLE):
        if line.strip() and not line.startswith("#"):
            left, want = line.rstrip("\n").split(" | ", 1)
            kind, *args = left.split()
            yield kind, tuple(int(a) for a in args), want


def test_flag_values_match_the_header():
    src = open(os.path.join(ROOT, "include", "univst.h")).read()
    got = {k: int(v) for k, v in re.findall(r"#define UNIVST_PLAN_([A-Z0-9_]+) (\d+)", src)}
    want = dict(BIAS=BIAS, RESIDUAL=RES, ROWBIAS=ROWBIAS, LN_STATS=LN_STATS, STATS_OUT=STATS_OUT, ACT=ACT, GATE=GATE, W32_ONLY=W32_ONLY, W32=W32, GN_OUT=GN_OUT,
                TAPINNER=TAPINNER, Y_UNALIGNED=Y_UNALIGNED, WORKSPACE=WORKSPACE, W4=W4, LDY_ODD=LDY_ODD)
    assert {k: got.get(k) for k in want} == want


def test_recorded_table(lib):
    """every row gives the recorded line, and the rows reach every kernel of the two launch tables (set equality: an instantiation that no row
    produces, or a symbol that is in no table, fails)"""
    produced, wrong, n = set(), [], 0
    for kind, args, want in _rows():
        rc, got = _call(lib.univst_debug_gemm_plan if kind == "gemm" else lib.univst_debug_attention_plan, args)
        n += 1
        if got != want or (rc == 0) != (" grid=" in want):
            wrong.append((kind, args, want, got, rc))
        if rc == 0:
            produced.add(got.split(" ")[0])
    assert not wrong, f"{len(wrong)} of {n} rows differ, first: {wrong[:3]}"
    assert n > 1000
    table = set(_call(lib.univst_debug_gemm_plan, (NCU,) + (0,) * 15)[1].split(";")) | set(_call(lib.univst_debug_attention_plan, (0,) * 9)[1].split(";"))
    assert len(table) == 23 + 61
    assert produced == table, f"never produced: {sorted(table - produced)}; in no launch table: {sorted(produced - table)}"


MS = sorted({64 << i for i in range(12)} | {196608, 98304, 49152, 24576, 12288, 6144, 3072, 1536, 384, 231, 333, 15984})
WIDTHS = (320, 640, 960, 1280, 2560, 3840, 5120, 10240, 1536, 4608, 6144, 768, 128, 256, 512)
NEAR = sorted({w + d for w in WIDTHS for d in (0, 8, -8, 160, -160) if w + d > 0})


def test_predicates_never_promise_what_the_plan_refuses(lib):
    """sweep M x N x K: whenever a predicate says yes, the plan of that feature has no error and takes the promised path — a direct 256x320
    kernel for takes_big_direct (here: weight sets, which exist nowhere else); splits=1 on a statistics-capable instantiation for the LayerNorm
    producer / consumer / GEGLU consumer; the X-resident kernel for geglu_xres.  No (predicate-true, plan-error) pair may exist."""
    # (the LayerNorm statistics come in 160-column slots: a consumer has K % 160 == 0 by the contract of univst_linear_ln, whatever path it takes)
    bad, yes = [], [0] * 5
    for M, N, K in itertools.product(MS, NEAR, NEAR):
        rc, line = gemm_line(lib, M, N, K, flags=BIAS)
        if rc != 0:
            continue            # (K % 8 != 0 and the like: every predicate is then a statement about a problem that cannot be launched at all)
        pred = [int(v) for v in re.search(r"big_direct=(\d) fold_producer=(\d) fold_consumer=(\d) geglu_consumer=(\d) geglu_xres=(\d)", line).groups()]
        checks = []
        if pred[0] and (M % 256 == 0 or M % 192 == 0):
            checks.append(("big_direct", gemm_line(lib, M, N, K, flags=RES, sets=M), r"gemm_big_kernel<0,[34],0> .* splits=1 "))
        if pred[1]:
            checks.append(("fold_producer", gemm_line(lib, M, N, K, flags=BIAS | RES | STATS_OUT), r"(gemm_big_kernel<0,[34],1>|gemm_kernel<5,0,4,1>) .* splits=1 "))
        if pred[2] and K % 160 == 0:
            checks.append(("fold_consumer", gemm_line(lib, M, N, K, flags=LN_STATS), r"(gemm_big_kernel<0,[34],2>|gemm_kernel<[45],0,[24],2>) .* splits=1 "))
        if pred[3] and K % 160 == 0:
            checks.append(("geglu_consumer", gemm_line(lib, M, N, K, geglu=1, flags=LN_STATS), r"gemm_big_kernel<0,[34],2> .* splits=1 "))
        if pred[4]:
            checks.append(("geglu_xres", gemm_line(lib, M, N, K, geglu=2, flags=LN_STATS), r"geglu_xres_kernel<2> .* splits=1 "))
            checks.append(("geglu_xres", gemm_line(lib, M, N, K, geglu=2, flags=BIAS), r"geglu_xres_kernel<0> .* splits=1 "))
        for i, p in enumerate(pred):
            yes[i] += p
        for name, (rc2, got), pattern in checks:
            if rc2 != 0 or not re.match(pattern, got) or "+splitk_reduce" in got:
                bad.append((name, M, N, K, rc2, got))
    assert not bad, f"{len(bad)} broken promises, first: {bad[:3]}"
    assert all(y > 0 for y in yes), yes            # the sweep reaches a yes of every predicate


def test_plan_errors_read_like_the_launchers(lib):
    """the plan errors the GPU tests provoke through _native.check (test_gpu_ops.py: test_linear_geglu_x_resident_rejects_other_shapes,
    test_conv3x3_lds_patch_rejects_ineligible) — same text from the debug entry, and last_error holds it too"""
    rc, msg = gemm_line(lib, 512, 2560, 640, geglu=2)
    assert rc == -1 and msg == ("geglu (X-resident order): needs K = 320, N % 256 == 0, 16-byte aligned rows, no residual / second bias (M=512 N=2560 K=640)")
    assert lib.univst_last_error().decode() == msg
    rc, msg = _call(lib.univst_debug_gemm_plan, (NCU, 1, 6, 320, 0, 0, W32_ONLY, 0, 32, 0, 4, 4, 0, 1, 9, 0))
    assert rc == -1 and msg.startswith("conv: only the [Cin/32][9][32] weight copy was given but the problem is not eligible for the LDS-patch kernel")
    rc, msg = _call(lib.univst_debug_attention_plan, (2, 8, 256, 256, 3, 48, 0, 0, 0))
    assert rc == -3 and msg == "attention: head_dim=48 not instantiated (16,32,40,64,80,160)"
    rc, msg = gemm_line(lib, 0, 320, 320)
    assert rc == -1 and msg == "gemm: empty problem M=0 N=320 K=320"
