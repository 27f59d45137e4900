"""The activation arena (csrc/model.h Arena) is plain host code: tools/arena_check.cpp walks it through a few hundred mixed alloc / release /
reset steps (no overlap, neighbours coalesce, high_water is the largest end offset, exhaustion returns null).  Built here as a stand-alone
program with AddressSanitizer + UBSan on the host side and run on the CPU; it opens no GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_arena_check_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "arena_check")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-std=c++17", f"-I{ROOT}/include", "-Xarch_host", "-fsanitize=address,undefined",
                    "-Xarch_host", "-fno-sanitize-recover=all", f"{ROOT}/tools/arena_check.cpp", f"{ROOT}/univst_amd/csrc/model.hip", "-o", exe],
                   check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, cwd=str(tmp_path))
    assert r.returncode == 0 and "arena_check: ok" in r.stdout, r.stdout + r.stderr
