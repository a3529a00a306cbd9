"""The scratch layout of the registration's moments (nr_moments_layout of csrc/nfl_geom_layout.h) under AddressSanitizer +
UBSan, as tests/test_meshdist_layout_sanitizer_cpu.py does for the mesh distance's: host arithmetic that turns a size into
device pointers, walked by a stand-alone program (tests/register_layout_sweep.cpp) over a sweep of sizes against a host buffer
of exactly the queried size.  Nothing is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_register_layout_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "register_layout_sweep")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "register_layout_sweep.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "layout invariant broken" not in r.stdout and "ERROR" not in r.stderr
    assert int(r.stdout.split("layouts ok")[1].split()[0]) == 16 + 2          # 16 sizes and 2 big ones
