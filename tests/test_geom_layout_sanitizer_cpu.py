"""The scratch layouts of the geometry entry points under AddressSanitizer + UBSan.  csrc/nfl_geom_layout.h is host
arithmetic that turns sizes into device pointers: a region that ends past the size the caller was told is a device write
out of bounds.  tests/geom_layout_sweep.cpp walks the layouts of all five entry points (surface, occupancy build, mesh
label, mesh compact, simplify) over a sweep of sizes against a host buffer of exactly nfl_*_bytes bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_geometry_layouts_are_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "geom_layout_sweep")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "geom_layout_sweep.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "layout invariant broken" not in r.stdout and "ERROR" not in r.stderr
    # 12 x 12 mesh sizes x 3 layouts + 4 big ones, 10 x 3 x 2 lattices x 2 layouts + 2 long rows
    assert int(r.stdout.split("layouts ok")[1].split()[0]) == 12 * 12 * 3 + 4 + 10 * 3 * 2 * 2 + 2
