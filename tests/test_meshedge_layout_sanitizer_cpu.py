"""The three scratch layouts of the mesh edges (ne_layout, nl_layout, nf_layout of csrc/nfl_geom_layout.h) under
AddressSanitizer + UBSan, as tests/test_meshsmooth_layout_sanitizer_cpu.py does for the smoothing's: host arithmetic that
turns sizes into device pointers, walked by a stand-alone program (tests/meshedge_layout_sweep.cpp) over a sweep of sizes --
0 and 1, the wave, the tile boundaries of the scan, the int32 limits -- against a host buffer of exactly the queried size.
The header itself must still build as plain C++ under -Wall -Werror."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_edge_layouts_are_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "meshedge_layout_sweep")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "meshedge_layout_sweep.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "layout invariant broken" not in r.stdout and "ERROR" not in r.stderr
    # 12 sizes x (12 edges + 1 loops + 1 fill) + 4 big ones
    assert int(r.stdout.split("layouts ok")[1].split()[0]) == 12 * 14 + 4
