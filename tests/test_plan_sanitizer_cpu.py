"""The host-side plan builder under AddressSanitizer + UBSan (GPU sanitizers are not available on this pool; the host code is
where fixed-size tables are filled by configuration-dependent loops): tests/plan_sweep.cpp builds forward and backward plans
for every encoder / latent width combination, accepted or rejected, and for every accepted one the weight-gradient job list
(csrc/nfl_wgrad_plan.cpp) and its launch schedule over segment counts, CU counts and both stash multipliers, and the host side
of the render and dgrad launchers (csrc/nfl_launch.cpp): ray split, argument-block fills, the entry points' refusals; and the
task lists of the composition through xyz_encoding_final (csrc/nfl_compose.cpp), evaluated on exactly-sized heap blocks by a
reference interpreter that lives in the sweep, with the refusals of nfl_mlp_wgrad (nfl_wgrad_check)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_plan_builder_is_clean_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "plan_sweep")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-fno-omit-frame-pointer", os.path.join(ROOT, "tests", "plan_sweep.cpp"),
           os.path.join(ROOT, "nerf_fl_amd", "csrc", "nfl_plan.cpp"),
           os.path.join(ROOT, "nerf_fl_amd", "csrc", "nfl_wgrad_plan.cpp"),
           os.path.join(ROOT, "nerf_fl_amd", "csrc", "nfl_launch.cpp"),
           os.path.join(ROOT, "nerf_fl_amd", "csrc", "nfl_compose.cpp"), "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if b.returncode != 0 and "sanitize" in b.stderr and "cannot find" in b.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert "plans ok" in r.stdout and "ERROR" not in r.stderr
    n_ok = int(r.stdout.split("plans ok")[1].split()[0])
    assert n_ok > 10000
    # every accepted field (11520 of the swept descriptors x transient on / off) got a wgrad plan, each scheduled 72 times
    print(r.stdout)
    assert "wgrad invariant broken" not in r.stdout
    n_wplans, n_sched = (int(r.stdout.split(k)[1].split()[0]) for k in ("wgrad plans", "schedules"))
    assert n_wplans > 10000 and n_sched == 72 * n_wplans
    assert "wgrad rows reached" in r.stdout
    # the launchers' host side: 13 x 4 x 9 x 2 ray splits once; per accepted field its argument-block fills and the refusal table
    assert "launch invariant broken" not in r.stdout
    n_splits, n_fills, n_refusals = (int(r.stdout.split(k)[1].split()[0]) for k in ("launch splits", "fills", "refusals"))
    assert n_splits == 936 and n_fills > 20 * n_wplans // 2 and n_refusals > 80 * n_wplans // 2
    # the composition through xyz_encoding_final: the sweep's accepted fields have 24 side widths of dir_encoding.0 (4 direction
    # encoders, alone or with one of 5 appearance widths) and no transient layers or 3 code widths: 24 x 4 forward folds; the
    # gradient composition per shape and plan (no transient layers 24, transient layers unused 72, used 72) x the 16 subsets
    # of the four composed gradients; the refusal rows of nfl_wgrad_check and the two builders once; nfl_wgrad_fill per plan
    assert "compose invariant broken" not in r.stdout
    n_fwd, n_bwd, n_rows, n_wfills = (int(r.stdout.split(k)[1].split()[0])
                                      for k in ("compose forward cases", "backward cases", "refusal rows", "wgrad fills"))
    assert n_fwd == 96 and n_bwd == 168 * 16 and n_rows == 75 and n_wfills == n_wplans
