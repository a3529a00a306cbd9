#!/usr/bin/env python3
"""What one iteration of the registration costs on one MI355X (nerf_fl_amd.registration).  Not a test:
prints one JSON record (and writes it to --out).  Nothing is asserted: there is no earlier time to compare against.

    The workload is time_meshdist.py's: the surface of `0.6 - |p|` on 256^3 (about 660 k triangles) as the target, and about
    10^5 and 10^6 samples of the same ball extracted on 200^3 as the source (--second-radius 0.58 puts them four triangle
    extents OFF the target, where the closest-point query is slow).  A ball is used for TIMING ONLY: a rotation of it is not
    observable, so plane mode's system is singular here but for the facets; the status its solve ends with is recorded beside
    its time, and the point-mode solve (always solvable) is timed as well.
    Per sample count: apply, closest (grid mode), moments (both modes), solve (both modes), each alone between device events,
    median of --iters; the sum of apply + moments + solve against closest; the bytes moments reads per pair (12 P, 12 Q,
    4 triangle, 4 distance, 12 indices, 36 corners = 80) and the rate that makes; and register_mesh itself, 10 iterations
    on the host's clock, the one read at the end included.

Every sample count runs in a child process of its own under its own time limit (--limit seconds), so a step that hangs ends
there and nothing more is started on the device."""
import argparse
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
from geom_timing import host_timed, timed  # noqa: E402
from time_meshdist import ball  # noqa: E402

BYTES_PER_PAIR = 12 + 12 + 4 + 4 + 12 + 36


def step(samples, a):
    from nerf_fl_amd import _lib, meshdist, registration as reg
    dev = torch.device("cuda:0")
    target, source = ball(a.points, dev), ball(a.second, dev, a.second_radius)
    grid = meshdist.triangle_grid(target)
    src = meshdist.sample_surface(source, n=samples, seed=1)["points"]
    N = src.shape[0]
    rec = {"triangles": target["triangles"].shape[0], "pairs": N, "grid": grid.dims}
    T13 = reg._identity(dev)
    moved = torch.empty_like(src)
    row = torch.empty(_lib.REGISTER_ROW["COLUMNS"], dtype=torch.float64, device=dev)
    history = torch.empty(_lib.REGISTER_HISTORY, dtype=torch.float64, device=dev)
    scratch = reg._scratch(_lib.lib().nfl_register_bytes(N), dev)
    centre = [0.0, 0.0, 0.0]
    t = lambda fn: timed(fn, a.warmup, a.iters)
    rec["apply_ms"] = t(lambda: reg._apply(src, moved, T13, False))
    got = meshdist.closest_on_mesh(moved, grid)
    rec["closest_ms"] = t(lambda: meshdist.closest_on_mesh(moved, grid))
    for name, code in _lib.REGISTER_MODES.items():
        moments = lambda: reg._moments(moved, got["point"], got["triangle"], got["distance"], grid.vertices, grid.triangles, code,
                                       float("inf"), centre, scratch, row)
        rec[f"moments_{name}_ms"] = t(moments)
        moments()
        fresh = T13.clone()
        rec[f"solve_{name}_ms"] = t(lambda: reg._solve(row, code, True, 6, centre, fresh, history, 0))
        rec[f"solve_{name}_status"] = int(history.cpu()[2])
    rec["moments_bytes_per_pair"] = BYTES_PER_PAIR
    rec["moments_plane_GBps"] = BYTES_PER_PAIR * N / rec["moments_plane_ms"]["median"] * 1e-6
    rec["around_closest_ms"] = rec["apply_ms"]["median"] + rec["moments_plane_ms"]["median"] + rec["solve_plane_ms"]["median"]
    rec["mean_distance"] = float(got["distance"].double().mean().cpu())
    run = lambda: reg.register_mesh(source, grid, mode="point", iterations=10, n=samples, seed=1)
    rec["register_mesh_point_10_iterations_ms_host_clock"] = host_timed(run, 1, max(a.iters // 3, 2))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=256, help="lattice of the target mesh")
    ap.add_argument("--second", type=int, default=200, help="lattice of the mesh that is sampled")
    ap.add_argument("--second-radius", "--second_radius", dest="second_radius", type=float, default=0.6,
                    help="radius of the sampled ball: 0.6 puts the points ON the target, another radius that far off it")
    ap.add_argument("--samples", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", type=int, default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_registration.py measures on the GPU; there is none here")
    if a.step is not None:
        print(json.dumps(step(a.step, a)))
        return
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "second_radius": a.second_radius}
    for samples in a.samples:                                           # a fresh child per step, each under its own limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", str(samples)] + [f"--{k}={getattr(a, k)}" for k in
                                                                                        ("points", "second", "second_radius", "warmup", "iters")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            rec[str(samples)] = {"failed": f"no result within {a.limit} s"}
            break                                                       # nothing more is started on a device that hung
        if r.returncode != 0:
            rec[str(samples)] = {"failed": r.returncode, "stderr": r.stderr[-400:]}
            break
        rec[str(samples)] = json.loads(r.stdout.strip().splitlines()[-1])
    text = json.dumps(rec)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
