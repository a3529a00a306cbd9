#!/usr/bin/env python3
"""What telling the inside of a mesh from the outside costs on one MI355X (nerf_fl_amd.solid).  Not a
test: prints one JSON record (and writes it to --out).

    The workload: the surface of `0.6 - |p|` on 256^3 (time_mesh.py's ball, about 660 k triangles) with its default grid.
    inside      inside_mesh at the 128^3 lattice points over [-1, 1]^3, with 1 and with 3 directions, as ms and points/s
    lattice     solid_lattice at 128^3: the grid, the closest point within trunc, and the sides
    crossings   count_crossings for the 640 000 rays of time_raycast.py's 800 x 800 frame, to set beside its first-hit time

Device events, 2 warm-up calls, the median of 10.  Every step runs in a child process of its own under its own time limit
(--limit seconds), so a step that hangs ends there and the others still report."""
import argparse
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
from geom_timing import timed  # noqa: E402
from time_meshdist import ball  # noqa: E402

STEPS = ("inside", "lattice", "crossings")
CUBE = ((-1.0,) * 3, (1.0,) * 3)


def step(name, a):
    from nerf_fl_amd import eval as nfl_eval, geometry, meshdist, raycast, solid
    dev = torch.device("cuda:0")
    mesh = ball(a.points, dev)
    grid = meshdist.triangle_grid(mesh)
    rec = {"triangles": mesh["triangles"].shape[0], "cell": grid.cell, "dims": grid.dims, "entries": grid.entries.shape[0]}
    res = (a.lattice,) * 3
    rate = lambda n, ms: n / ms["median"] * 1e3
    if name == "inside":
        pts = geometry.lattice_points(*CUBE, res, dev).reshape(-1, 3)
        for K in (1, 3):
            ms = timed(lambda: solid.inside_mesh(pts, grid, directions=K), a.warmup, a.iters)
            rec.update({f"k{K}_ms": ms, f"k{K}_points_per_s": rate(pts.shape[0], ms)})
        got = solid.inside_mesh(pts, grid)
        rec.update(points=pts.shape[0], inside_share=float(got["inside"].float().mean().item()),
                   split_votes=int(((got["votes"] != 0) & (got["votes"] != 3)).sum().item()))
    elif name == "lattice":
        ms = timed(lambda: solid.solid_lattice(mesh, *CUBE, res), a.warmup, a.iters)
        rec.update(points=a.lattice ** 3, ms=ms, points_per_s=rate(a.lattice ** 3, ms))
    else:
        c2w = torch.eye(4)[:3].clone()
        c2w[2, 3] = 2.0                                                 # at (0, 0, 2), looking down -z at the ball
        K = nfl_eval.fov60_intrinsics(a.width, a.width)
        rays = nfl_eval.frame_rays(c2w, K, a.width, a.width, 0.0, 10.0, dev)
        ms = timed(lambda: solid.count_crossings(rays, grid), a.warmup, a.iters)
        first = timed(lambda: raycast.cast_rays(rays, grid), a.warmup, a.iters)
        count = solid.count_crossings(rays, grid)
        rec.update(rays=rays.shape[0], ms=ms, rays_per_s=rate(rays.shape[0], ms), first_hit_ms=first,
                   twice_share=float((count == 2).float().mean().item()), odd=int((count % 2 == 1).sum().item()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=256, help="lattice of the ball")
    ap.add_argument("--lattice", type=int, default=128, help="the queries are the lattice^3 points over [-1, 1]^3")
    ap.add_argument("--width", type=int, default=800, help="the frame is width x width")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_solid.py measures on the GPU; there is none here")
    if a.step:
        print(json.dumps(step(a.step, a)))
        return
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters}
    for name in STEPS:                                                  # a fresh child per step, each under its own limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [f"--{k}={getattr(a, k)}" for k in
                                                                              ("points", "lattice", "width", "warmup", "iters")]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.limit)
        except subprocess.TimeoutExpired:
            rec[name] = {"failed": f"no result within {a.limit} s"}
            break                                                       # nothing more is started on a device that hung
        if r.returncode != 0:
            rec[name] = {"failed": r.returncode, "stderr": r.stderr[-400:]}
            break
        rec[name] = json.loads(r.stdout.strip().splitlines()[-1])
    text = json.dumps(rec)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
