#!/usr/bin/env python3
"""What casting rays against a mesh costs on one MI355X (nerf_fl_amd.raycast).  Not a test: prints one
JSON record (and writes it to --out).

    The workload: the surface of `0.6 - |p|` on 256^3 (time_mesh.py's ball, about 660 k triangles) with its default grid.
    frame       cast_rays for the 640 000 rays of an 800 x 800 frame looking at the ball: grid mode, first hit and any hit, as
                ms and rays/s; beside them mesh_visibility for the same camera, for scale (a raster: it answers pixel centres)
    brute       brute mode against the first 4096 triangles only, for scale
    occlusion   vertex_occlusion of every vertex at 64 rays
    incoherent  10^6 rays from random surface samples in random directions: neighbouring lanes walk unrelated cells

Device events, 2 warm-up calls, the median of 10.  Every step runs in a child process of its own under its own time limit
(--limit seconds), so a step that hangs ends there and the others still report.  Beside the grid times stand their
yardsticks, the cells read and the ray-triangle tests made per ray.  Those are counted by a diagnostic build of the kernel,
    make -C nerf_fl_amd/csrc variant VNAME=_mccount VFLAGS=-DNFL_MESHCAST_COUNT_TESTS=1 VTU=nfl_meshcast
when libnerf_fl_amd_mccount.so lies beside the library (the shipped kernel counts nothing)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
from geom_timing import timed  # noqa: E402
from time_meshdist import ball  # noqa: E402

STEPS = ("frame", "brute", "occlusion", "incoherent")


def counted(rays, grid, mode):
    """(tests, cells, rays walked) of one nfl_mesh_cast call on the diagnostic build, or None without that build."""
    from nerf_fl_amd import _lib, raycast
    from nerf_fl_amd.geometry._call import _ptr
    path = os.path.join(ROOT, "nerf_fl_amd", "libnerf_fl_amd_mccount.so")
    if not os.path.exists(path):
        return None
    h = C.CDLL(path)
    by_name = {s[0]: s for s in _lib.SYMBOLS}
    h.nfl_mesh_cast.restype, h.nfl_mesh_cast.argtypes = by_name["nfl_mesh_cast"][1], by_name["nfl_mesh_cast"][2]
    out = (C.c_uint64 * 3)()
    t = torch.empty(rays.shape[0], device=rays.device)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    args = raycast._grid_args(grid.vertices, grid.triangles, grid, True)
    if h.nfl_meshcast_debug_counts(None, 1) or h.nfl_mesh_cast(_ptr(rays), rays.shape[0], *args, mode, _ptr(t), None, None, None, stream):
        return None
    torch.cuda.synchronize()
    return None if h.nfl_meshcast_debug_counts(out, 0) else list(out)


def _per_ray(rec, key, counts, ms):
    if counts is not None:
        tests, cells, n = counts
        rec[key + "_tests_per_ray"], rec[key + "_cells_per_ray"] = tests / max(n, 1), cells / max(n, 1)
        rec[key + "_tests_per_s"] = tests / ms["median"] * 1e3


def step(name, a):
    from nerf_fl_amd import eval as nfl_eval, geometry, meshdist, raycast
    dev = torch.device("cuda:0")
    mesh = ball(a.points, dev)
    grid = meshdist.triangle_grid(mesh)
    T, V = mesh["triangles"].shape[0], mesh["vertices"].shape[0]
    rec = {"triangles": T, "vertices": V, "cell": grid.cell, "dims": grid.dims, "entries": grid.entries.shape[0]}
    c2w = torch.eye(4)[:3].clone()
    c2w[2, 3] = 2.0                                                     # at (0, 0, 2), looking down -z at the ball
    K = nfl_eval.fov60_intrinsics(a.width, a.width)
    rate = lambda n, ms: n / ms["median"] * 1e3
    if name == "frame":
        rays = nfl_eval.frame_rays(c2w, K, a.width, a.width, 0.0, 10.0, dev)
        R = rays.shape[0]
        for mode in ("first", "any"):
            ms = timed(lambda: raycast.cast_rays(rays, grid, mode=mode), a.warmup, a.iters)
            rec.update({mode + "_ms": ms, mode + "_rays_per_s": rate(R, ms)})
            _per_ray(rec, mode, counted(rays, grid, 0 if mode == "first" else 1), ms)
        got = raycast.cast_rays(rays, grid)
        rec.update(rays=R, hit_share=float(torch.isfinite(got["t"]).float().mean().item()))
        c2w_d, K_d = c2w.to(dev), K.to(dev)
        ms = timed(lambda: geometry.mesh_visibility(mesh, c2w_d, K_d, a.width, a.width), a.warmup, a.iters)
        rec.update(mesh_visibility_ms=ms, mesh_visibility_pixels_per_s=rate(R, ms))
    elif name == "brute":
        rays = nfl_eval.frame_rays(c2w, K, a.width, a.width, 0.0, 10.0, dev)
        few = dict(mesh, triangles=mesh["triangles"][:a.brute].contiguous())
        ms = timed(lambda: raycast.cast_rays(rays, few, method="brute"), 1, max(a.iters // 4, 2))
        rec.update(rays=rays.shape[0], brute_triangles=a.brute, ms=ms, rays_per_s=rate(rays.shape[0], ms),
                   tests_per_s=rays.shape[0] * a.brute / ms["median"] * 1e3)
    elif name == "occlusion":
        ms = timed(lambda: raycast.vertex_occlusion(mesh, rays=64, grid=grid), a.warmup, a.iters)
        opn = raycast.vertex_occlusion(mesh, rays=64, grid=grid)
        rec.update(rays=64 * V, ms=ms, rays_per_s=rate(64 * V, ms), mean_open=float(opn.mean().item()))
    else:
        s = meshdist.sample_surface(mesh, n=a.samples, seed=1)
        g = torch.Generator(device=dev).manual_seed(2)
        d = torch.randn(s["points"].shape[0], 3, device=dev, generator=g)
        N = d.shape[0]
        rays = torch.cat([s["points"] + 1e-4 * s["normals"], d, torch.zeros(N, 1, device=dev), torch.full((N, 1), np.inf, device=dev)], 1).contiguous()
        for mode in ("first", "any"):
            ms = timed(lambda: raycast.cast_rays(rays, grid, mode=mode), a.warmup, a.iters)
            rec.update({mode + "_ms": ms, mode + "_rays_per_s": rate(N, ms)})
            _per_ray(rec, mode, counted(rays, grid, 0 if mode == "first" else 1), ms)
        rec.update(rays=N, hit_share=float(torch.isfinite(raycast.cast_rays(rays, grid)["t"]).float().mean().item()))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=256, help="lattice of the ball")
    ap.add_argument("--width", type=int, default=800, help="the frame is width x width")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--brute", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_raycast.py measures on the GPU; there is none here")
    if a.step:
        print(json.dumps(step(a.step, a)))
        return
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters}
    for name in STEPS:                                                  # a fresh child per step, each under its own limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [f"--{k}={getattr(a, k)}" for k in
                                                                              ("points", "width", "samples", "brute", "warmup", "iters")]
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
