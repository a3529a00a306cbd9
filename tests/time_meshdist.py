#!/usr/bin/env python3
"""What the mesh distance costs on one MI355X (nerf_fl_amd.meshdist).  Not a test: prints one JSON
record (and writes it to --out).

    The workload: the surface of `0.6 - |p|` on 256^3 (time_mesh.py's ball, about 10^6 triangles) as the mesh, and about 10^6
    samples of the same ball extracted on 200^3 -- another triangulation of the same sphere -- as the queries
    (--second-radius 0.58 samples a ball 0.02 inside it instead: queries some four triangle extents OFF the mesh).
    grid:F   F = 1, 2, 4 times the mean longest bounding-box side of the triangles as the cell: the grid build (count, host
             read, emit: a host clock), nfl_mesh_closest in grid mode and nfl_meshdist_reduce (device events)
    brute    nfl_mesh_closest in brute mode against the first 4096 triangles only, for scale

Every step runs in a child process of its own under its own time limit (--limit seconds), so a step that hangs ends there
and the others still report.  Beside every query time stand its yardsticks: the cells and row entries read and the
point-triangle tests made per query.  Those are counted by a diagnostic build of the kernel,
    make -C nerf_fl_amd/csrc variant VNAME=_mdcount VFLAGS=-DNFL_MESHDIST_COUNT_TESTS=1 VTU=nfl_meshdist
when libnerf_fl_amd_mdcount.so lies beside the library (the shipped kernel counts nothing); a row entry is 4 B, a cell two
8-byte offsets, a test the 36 B of three corners through 12 B of indices."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [ROOT, HERE]
from geom_timing import host_timed, timed  # noqa: E402

STEPS = ("grid:1", "grid:2", "grid:4", "brute")


def ball(n, dev, radius=0.6):
    from nerf_fl_amd import geometry
    c = torch.linspace(-1, 1, n, device=dev, dtype=torch.float64)
    lat = (radius - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()
    return geometry.extract_surface(lat, 0.0, (-1.0,) * 3, (1.0,) * 3)


def counted(a):
    """(tests, cells, queries) of one nfl_mesh_closest call on the diagnostic build, or None without that build."""
    path = os.path.join(ROOT, "nerf_fl_amd", "libnerf_fl_amd_mdcount.so")
    if not os.path.exists(path):
        return None
    h = C.CDLL(path)
    out = (C.c_uint64 * 3)()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    if h.nfl_meshdist_debug_counts(None, 1) or h.nfl_mesh_closest(C.byref(a), stream):
        return None
    torch.cuda.synchronize()
    return None if h.nfl_meshdist_debug_counts(out, 0) else list(out)


def step(name, a):
    from nerf_fl_amd import _lib, meshdist
    from nerf_fl_amd.geometry._call import _ptr
    dev = torch.device("cuda:0")
    mesh, other = ball(a.points, dev), ball(a.second, dev, a.second_radius)
    queries = meshdist.sample_surface(other, n=a.samples, seed=1)
    p, nrm = queries["points"], queries["normals"]
    N, T = p.shape[0], mesh["triangles"].shape[0]
    rec = {"triangles": T, "queries": N}
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {k: torch.empty(N, *s, dtype=d, device=dev) for k, s, d in (("distance", (), torch.float32), ("triangle", (), torch.int32),
           ("point", (3,), torch.float32), ("bary", (3,), torch.float32), ("dot", (), torch.float32))}
    q = _lib.MeshClosestArgs()
    q.d_points, q.n_points, q.d_vertices, q.n_vertices, q.max_distance = _ptr(p), N, _ptr(mesh["vertices"]), mesh["vertices"].shape[0], float("inf")
    q.d_normals, q.d_dot = _ptr(nrm), _ptr(out["dot"])
    q.d_distance, q.d_triangle, q.d_point, q.d_bary = (_ptr(out[k]) for k in ("distance", "triangle", "point", "bary"))
    closest = lambda: _lib.check(lib.nfl_mesh_closest(C.byref(q), stream()), "closest")
    if name == "brute":
        few = mesh["triangles"][:a.brute].contiguous()
        q.d_triangles, q.n_triangles = _ptr(few), few.shape[0]
        t = timed(closest, 1, max(a.iters // 4, 2))
        rec.update(brute_triangles=few.shape[0], ms=t, tests_per_query=few.shape[0], tests_per_s=N * few.shape[0] / t["median"] * 1e3)
        return rec
    factor = float(name.split(":")[1])
    extent = meshdist._mesh_box(mesh["vertices"], mesh["triangles"])[2]
    cell = factor * extent
    rec.update(factor=factor, mean_triangle_extent=extent, cell=cell)
    rec["build_ms_host_clock"] = host_timed(lambda: meshdist.triangle_grid(mesh, cell=cell), 1, a.iters)
    grid = meshdist.triangle_grid(mesh, cell=cell)
    rec.update(dims=grid.dims, entries=grid.entries.shape[0], entries_per_cell=grid.entries.shape[0] / (grid.offsets.shape[0] - 1))
    q.d_triangles, q.n_triangles = _ptr(mesh["triangles"]), T
    q.d_offsets, q.d_entries, q.n_entries = _ptr(grid.offsets), _ptr(grid.entries), grid.entries.shape[0]
    q.lo[:], q.cell, q.dims[:] = grid.lo, grid.cell, grid.dims
    rec["query_ms"] = timed(closest, a.warmup, a.iters)
    rec["reduce_ms"] = timed(lambda: meshdist._reduce(out["distance"], out["dot"], [0.001, 0.01]), a.warmup, a.iters)
    row = meshdist._reduce(out["distance"], out["dot"], [0.001, 0.01]).tolist()
    rec.update(mean_distance=row[1] / max(row[0], 1), max_distance=row[3], reduce_bytes=8 * N)
    counts = counted(q)
    if counts is not None:
        tests, cells, n = counts
        rec.update(tests_per_query=tests / n, cells_per_query=cells / n, row_bytes_per_query=(4 * tests + 16 * cells) / n,
                   corner_bytes_per_query=48 * tests / n, tests_per_s=tests / rec["query_ms"]["median"] * 1e3)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=256, help="lattice of the mesh that is queried")
    ap.add_argument("--second", type=int, default=200, help="lattice of the mesh that is sampled")
    ap.add_argument("--second-radius", "--second_radius", dest="second_radius", type=float, default=0.6,
                    help="radius of the sampled ball: 0.6 puts the queries ON the mesh, another radius that far off it")
    ap.add_argument("--samples", type=int, default=1_000_000)
    ap.add_argument("--brute", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--limit", type=int, default=120, help="seconds a step may take")
    ap.add_argument("--step", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_meshdist.py measures on the GPU; there is none here")
    if a.step:
        print(json.dumps(step(a.step, a)))
        return
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "second_radius": a.second_radius}
    for name in STEPS:                                                  # a fresh child per step, each under its own limit
        cmd = [sys.executable, os.path.abspath(__file__), "--step", name] + [f"--{k}={getattr(a, k)}" for k in
                                                                              ("points", "second", "second_radius", "samples", "brute", "warmup", "iters")]
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
