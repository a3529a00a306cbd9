#!/usr/bin/env python3
"""What the geometry feature costs on one MI355X: geometry.extract_surface on a sphere lattice (default 512^3) and
geometry.density_lattice on the base field (default 256^3).  Not a test: prints one JSON record (and writes it to --out).

Every figure is a median over `--iters` calls after `--warmup`, bracketed by device events; the count pass (two launches)
and the emit pass (one launch) of the extraction are timed through the C ABI on their own, and the whole
extract_surface call (allocation, both passes and its one host synchronisation) under a host clock.  The bytes are those
the algorithm needs, computed from the shapes:
    count  4 B read + 4 B written per lattice point (+ 16 B per slab of 256 points)
    emit   4 B + 4 B read per lattice point, 24 B written per vertex, 12 B per triangle
    field  36 B written per evaluated point (the pass's per-sample record), 4 B depth read, 4 B read + 4 B written by the copy
`--bench-render FILE` takes the JSON line of `bench.py --mode render` from the same machine, to set the lattice pass's
ray-samples/s next to the renderer's."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sphere", type=int, default=512)
    ap.add_argument("--field", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bench-render", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_geometry.py measures on the GPU; there is none here")
    from nerf_fl_amd import NeRF, PosEmbedding, _lib, geometry, rendering, synth
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters}

    # ---- extraction: r0 - |p| on n^3 over [-1, 1]^3
    n = a.sphere
    c = torch.linspace(-1, 1, n, device=dev, dtype=torch.float64)
    lat = (0.6 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    mesh = geometry.extract_surface(lat, 0.0, lo, hi)
    V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    lib = _lib.lib()
    nbytes = lib.nfl_surface_bytes(n, n, n)
    scratch = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    sa = _lib.SurfaceArgs()
    sa.d_lattice, sa.nx, sa.ny, sa.nz, sa.iso = lat.data_ptr(), n, n, n, 0.0
    for k in range(3):
        sa.lo[k], sa.spacing[k] = -1.0, 2.0 / (n - 1)
    sa.d_scratch, sa.scratch_bytes, sa.d_totals = scratch.data_ptr(), scratch.numel() * 8, totals.data_ptr()
    sa.n_vertices, sa.n_triangles = V, T
    sa.d_vertices, sa.d_normals, sa.d_triangles = (mesh[k].data_ptr() for k in ("vertices", "normals", "triangles"))
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    t_count = timed(lambda: _lib.check(lib.nfl_surface_count(C.byref(sa), stream()), "count"), a.warmup, a.iters)
    assert totals.tolist() == [V, T]
    t_emit = timed(lambda: _lib.check(lib.nfl_surface_emit(C.byref(sa), stream()), "emit"), a.warmup, a.iters)
    again = geometry.extract_surface(lat, 0.0, lo, hi)
    assert all(torch.equal(mesh[k], again[k]) for k in mesh)
    host = []
    for _ in range(a.iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        geometry.extract_surface(lat, 0.0, lo, hi)
        torch.cuda.synchronize()
        host.append((time.perf_counter() - t0) * 1e3)
    P = n ** 3
    slabs = -(-n // 256) * n * n
    b_count = 8 * P + 16 * slabs
    b_emit = 8 * P + 24 * V + 12 * T
    rec["extract_surface"] = {
        "lattice": [n, n, n], "vertices": V, "triangles": T, "scratch_bytes": nbytes,
        "count_ms": t_count, "emit_ms": t_emit, "whole_call_host_ms_median": statistics.median(host),
        "count_bytes": b_count, "emit_bytes": b_emit,
        "count_GBps": b_count / t_count["median"] / 1e6, "emit_GBps": b_emit / t_emit["median"] / 1e6,
        "bytes_per_voxel": {"count": b_count / P, "emit": b_emit / P}}
    del lat, mesh, again, scratch

    # ---- the field on a lattice: the base fine model, seeded synthetic weights
    m = a.field
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(dev)
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    res = (m, m, m)
    with torch.no_grad():
        t_field = timed(lambda: geometry.density_lattice(model, emb, lo, hi, res), max(1, a.warmup - 1), max(3, a.iters // 2))
        # worst deviation from field_forward on the same points, on a slice of the lattice
        sig = geometry.density_lattice(model, emb, lo, hi, res)
        pts = geometry.lattice_points(lo, hi, res, dev)[m // 2].reshape(-1, 3)
        exp = rendering.field_forward(model, rendering.posenc(pts, 10), sigma_only=True).reshape(m, m)
        err = ((sig[m // 2] - exp).abs() / exp.abs().clamp(min=1.0)).max().item()
    rendering.check_status(dev)
    cdiv = lambda p, q: -(-p // q)
    pieces = cdiv(m, 256)                                    # as geometry.density_lattice cuts the rows
    S = cdiv(cdiv(m, pieces), 32) * 32 if pieces > 1 else m
    evaluated = m * m * pieces * (-(-S // 32) * 32)          # the kernel evaluates whole 32-sample segments
    b_field = m * m * pieces * S * 40 + 8 * m ** 3
    rec["density_lattice"] = {
        "lattice": [m, m, m], "ms": t_field, "points": m ** 3, "points_evaluated": evaluated,
        "ray_samples_per_s": m ** 3 / t_field["median"] * 1e3,
        "bytes": b_field, "GBps": b_field / t_field["median"] / 1e6, "bytes_per_voxel": b_field / m ** 3,
        "worst_relative_error_vs_field_forward": err, "precision": rendering.get_precision()}
    if a.bench_render and os.path.exists(a.bench_render):
        for line in open(a.bench_render):
            line = line.strip()
            if line.startswith("{"):
                b = json.loads(line)
                rec["bench_render"] = {"metric": b.get("metric"), "ray_samples_per_s": b.get("value"),
                                       "ms_per_step": b.get("ms_per_step"), "dtype": b.get("dtype")}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
