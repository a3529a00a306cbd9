#!/usr/bin/env python3
"""What smoothing a mesh costs on one MI355X: the C calls of csrc/nfl_meshsmooth.hip on the surface of a ball of radius 1.2
in [-1.5, 1.5]^3 extracted on a 257^3 lattice (the mesh of DESIGN section 21's table) -- adjacency count and emit, one
smoothing step, ten Taubin iterations, the vertex normals -- the whole geometry.smooth_mesh call (allocation and the one
host synchronisation of its adjacency included); the same calls on a fan with a hub of 4096 triangles, where one row is
long; and extract_mesh on a seeded field with and without smooth=3.
Not a test: prints one JSON record (and writes it to --out).

The C calls are medians over `--iters` calls after `--warmup`, bracketed by device events; smooth_mesh and extract_mesh
are timed under a host clock, synchronised either side.  Beside every step the bytes it has to move (24 B a vertex of own
position read and written, 4 B of index and 12 B of gathered position a neighbour entry) and the rate that implies: at this
size the buffers fit the last-level cache and repeated calls read the same data, so that rate is not an HBM figure."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import host_timed, timed  # noqa: E402
from time_simplify import ball  # noqa: E402


def measure_mesh(name, mesh, a, rec):
    from nerf_fl_amd import _lib, geometry
    dev = mesh["vertices"].device
    V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    adj = geometry.mesh_adjacency(mesh)
    I, N = adj["incident"].shape[0], adj["neighbors"].shape[0]
    nbytes = lib.nfl_mesh_adjacency_bytes(V, T)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    out = {k: torch.empty_like(adj[k]) for k in ("offsets", "neighbors", "boundary", "tri_offsets", "incident")}
    s = _lib.MeshAdjacencyArgs()
    s.d_triangles, s.n_vertices, s.n_triangles = mesh["triangles"].data_ptr(), V, T
    s.d_scratch, s.scratch_bytes, s.d_totals = scratch.data_ptr(), nbytes, totals.data_ptr()
    t_count = timed(lambda: _lib.check(lib.nfl_mesh_adjacency_count(C.byref(s), stream()), "count"), a.warmup, a.iters)
    assert totals.tolist()[:2] == [I, N]
    s.n_incident, s.n_neighbors = I, N
    s.d_tri_offsets, s.d_incident = out["tri_offsets"].data_ptr(), out["incident"].data_ptr()
    s.d_offsets, s.d_neighbors, s.d_boundary = out["offsets"].data_ptr(), out["neighbors"].data_ptr(), out["boundary"].data_ptr()
    t_emit = timed(lambda: _lib.check(lib.nfl_mesh_adjacency_emit(C.byref(s), stream()), "emit"), a.warmup, a.iters)
    assert all(torch.equal(out[k], adj[k]) for k in out)

    ping = torch.empty(lib.nfl_mesh_smooth_bytes(V) // 8 + 1, dtype=torch.int64, device=dev)
    moved = torch.empty_like(mesh["vertices"])
    m = _lib.MeshSmoothArgs()
    m.d_vertices, m.d_offsets, m.d_neighbors = mesh["vertices"].data_ptr(), adj["offsets"].data_ptr(), adj["neighbors"].data_ptr()
    m.n_vertices, m.n_neighbors, m.d_boundary, m.fix_boundary = V, N, adj["boundary"].data_ptr(), 1
    m.d_scratch, m.scratch_bytes, m.d_out_vertices = ping.data_ptr(), ping.numel() * 8, moved.data_ptr()
    steps = {}
    for label, factors in (("one_step", [0.5]), ("ten_taubin_iterations", [0.5, -0.53] * 10)):
        host = (C.c_double * len(factors))(*factors)
        m.n_steps, m.factors = len(factors), host
        steps[label] = timed(lambda: _lib.check(lib.nfl_mesh_smooth(C.byref(m), stream()), "smooth"), a.warmup, a.iters)
    normals = torch.empty_like(mesh["vertices"])
    n = _lib.MeshNormalsArgs()
    n.d_vertices, n.d_triangles, n.n_vertices, n.n_triangles = mesh["vertices"].data_ptr(), mesh["triangles"].data_ptr(), V, T
    n.d_tri_offsets, n.d_incident, n.n_incident = adj["tri_offsets"].data_ptr(), adj["incident"].data_ptr(), I
    n.weighting, n.d_fallback_normals, n.d_out_normals = 0, mesh["normals"].data_ptr(), normals.data_ptr()
    t_normals = timed(lambda: _lib.check(lib.nfl_mesh_normals(C.byref(n), stream()), "normals"), a.warmup, a.iters)
    t_call = host_timed(lambda: geometry.smooth_mesh(mesh, 10), a.warmup, a.iters)
    t_given = host_timed(lambda: geometry.smooth_mesh(mesh, 10, adjacency=adj), a.warmup, a.iters)
    step_bytes = 24 * V + 16 * N + 16 * V                   # own position in and out, index + position a neighbour, two offsets
    normal_bytes = 12 * V + 16 * V + I * (4 + 12 + 36)      # out, two offsets, entry + triangle + three positions
    case = {"mesh": name, "vertices": V, "triangles": T, "incident": I, "neighbors": N,
            "longest_row": int((adj["offsets"][1:] - adj["offsets"][:-1]).max().item()) if V else 0,
            "adjacency_scratch_bytes": nbytes, "adjacency_count_ms": t_count, "adjacency_emit_ms": t_emit,
            "smooth_one_step_ms": steps["one_step"], "smooth_ten_taubin_iterations_ms": steps["ten_taubin_iterations"],
            "vertex_normals_ms": t_normals, "smooth_mesh_whole_call_host_ms": t_call,
            "smooth_mesh_given_adjacency_host_ms": t_given,
            "step_bytes": step_bytes, "step_gb_per_s": step_bytes / steps["one_step"]["median"] / 1e6,
            "step_of_twenty_gb_per_s": 20 * step_bytes / steps["ten_taubin_iterations"]["median"] / 1e6,
            "normals_bytes": normal_bytes, "normals_gb_per_s": normal_bytes / t_normals["median"] / 1e6}
    rec["meshes"].append(case)
    print(json.dumps(case), flush=True)


def measure_extract(a, rec):
    import nerf_fl_amd
    from gpu_util import make_embeddings
    from nerf_fl_amd import NeRF, geometry, synth
    dev = torch.device("cuda:0")
    nerf_fl_amd.set_precision("f16x3")
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(dev)
    emb = make_embeddings(10, False)
    n = a.field_lattice
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (n, n, n)
    with torch.no_grad():
        iso = geometry.density_lattice(model, emb, lo, hi, res).median().item()
        rec["extract_mesh"] = {"lattice": n, "iso": iso, "cases": []}
        for smooth in (None, 3):
            kw = {} if smooth is None else {"smooth": smooth}
            mesh = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, **kw)
            t = host_timed(lambda: geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, **kw), a.warmup, a.iters)
            case = {"smooth": smooth, "vertices": mesh["vertices"].shape[0], "triangles": mesh["triangles"].shape[0],
                    "extract_mesh_host_ms": t}
            rec["extract_mesh"]["cases"].append(case)
            print(json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=257)
    ap.add_argument("--field-lattice", type=int, default=129)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "meshsmooth.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_meshsmooth.py measures on the GPU; there is none here")
    from nerf_fl_amd import geometry
    import meshsmooth_ref as mr
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "meshes": []}
    lo, hi = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
    measure_mesh(f"ball {a.lattice}^3", geometry.extract_surface(ball(a.lattice, dev), 0.0, lo, hi), a, rec)
    fan = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in mr.fan(4096, 300, seed=0).items()}
    measure_mesh("fan, hub of 4096", fan, a, rec)
    measure_extract(a, rec)
    print(json.dumps(rec))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
