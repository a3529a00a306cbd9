#!/usr/bin/env python3
"""What simplifying a mesh costs on one MI355X: geometry.simplify_mesh (nfl_mesh_simplify_count / _emit, allocation and
the one host synchronisation included) on the surface of a ball of radius 1.2 in [-1.5, 1.5]^3 (the case of DESIGN section
20's table) extracted on a 257^3 lattice, at cells of 2, 4 and 8 lattice spacings and both placements; the two C calls on
their own; and extract_mesh on a seeded field with and without simplify=, which shows the colour pass shrinking.
Not a test: prints one JSON record (and writes it to --out).

The C calls are medians over `--iters` calls after `--warmup`, bracketed by device events; simplify_mesh and extract_mesh
are timed under a host clock, synchronised either side."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import host_timed, timed  # noqa: E402


def ball(n, dev):
    """1.2 - |p| on n^3 over [-1.5, 1.5]^3."""
    c = torch.linspace(-1.5, 1.5, n, device=dev, dtype=torch.float64)
    return (1.2 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()


def measure_ball(a, rec):
    from nerf_fl_amd import _lib, geometry
    dev = torch.device("cuda:0")
    lo, hi = (-1.5, -1.5, -1.5), (1.5, 1.5, 1.5)
    mesh = geometry.extract_surface(ball(a.lattice, dev), 0.0, lo, hi)
    mesh["colors"] = (mesh["normals"].abs() * 0.5 + 0.25).contiguous()
    V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    spacing = 3.0 / (a.lattice - 1)
    lib = _lib.lib()
    nbytes = lib.nfl_mesh_simplify_bytes(V, T)
    rec["ball"] = {"lattice": a.lattice, "vertices": V, "triangles": T, "scratch_bytes": nbytes,
                   "input_bytes": 36 * V + 12 * T, "cases": []}
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev)
    totals = torch.empty(4, dtype=torch.int64, device=dev)
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for k in a.cells:
        for placement in ("mean", "quadric"):
            cell = k * spacing
            out = geometry.simplify_mesh(mesh, cell, origin=lo, placement=placement)
            Vo, To = out["vertices"].shape[0], out["triangles"].shape[0]
            s = _lib.MeshSimplifyArgs()
            s.d_vertices, s.d_normals, s.d_colors = mesh["vertices"].data_ptr(), mesh["normals"].data_ptr(), mesh["colors"].data_ptr()
            s.d_triangles, s.n_vertices, s.n_triangles = mesh["triangles"].data_ptr(), V, T
            s.cell, s.placement = cell, _lib.SIMPLIFY_PLACEMENTS[placement]
            for i in range(3):
                s.origin[i] = lo[i]
            s.d_scratch, s.scratch_bytes, s.d_totals, s.d_cluster = scratch.data_ptr(), nbytes, totals.data_ptr(), cluster.data_ptr()
            t_count = timed(lambda: _lib.check(lib.nfl_mesh_simplify_count(C.byref(s), stream()), "count"), a.warmup, a.iters)
            assert totals.tolist()[:2] == [Vo, To]
            bufs = [torch.empty(Vo, 3, dtype=torch.float32, device=dev) for _ in range(3)]
            tri = torch.empty(To, 3, dtype=torch.int32, device=dev)
            s.n_out_vertices, s.n_out_triangles = Vo, To
            s.d_out_vertices, s.d_out_normals, s.d_out_colors = (b.data_ptr() for b in bufs)
            s.d_out_triangles = tri.data_ptr()
            t_emit = timed(lambda: _lib.check(lib.nfl_mesh_simplify_emit(C.byref(s), stream()), "emit"), a.warmup, a.iters)
            assert torch.equal(tri, out["triangles"]) and torch.equal(bufs[2], out["colors"])
            t_call = host_timed(lambda: geometry.simplify_mesh(mesh, cell, origin=lo, placement=placement), a.warmup, a.iters)
            case = {"cell_spacings": k, "placement": placement, "out_vertices": Vo, "out_triangles": To,
                    "count_ms": t_count, "emit_ms": t_emit, "simplify_mesh_whole_call_host_ms": t_call}
            rec["ball"]["cases"].append(case)
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
        for k in (None,) + tuple(a.cells):
            kw = {} if k is None else {"simplify": k * 2.0 / (n - 1)}
            mesh = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, **kw)
            t = host_timed(lambda: geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, **kw), a.warmup, a.iters)
            ver, nrm = mesh["vertices"], mesh["normals"]
            t_col = host_timed(lambda: geometry.surface_colors(model, emb, ver, nrm), a.warmup, a.iters)
            case = {"cell_spacings": k, "vertices": ver.shape[0], "triangles": mesh["triangles"].shape[0],
                    "extract_mesh_host_ms": t, "surface_colors_host_ms": t_col}
            rec["extract_mesh"]["cases"].append(case)
            print(json.dumps(case), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lattice", type=int, default=257)
    ap.add_argument("--field-lattice", type=int, default=129)
    ap.add_argument("--cells", type=float, nargs="+", default=[2.0, 4.0, 8.0])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_simplify.py measures on the GPU; there is none here")
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters}
    measure_ball(a, rec)
    measure_extract(a, rec)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
