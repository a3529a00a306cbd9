#!/usr/bin/env python3
"""What cleaning a mesh costs on one MI355X: nfl_mesh_label, nfl_mesh_stats, nfl_mesh_compact_count / _emit and the whole
geometry.clean_mesh call on the surface of `0.6 - |p|` (default 512^3), alone and with a few thousand small blobs added,
beside the host route they replace.  Not a test: prints one JSON record (and writes it to --out).

Every device figure is a median over `--iters` calls after `--warmup`, bracketed by device events; clean_mesh (allocation,
all passes and its two host synchronisations) and the host route are timed under a host clock.  The host route: copy the
index buffer to the host, label it with the numpy restatement (tests/mesh_ref.py), copy a vertex mask back; re-indexing the
triangles, which the device route includes, is not even in it.  The bytes are those the algorithm needs, from the shapes:
    label    12 B read per triangle; per vertex 4 B (init) + 4 + 4 + 4 (flatten: parent in, root and flag out) + 4 + 8
             (scan) + 4 + 8 + 4 (rank): 44 B.  The hooks' finds and compare-and-swaps come on top and are data-dependent.
    stats    16 B read per vertex, 4 + 4 B per triangle (first index, its id); the table is 32 B per component
    compact  count: per vertex 4 + 1 in, 4 out, 4 + 8 scan; per triangle 12 + 3 (4 + 1) in, 4 out, 4 + 8 scan;
             emit: per vertex 4 flag, kept ones 8 + 24 R (R = rows: vertices, normals, colors) ; per triangle 4 flag, kept
             ones 8 + 12 + 24 + 12"""
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


def lattice(n, blobs, dev):
    """0.6 - |p| on n^3 over [-1, 1]^3; with `blobs` > 0, small balls of radius 3 spacings on a regular grid outside it."""
    c = torch.linspace(-1, 1, n, device=dev, dtype=torch.float64)
    lat = (0.6 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float()
    if blobs:
        m = round(blobs ** (1 / 3))
        period = 2.0 / m
        d = (c + 1.0) % period - period / 2                                 # offset from the nearest blob centre, per axis
        r = 3 * 2.0 / (n - 1)
        ball = (r - torch.sqrt(d[:, None, None] ** 2 + d[None, :, None] ** 2 + d[None, None, :] ** 2)).float()
        lat = torch.where(lat < -0.1, torch.maximum(lat, ball), lat)       # only well outside the sphere
    return lat.contiguous()


def measure(name, lat, a, rec):
    from nerf_fl_amd import _lib, geometry
    import mesh_ref as mr
    dev = lat.device
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    mesh = geometry.extract_surface(lat, 0.0, lo, hi)
    ver, nrm, tri = mesh["vertices"], mesh["normals"], mesh["triangles"]
    V, T = ver.shape[0], tri.shape[0]
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    comps = geometry.mesh_components(mesh)
    n_comp = comps["n_components"]

    la = _lib.MeshLabelArgs()
    l_bytes = lib.nfl_mesh_label_bytes(V, T)
    l_scratch = torch.empty(l_bytes // 8 + 1, dtype=torch.int64, device=dev)
    component = torch.empty(V, dtype=torch.int32, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    la.d_triangles, la.n_vertices, la.n_triangles = tri.data_ptr(), V, T
    la.d_scratch, la.scratch_bytes, la.d_component, la.d_totals = l_scratch.data_ptr(), l_bytes, component.data_ptr(), totals.data_ptr()
    t_label = timed(lambda: _lib.check(lib.nfl_mesh_label(C.byref(la), stream()), "label"), a.warmup, a.iters)
    assert totals.tolist() == [n_comp, 0] and torch.equal(component, comps["component"])

    sa = _lib.MeshStatsArgs()
    n_ver, n_tri = torch.empty_like(comps["vertices"]), torch.empty_like(comps["triangles"])
    bounds = torch.empty_like(comps["bounds"])
    sa.d_component, sa.d_positions, sa.d_triangles = component.data_ptr(), ver.data_ptr(), tri.data_ptr()
    sa.n_vertices, sa.n_triangles, sa.n_components = V, T, n_comp
    sa.d_n_vertices, sa.d_n_triangles, sa.d_bounds = n_ver.data_ptr(), n_tri.data_ptr(), bounds.data_ptr()
    t_stats = timed(lambda: _lib.check(lib.nfl_mesh_stats(C.byref(sa), stream()), "stats"), a.warmup, a.iters)
    assert torch.equal(n_tri, comps["triangles"]) and torch.equal(bounds, comps["bounds"])

    keep = torch.zeros(n_comp, dtype=torch.bool, device=dev)
    keep[n_tri.to(torch.int64).argmax()] = True                            # what clean_mesh(largest=1) keeps
    ca = _lib.MeshCompactArgs()
    c_bytes = lib.nfl_mesh_compact_bytes(V, T)
    c_scratch = torch.empty(c_bytes // 8 + 1, dtype=torch.int64, device=dev)
    ca.d_component, ca.d_keep, ca.d_triangles = component.data_ptr(), keep.view(torch.uint8).data_ptr(), tri.data_ptr()
    ca.n_vertices, ca.n_triangles, ca.n_components = V, T, n_comp
    ca.d_scratch, ca.scratch_bytes, ca.d_totals = c_scratch.data_ptr(), c_bytes, totals.data_ptr()
    t_count = timed(lambda: _lib.check(lib.nfl_mesh_compact_count(C.byref(ca), stream()), "count"), a.warmup, a.iters)
    Vk, Tk = totals.tolist()
    out = [torch.empty(Vk, 3, dtype=torch.float32, device=dev) for _ in range(2)] + [torch.empty(Tk, 3, dtype=torch.int32, device=dev)]
    ca.n_kept_vertices, ca.n_kept_triangles = Vk, Tk
    ca.d_vertices, ca.d_normals, ca.d_out_vertices, ca.d_out_normals = ver.data_ptr(), nrm.data_ptr(), out[0].data_ptr(), out[1].data_ptr()
    ca.d_out_triangles = out[2].data_ptr()
    t_emit = timed(lambda: _lib.check(lib.nfl_mesh_compact_emit(C.byref(ca), stream()), "emit"), a.warmup, a.iters)
    cleaned = geometry.clean_mesh(mesh, largest=1)
    assert torch.equal(cleaned["vertices"], out[0]) and torch.equal(cleaned["triangles"], out[2])
    t_clean = host_timed(lambda: geometry.clean_mesh(mesh, largest=1), 0, a.iters)

    # the host route: indices to the host, components there, a vertex mask back
    def host_route():
        h = tri.cpu().numpy()
        comp, n, _ = mr.label(h, V)
        big = np.bincount(comp[h[:, 0]], minlength=n).argmax()
        return torch.from_numpy(comp == big).to(dev), comp
    mask, h_comp = host_route()
    assert np.array_equal(h_comp, component.cpu().numpy()) and int(mask.sum().item()) == Vk
    t_host = host_timed(lambda: host_route(), 0, a.host_iters)
    t_copy = host_timed(lambda: tri.cpu(), 0, a.iters)

    b_label = 12 * T + 44 * V
    b_stats = 16 * V + 8 * T + 32 * n_comp
    b_count = 21 * V + 43 * T
    b_emit = 4 * V + (8 + 24 * 2) * Vk + 4 * T + (8 + 12 + 24 + 12) * Tk
    gbps = lambda b, t: b / t["median"] / 1e6
    rec[name] = {
        "lattice": list(lat.shape), "vertices": V, "triangles": T, "components": n_comp, "kept_vertices": Vk, "kept_triangles": Tk,
        "label_scratch_bytes": l_bytes, "compact_scratch_bytes": c_bytes,
        "label_ms": t_label, "stats_ms": t_stats, "compact_count_ms": t_count, "compact_emit_ms": t_emit,
        "clean_mesh_whole_call_host_ms": t_clean,
        "host_route_ms": t_host, "host_route_index_copy_ms": t_copy,
        "label_bytes": b_label, "stats_bytes": b_stats, "compact_count_bytes": b_count, "compact_emit_bytes": b_emit,
        "label_GBps": gbps(b_label, t_label), "stats_GBps": gbps(b_stats, t_stats),
        "compact_count_GBps": gbps(b_count, t_count), "compact_emit_GBps": gbps(b_emit, t_emit)}
    print(json.dumps({name: rec[name]}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sphere", type=int, default=512)
    ap.add_argument("--blobs", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--host-iters", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_mesh.py measures on the GPU; there is none here")
    dev = torch.device("cuda:0")
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "host_iters": a.host_iters}
    measure("sphere", lattice(a.sphere, 0, dev), a, rec)
    measure("sphere_and_blobs", lattice(a.sphere, a.blobs, dev), a, rec)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
