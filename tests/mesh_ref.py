"""numpy restatement of the mesh cleaning of csrc/nfl_mesh.hip (include/nerf_fl_amd.h, "mesh"), for tests/test_mesh_cpu.py,
tests/test_mesh_gpu.py and tests/time_mesh.py.  It depends on numpy alone (no scipy), not on the product package.

The same definitions as the kernels:

* two vertices are connected when a triangle names both; a vertex no triangle names is a component of its own; sharing
  one vertex connects two triangles; repeated indices inside a triangle are allowed;
* the root of a vertex is the smallest vertex index of its component; components are numbered in ascending order of root;
* a triangle with an index outside [0, V) is ignored everywhere and counted;
* the table: vertex count, triangle count (by the FIRST index), per-axis min and max of the finite coordinates taken in
  the order-preserving integer map of fp32 (so that -0 < +0, as on the device), +inf / -inf where there is none;
* compaction: a vertex is kept when its component is, a triangle when it is not ignored and its three vertices are kept;
  kept rows stay in their order, triangle indices are remapped.
"""
import numpy as np


def valid_triangles(triangles, V):
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    return ((tri >= 0) & (tri < V)).all(axis=1)


def roots(triangles, V):
    """-> (root (V,) int64, number of ignored triangles): min-label propagation over the triangle edges with pointer
    jumping, to a fixed point."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    ok = valid_triangles(tri, V)
    tri = tri[ok]
    label = np.arange(V, dtype=np.int64)
    while True:
        before = label.copy()
        if len(tri):
            seen = label[tri]                               # after the jumping below these are roots: label[r] == r
            low = seen.min(axis=1)                          # the smallest label a triangle sees goes to the other two roots
            np.minimum.at(label, seen.reshape(-1), np.repeat(low, 3))
        while True:                                         # pointer jumping: label[v] <= v, follow it to its end
            nxt = label[label]
            if np.array_equal(nxt, label):
                break
            label = nxt
        if np.array_equal(label, before):
            return label, int((~ok).sum())


def label(triangles, V):
    """-> (component (V,) int32, C, ignored)."""
    root, ignored = roots(triangles, V)
    is_root = root == np.arange(V)
    rank = np.cumsum(is_root) - is_root                     # exclusive scan of the root flags
    return rank[root].astype(np.int32), int(is_root.sum()), ignored


def _key(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def _unkey(k):
    k = np.asarray(k, dtype=np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


def stats(component, C, positions, triangles):
    """-> (vertices (C,) int32, triangles (C,) int32, bounds (C, 2, 3) fp32)."""
    component = np.asarray(component, dtype=np.int64)
    V = len(component)
    pos = np.asarray(positions, dtype=np.float32).reshape(V, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    tri = tri[valid_triangles(tri, V)]
    n_ver = np.bincount(component, minlength=C).astype(np.int32)
    n_tri = np.bincount(component[tri[:, 0]], minlength=C).astype(np.int32)
    lo = np.full((C, 3), 0xFF800000, dtype=np.uint32)      # key(+inf)
    hi = np.full((C, 3), 0x007FFFFF, dtype=np.uint32)      # key(-inf)
    key = _key(pos)
    for k in range(3):
        fin = np.isfinite(pos[:, k])
        np.minimum.at(lo[:, k], component[fin], key[fin, k])
        np.maximum.at(hi[:, k], component[fin], key[fin, k])
    return n_ver, n_tri, np.stack([_unkey(lo), _unkey(hi)], axis=1)


def compact(component, keep, mesh):
    """`mesh`: dict of arrays (vertices, normals, triangles, perhaps colors); keep (C,) bool -> the filtered dict."""
    component = np.asarray(component, dtype=np.int64)
    keep = np.asarray(keep, dtype=bool)
    V = len(component)
    tri = np.asarray(mesh["triangles"], dtype=np.int64).reshape(-1, 3)
    kv = keep[component] if V else np.zeros(0, dtype=bool)
    ok = valid_triangles(tri, V)
    kt = np.zeros(len(tri), dtype=bool)
    kt[ok] = kv[tri[ok]].all(axis=1)
    new_id = np.cumsum(kv) - kv
    out = {k: np.asarray(mesh[k])[kv] for k in ("vertices", "normals", "colors") if mesh.get(k) is not None}
    out["triangles"] = new_id[tri[kt]].astype(np.int32).reshape(-1, 3)
    return out


def clean_keep(n_triangles, bounds, largest=None, min_triangles=None, box=None):
    """The keep flags geometry.clean_mesh builds: every criterion judged on its own over all components."""
    n_triangles = np.asarray(n_triangles, dtype=np.int64)
    keep = np.ones(len(n_triangles), dtype=bool)
    if min_triangles is not None:
        keep &= n_triangles >= min_triangles
    if box is not None:
        lo, hi = (np.asarray(b, dtype=np.float32) for b in box)
        keep &= ((bounds[:, 0] <= bounds[:, 1]) & (bounds[:, 0] >= lo) & (bounds[:, 1] <= hi)).all(axis=1)   # +inf > -inf: no bounds
    if largest is not None:
        among = np.zeros(len(keep), dtype=bool)
        among[np.argsort(-n_triangles, kind="stable")[:largest]] = True
        keep &= among
    return keep


def three_balls():
    """The end-to-end case: (lattice (22, 24, 40) fp32, lo, hi, spacing), max of three balls r - |p - c|."""
    lo, hi, res = (-1.0, -0.6, -0.55), (1.0, 0.6, 0.55), (40, 24, 22)
    sp = [np.float32((h - l) / (n - 1)) for l, h, n in zip(lo, hi, res)]
    ax = [(np.float32(l) + np.arange(n, dtype=np.float32) * s).astype(np.float64) for l, s, n in zip(lo, sp, res)]
    zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    lat = np.full(xx.shape, -np.inf)
    for c, r in (((-0.45, 0.0, 0.0), 0.4), ((0.5, 0.1, 0.0), 0.22), ((0.5, -0.4, -0.3), 0.09)):
        lat = np.maximum(lat, r - np.sqrt((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2))
    return lat.astype(np.float32), lo, hi, sp, xx
