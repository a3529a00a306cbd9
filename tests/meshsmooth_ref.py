"""numpy restatement of the mesh smoothing of csrc/nfl_meshsmooth.hip (include/nerf_fl_amd.h, "mesh smoothing"), for
tests/test_meshsmooth_cpu.py, tests/test_meshsmooth_gpu.py and tests/time_meshsmooth.py.  numpy alone, int64 and fp64,
sort based; nothing of the product package, no hash table.

The same definitions as the kernels:

* a triangle with an index outside [0, V) is counted and takes part in nothing;
* the incident entries of v are the numbers 3 t + c with tri[t][c] == v, ascending; I is their total;
* the candidates of v are, per incident entry, the other two indices of the triangle without those equal to v; the
  neighbour row holds the distinct candidates ascending; boundary[v] = some candidate has multiplicity 1;
* a smoothing step: a vertex that is not finite or pinned stays; else the fp64 sum of its finite neighbours in row order
  (np.add.at adds unbuffered, in array order), m = s / d, fl32(p + f * (m - p));
* a vertex normal: the fp64 sum in entry order of (p1 - p0) x (p2 - p0) ("area") or of that vector over its length
  ("uniform"), vectors with a non-finite component or all zero left out; fl32(s / |s|), the fallback row when |s| is 0 or
  not finite.
"""
import numpy as np

AREA, UNIFORM = "area", "uniform"


def adjacency(triangles, V):
    """-> dict(tri_offsets (V + 1,) int64, incident (I,) int32, offsets (V + 1,) int64, neighbors (N,) int32,
    boundary (V,) bool, totals [I, N, out of range, boundary vertices])."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    inside = ((tri >= 0) & (tri < V)).all(axis=1)
    t_in = np.flatnonzero(inside)
    e = (3 * t_in[:, None] + np.arange(3)).reshape(-1)      # ascending
    ver = tri[t_in].reshape(-1)
    order = np.argsort(ver, kind="stable")                  # by (vertex, entry)
    incident, owner = e[order], ver[order]
    tri_offsets = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(owner, minlength=V), out=tri_offsets[1:])
    t, c = incident // 3, incident % 3
    other = np.stack([tri[t, (c + 1) % 3], tri[t, (c + 2) % 3]], axis=1).reshape(-1)
    own2 = np.repeat(owner, 2)
    keep = other != own2
    pair, mult = np.unique(own2[keep] * max(V, 1) + other[keep], return_counts=True)      # sorted by (vertex, neighbour)
    row, neighbors = pair // max(V, 1), pair % max(V, 1)
    offsets = np.zeros(V + 1, dtype=np.int64)
    np.cumsum(np.bincount(row, minlength=V), out=offsets[1:])
    boundary = np.zeros(V, dtype=bool)
    boundary[row[mult == 1]] = True
    return {"tri_offsets": tri_offsets, "incident": incident.astype(np.int32), "offsets": offsets,
            "neighbors": neighbors.astype(np.int32), "boundary": boundary,
            "totals": [len(incident), len(neighbors), int((~inside).sum()), int(boundary.sum())]}


def factors(iterations, lam=0.5, mu=-0.53):
    return [lam] * iterations if mu is None else [lam, mu] * iterations


def smooth(vertices, adj, steps, pinned=None, fix_boundary=True):
    """The positions after the steps of factors `steps`: (V, 3) fp32."""
    P = np.array(vertices, dtype=np.float32).reshape(-1, 3)
    V = len(P)
    offsets, nbr = adj["offsets"], adj["neighbors"].astype(np.int64)
    row = np.repeat(np.arange(V), np.diff(offsets))
    stays = np.zeros(V, dtype=bool) if pinned is None else np.asarray(pinned).astype(bool).copy()
    if fix_boundary:
        stays |= adj["boundary"]
    for f in steps:
        fin = np.isfinite(P).all(axis=1)
        ok = fin[nbr]
        s = np.zeros((V, 3), dtype=np.float64)
        np.add.at(s, row[ok], P[nbr[ok]].astype(np.float64))
        d = np.bincount(row[ok], minlength=V)
        move = fin & ~stays & (d > 0)
        p = P[move].astype(np.float64)
        m = s[move] / d[move].astype(np.float64)[:, None]
        nxt = P.copy()
        nxt[move] = (p + np.float64(f) * (m - p)).astype(np.float32)
        P = nxt
    return P


def normals(vertices, triangles, adj, weighting=AREA, fallback=None):
    """(V, 3) fp32 vertex normals from the triangles."""
    assert weighting in (AREA, UNIFORM)
    ver = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = len(ver)
    incident = adj["incident"].astype(np.int64)
    row = np.repeat(np.arange(V), np.diff(adj["tri_offsets"]))
    p = ver.astype(np.float64)[tri[incident // 3]]          # (I, 3 corners, 3)
    s = np.zeros((V, 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        good = np.isfinite(cr).all(axis=1) & (cr != 0.0).any(axis=1)
        cr, row = cr[good], row[good]
        if weighting == UNIFORM:
            cr = cr / np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])[:, None]
        np.add.at(s, row, cr)
        length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
        ok = np.isfinite(length) & (length > 0.0)
        out = np.where(ok[:, None], s / length[:, None], 0.0).astype(np.float32)
    if fallback is not None:
        out[~ok] = np.asarray(fallback, dtype=np.float32).reshape(-1, 3)[~ok]
    return out


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", pinned=None, normals_weighting=AREA):
    """What nerf_fl_amd.geometry.smooth_mesh returns, on arrays."""
    adj = adjacency(mesh["triangles"], len(mesh["vertices"]))
    out = dict(mesh)
    out["vertices"] = smooth(mesh["vertices"], adj, factors(iterations, lam, mu), pinned, boundary == "fixed")
    if normals_weighting is not None:
        out["normals"] = normals(out["vertices"], mesh["triangles"], adj, normals_weighting, mesh["normals"])
    return out


# ---- the meshes of the tests

def _mesh(ver, tri):
    ver = np.asarray(ver, dtype=np.float32).reshape(-1, 3)
    return {"vertices": ver, "normals": np.tile(np.float32([0, 0, 1]), (len(ver), 1)),
            "triangles": np.asarray(tri, dtype=np.int32).reshape(-1, 3)}


def hand_cases():
    """name -> mesh: the cases whose rows and flags tests/test_meshsmooth_cpu.py writes out."""
    sq = [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]]
    return {
        "one_triangle": _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 1, 2]]),
        "tetrahedron": _mesh([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], [[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]]),
        "square": _mesh(sq, [[0, 1, 2], [0, 2, 3]]),
        "three_on_an_edge": _mesh([[0, 0, 0], [0, 0, 1], [1, 0, 0], [0, 1, 0], [-1, -1, 0]], [[0, 1, 2], [0, 1, 3], [0, 1, 4]]),
        "bow_tie": _mesh([[0, 0, 0], [1, 1, 0], [1, -1, 0], [-1, 1, 0], [-1, -1, 0]], [[0, 1, 2], [0, 3, 4]]),
        "isolated_vertex": _mesh(sq + [[5, 5, 5]], [[0, 1, 2], [0, 2, 3]]),
        "repeated_index": _mesh([[0, 0, 0], [1, 0, 0], [0, 1, 0]], [[0, 0, 1], [0, 1, 2]]),
        "out_of_range": _mesh(sq, [[0, 1, 2], [0, 2, 4], [-1, 0, 1], [0, 2, 3]]),
        "nan_vertex": _mesh([[0, 0, 0], [1, np.nan, 0], [1, 1, 0], [0, 1, 0], [2, 0, 0]], [[0, 1, 2], [0, 2, 3], [1, 4, 2]]),
    }


def grid_patch(n=5):
    """An open n x n grid of vertices in the plane z = 0.1 sin(3 x) cos(2 y), every square split in two."""
    g = np.arange(n, dtype=np.float64)
    yy, xx = np.meshgrid(g, g, indexing="ij")
    ver = np.stack([xx, yy, 0.1 * np.sin(3.0 * xx) * np.cos(2.0 * yy)], axis=-1).reshape(-1, 3)
    tri = []
    for j in range(n - 1):
        for i in range(n - 1):
            a = j * n + i
            tri += [[a, a + 1, a + n + 1], [a, a + n + 1, a + n]]
    return _mesh(ver, tri)


def soup(V, T, seed, span=3.0):
    """A random triangle soup: a few non-finite vertices and a few repeated indices (every index in range)."""
    rng = np.random.default_rng(seed)
    ver = rng.uniform(-span, span, (V, 3)).astype(np.float32)
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    tri = rng.integers(0, V, (T, 3)).astype(np.int32)
    if V >= 16:
        ver[3, 0], ver[5, 2], ver[7, 1] = np.nan, np.inf, -np.inf
    return {"vertices": ver, "normals": nrm, "triangles": tri}


def fan(hub_triangles=4096, ordinary=300, seed=0):
    """A closed fan of `hub_triangles` triangles around vertex 0 (a row of that many incident entries and neighbours)
    beside a strip of `ordinary` vertices with rows of a few; the triangles are shuffled."""
    rng = np.random.default_rng(seed)
    n = hub_triangles
    ang = 2.0 * np.pi * np.arange(n) / n
    rim = np.stack([np.cos(ang), np.sin(ang), 0.05 * rng.standard_normal(n)], axis=1)
    ver = [np.array([[0.0, 0.0, 0.3]]), rim]
    tri = [[0, 1 + k, 1 + (k + 1) % n] for k in range(n)]
    base = 1 + n
    m = ordinary // 2
    strip = np.stack([np.repeat(np.arange(m), 2) * 0.1 + 3.0, np.tile([0.0, 0.1], m), 0.02 * rng.standard_normal(2 * m)], axis=1)
    ver.append(strip)
    for k in range(m - 1):
        a = base + 2 * k
        tri += [[a, a + 2, a + 1], [a + 1, a + 2, a + 3]]
    tri = np.array(tri, dtype=np.int32)
    return _mesh(np.concatenate(ver), tri[rng.permutation(len(tri))])


def noisy_ball(n=33, sigma=0.01, seed=0):
    """(the marching-tetrahedra mesh of a ball of radius 0.6 on an n^3 lattice, the same with seeded radial noise)."""
    import geometry_ref as gr
    lat, lo, sp = gr.sphere_lattice(n)
    clean = gr.extract(lat, 0.0, lo, sp)
    rng = np.random.default_rng(seed)
    ver = clean["vertices"].astype(np.float64)
    r = np.linalg.norm(ver, axis=1, keepdims=True)
    noisy = dict(clean, vertices=(ver * (1.0 + sigma * rng.standard_normal((len(ver), 1)) / r)).astype(np.float32))
    return clean, noisy
