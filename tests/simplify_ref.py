"""numpy restatement of the mesh simplification of csrc/nfl_simplify.hip (include/nerf_fl_amd.h, "mesh simplification"), for
tests/test_simplify_cpu.py, tests/test_simplify_gpu.py and tests/time_simplify.py.  numpy alone, int64 and fp64, sort and
dict based; nothing of the product package, no hash table.

The same definitions as the kernels:

* cell of a vertex: per axis i = floor(((double)p - origin) / cell); valid when the coordinates are finite and every i lies
  in [-2^20, 2^20); the key packs the three shifted indices into 63 bits; the centre is origin + (i + 0.5) * cell;
* clusters are numbered in ascending order of their smallest member; cluster[v] = -1 for a vertex that is not valid;
* a triangle with an index outside [0, V) is counted and dropped; so is one on a vertex without a cluster or with two
  equal new ids; of the triangles equal up to rotation the lowest index survives, in its own corner order;
* a cluster of one keeps its member's bits; otherwise sums of rint(x * 2^30) in int64 (x relative to the cell centre in cell
  units for positions; non-finite normal and colour components count 0); mean, normalised normal, mean colour;
* "quadric": A += w n n^T, b += w d n per corner of every triangle with valid corners and a finite non-zero area, in fp64 in
  the order of the triangles, then (A + mu I) u = mu u~ - b with mu = LAMBDA trace(A), clamped to the cell.
"""
import numpy as np

HALF = 1 << 20
FIX = float(1 << 30)
LAMBDA = 1e-3


def cells(vertices, cell, origin=(0.0, 0.0, 0.0)):
    """-> (valid (V,) bool, ijk (V, 3) int64 -- 0 where not valid, pd (V, 3) fp64)."""
    ver = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
    pd = ver.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        fi = np.floor((pd - np.asarray(origin, dtype=np.float64)) / np.float64(cell))
        valid = (np.isfinite(ver) & (fi >= -HALF) & (fi < HALF)).all(axis=1)
    ijk = np.zeros(fi.shape, dtype=np.int64)
    ijk[valid] = fi[valid].astype(np.int64)
    return valid, ijk, pd


def keys(ijk):
    s = ijk + HALF
    return s[:, 0] | (s[:, 1] << 21) | (s[:, 2] << 42)


def clusters(vertices, cell, origin=(0.0, 0.0, 0.0)):
    """-> (cluster (V,) int32, V', leader (V',) int64: the smallest member of every cluster)."""
    valid, ijk, _ = cells(vertices, cell, origin)
    cluster = np.full(len(valid), -1, dtype=np.int32)
    idx = np.flatnonzero(valid)
    if len(idx) == 0:
        return cluster, 0, np.zeros(0, dtype=np.int64)
    _, first, inverse = np.unique(keys(ijk[idx]), return_index=True, return_inverse=True)      # first: in idx order = ascending v
    order = np.argsort(first, kind="stable")                # sorted keys -> ascending smallest member
    rank = np.empty(len(order), dtype=np.int64)
    rank[order] = np.arange(len(order))
    cluster[idx] = rank[inverse.reshape(-1)]
    return cluster, len(order), idx[first[order]]


def triangles(tri, cluster):
    """-> (new triangles (T', 3) int32, survivors (T',) int64 input indices, number out of range)."""
    tri = np.asarray(tri, dtype=np.int64).reshape(-1, 3)
    V = len(cluster)
    inside = ((tri >= 0) & (tri < V)).all(axis=1)
    cand = np.flatnonzero(inside)
    m = cluster[tri[cand]].astype(np.int64)
    ok = (m >= 0).all(axis=1) & (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    cand, m = cand[ok], m[ok]
    if len(cand) == 0:
        return np.zeros((0, 3), dtype=np.int32), cand, int((~inside).sum())
    start = m.argmin(axis=1)
    canon = np.take_along_axis(m, (start[:, None] + np.arange(3)) % 3, axis=1)
    _, first = np.unique(canon, axis=0, return_index=True)  # the first of every set, cand being ascending
    keep = np.sort(first)
    return m[keep].astype(np.int32), cand[keep], int((~inside).sum())


def _fixed(x):
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.rint(np.where(np.isfinite(x), x, 0.0) * FIX), 0.0).astype(np.int64)


def quadric_sums(mesh, cell, origin, cluster, n_out, order=None):
    """-> (V', 9) fp64: A (xx xy xz yy yz zz) and b of every cluster, accumulated in the order `order` of the triangles."""
    valid, ijk, pd = cells(mesh["vertices"], cell, origin)
    cell, origin = np.float64(cell), np.asarray(origin, dtype=np.float64)
    tri = np.asarray(mesh["triangles"], dtype=np.int64).reshape(-1, 3)
    if order is not None:
        tri = tri[order]
    tri = tri[((tri >= 0) & (tri < len(valid))).all(axis=1)]
    tri = tri[valid[tri].all(axis=1)]
    Q = np.zeros((n_out, 9))
    if len(tri) == 0:
        return Q
    p = pd[tri]                                             # (t, 3 corners, 3)
    e1, e2 = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    with np.errstate(all="ignore"):
        cr = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2],
                       e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], axis=1)
        length = np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
        area = 0.5 * length
        good = np.isfinite(area) & (area > 0.0)
    tri, p, cr, length, area = tri[good], p[good], cr[good], length[good], area[good]
    n = cr / length[:, None]
    w = area / (cell * cell)
    for j in range(3):
        centre = origin + (ijk[tri[:, j]].astype(np.float64) + 0.5) * cell
        u0 = (p[:, 0] - centre) / cell
        d = -((n[:, 0] * u0[:, 0] + n[:, 1] * u0[:, 1]) + n[:, 2] * u0[:, 2])
        rows = np.stack([w * n[:, 0] * n[:, 0], w * n[:, 0] * n[:, 1], w * n[:, 0] * n[:, 2], w * n[:, 1] * n[:, 1],
                         w * n[:, 1] * n[:, 2], w * n[:, 2] * n[:, 2], w * d * n[:, 0], w * d * n[:, 1], w * d * n[:, 2]], axis=1)
        np.add.at(Q, cluster[tri[:, j]], rows)
    return Q


def quadric_solve(Q, ubar):
    """u (V', 3) fp64 of the definition from the sums Q (V', 9) and the fixed-point means."""
    u = ubar.copy()
    for c in range(len(Q)):
        A = np.array([[Q[c, 0], Q[c, 1], Q[c, 2]], [Q[c, 1], Q[c, 3], Q[c, 4]], [Q[c, 2], Q[c, 4], Q[c, 5]]])
        tr = (Q[c, 0] + Q[c, 3]) + Q[c, 5]
        if tr == 0.0:
            continue
        mu = LAMBDA * tr
        try:
            with np.errstate(all="ignore"):
                x = np.linalg.solve(A + mu * np.eye(3), mu * ubar[c] - Q[c, 6:9])
        except np.linalg.LinAlgError:
            continue
        if np.isfinite(x).all():
            u[c] = np.clip(x, -0.5, 0.5)
    return u


def simplify(mesh, cell, origin=(0.0, 0.0, 0.0), placement="mean", order=None):
    """`mesh`: dict of arrays (vertices, normals, triangles, perhaps colors) -> (the simplified dict, cluster, totals
    [V', T', out of range, invalid]).  `order` permutes the triangles of the quadric sums only."""
    assert placement in ("mean", "quadric")
    ver = np.asarray(mesh["vertices"], dtype=np.float32).reshape(-1, 3)
    nrm = np.asarray(mesh["normals"], dtype=np.float32).reshape(-1, 3)
    col = None if mesh.get("colors") is None else np.asarray(mesh["colors"], dtype=np.float32).reshape(-1, 3)
    V = len(ver)
    valid, ijk, pd = cells(ver, cell, origin)
    cluster, n_out, leader = clusters(ver, cell, origin)
    new_tri, _, outside = triangles(mesh["triangles"], cluster)
    members = np.flatnonzero(valid)
    cl = cluster[members].astype(np.int64)
    n = np.bincount(cl, minlength=n_out)
    cellf, originf = np.float64(cell), np.asarray(origin, dtype=np.float64)
    centre_v = originf + (ijk.astype(np.float64) + 0.5) * cellf
    sums = np.zeros((n_out, 9), dtype=np.int64)
    np.add.at(sums[:, 0:3], cl, _fixed((pd[members] - centre_v[members]) / cellf))
    np.add.at(sums[:, 3:6], cl, _fixed(nrm[members].astype(np.float64)))
    if col is not None:
        np.add.at(sums[:, 6:9], cl, _fixed(col[members].astype(np.float64)))
    scale = n.astype(np.float64)[:, None] * FIX
    ubar = sums[:, 0:3].astype(np.float64) / scale if n_out else np.zeros((0, 3))
    u = ubar
    if placement == "quadric" and n_out:
        u = quadric_solve(quadric_sums(mesh, cell, origin, cluster, n_out, order), ubar)
    centre = centre_v[leader]
    s = sums[:, 3:6].astype(np.float64)
    length = np.sqrt((s[:, 0] * s[:, 0] + s[:, 1] * s[:, 1]) + s[:, 2] * s[:, 2])
    with np.errstate(all="ignore"):
        out = {"vertices": (centre + cellf * u).astype(np.float32),
               "normals": np.where(length[:, None] > 0.0, s / length[:, None], 0.0).astype(np.float32),
               "triangles": new_tri}
        if col is not None:
            out["colors"] = (sums[:, 6:9].astype(np.float64) / scale).astype(np.float32)
    alone = n == 1
    out["vertices"][alone], out["normals"][alone] = ver[leader[alone]], nrm[leader[alone]]
    if col is not None:
        out["colors"][alone] = col[leader[alone]]
    return out, cluster, [n_out, len(new_tri), outside, int(V - valid.sum())]


# ---- the meshes of the tests

def cube_surface(n=6, lo=-1.0, hi=1.0):
    """The surface of the axis-aligned cube [lo, hi]^3, every face an n x n grid of quads split in two, welded, wound
    outwards; normals are the normalised sums of the face normals a vertex lies on."""
    g = np.linspace(lo, hi, n + 1)
    index, ver, tri = {}, [], []

    def vid(p):
        key = tuple(np.round((np.asarray(p) - lo) / (hi - lo) * n).astype(int))
        if key not in index:
            index[key] = len(ver)
            ver.append(p)
        return index[key]

    for axis in range(3):
        for side, w in ((0, lo), (1, hi)):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            for i in range(n):
                for j in range(n):
                    q = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = [0.0, 0.0, 0.0]
                        p[axis], p[a], p[b] = w, g[i + di], g[j + dj]
                        q.append(vid(p))
                    if side == 0:
                        q = q[::-1]                         # e_a x e_b = +e_axis: the low face looks the other way
                    tri += [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    ver = np.array(ver, dtype=np.float32)
    nrm = ((ver == np.float32(hi)).astype(np.float64) - (ver == np.float32(lo)).astype(np.float64))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return {"vertices": ver, "normals": nrm.astype(np.float32), "triangles": np.array(tri, dtype=np.int32)}


def ball_lattice(n=33, radius=0.6):
    """(lattice (n, n, n) fp32 of radius - |p| over [-1, 1]^3, lo, hi, spacing)."""
    lo, hi = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
    sp = [np.float32(2.0 / (n - 1))] * 3
    ax = (np.float32(-1.0) + np.arange(n, dtype=np.float32) * sp[0]).astype(np.float64)
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing="ij")
    return (radius - np.sqrt(xx * xx + yy * yy + zz * zz)).astype(np.float32), lo, hi, sp


def soup(V, T, seed, span=3.0):
    """A random triangle soup with colours; a few vertices that belong to no cluster and a few repeated indices."""
    rng = np.random.default_rng(seed)
    ver = rng.uniform(-span, span, (V, 3)).astype(np.float32)
    nrm = rng.standard_normal((V, 3)).astype(np.float32)
    col = rng.random((V, 3)).astype(np.float32)
    tri = rng.integers(0, V, (T, 3)).astype(np.int32)
    if V >= 16:
        ver[3, 0], ver[5, 2], ver[7, 1] = np.nan, np.inf, -np.inf
        nrm[9, 1], col[11, 0] = np.nan, np.inf
    return {"vertices": ver, "normals": nrm, "colors": col, "triangles": tri}


def _mesh(ver, tri, nrm=None, col=None):
    ver = np.asarray(ver, dtype=np.float32).reshape(-1, 3)
    nrm = np.tile(np.float32([0, 0, 1]), (len(ver), 1)) if nrm is None else np.asarray(nrm, dtype=np.float32)
    mesh = {"vertices": ver, "normals": nrm, "triangles": np.asarray(tri, dtype=np.int32).reshape(-1, 3)}
    if col is not None:
        mesh["colors"] = np.asarray(col, dtype=np.float32)
    return mesh


def hand_cases():
    """name -> (mesh, cell, origin): the cases whose results tests/test_simplify_cpu.py writes out."""
    below = np.nextafter(np.float32(1), np.float32(0))
    lim = float(HALF)
    row = lambda xs: [[x, 0.5, 0.5] for x in xs]
    return {
        "two_in_one_cell": (_mesh([[0.25, 0.25, 0.25], [0.75, 0.5, 0.25], [1.5, 0.5, 0.5]], [[0, 1, 2]],
                                  nrm=[[1, 0, 0], [0, 1, 0], [0, 0, 1]], col=[[0, 0.5, 1], [1, 0.5, 0], [0.25, 0.25, 0.25]]),
                            1.0, (0.0, 0.0, 0.0)),
        "on_a_face_and_on_origin": (_mesh([[1, 1, 1], [1.5, 1, 0.5], [below, 1, 1]], [[0, 1, 2]]), 0.5, (1.0, 1.0, 1.0)),
        "negative": (_mesh([[-0.5, -1.0, -1.5], [-0.25, -0.75, -1.25], [0.5, 0.5, 0.5]], [[0, 2, 1]]), 1.0, (0.0, 0.0, 0.0)),
        "limits": (_mesh(row([-lim, lim - 0.5, lim, -lim - 0.5]), [[0, 1, 2], [1, 0, 3], [0, 1, 1]]), 1.0, (0.0, 0.0, 0.0)),
        "nan_vertex": (_mesh([[0.5, 0.5, 0.5], [1.5, np.nan, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5]], [[0, 1, 2], [0, 2, 3]]),
                       1.0, (0.0, 0.0, 0.0)),
        "square_to_nothing": (_mesh([[0.125, 0.125, 0.5], [0.875, 0.125, 0.5], [0.875, 0.875, 0.5], [0.125, 0.875, 0.5]],
                                    [[0, 1, 2], [0, 2, 3]]), 1.0, (0.0, 0.0, 0.0)),
        "rotation_and_mirror": (_mesh(row([0.5, 1.5, 2.5, 0.25, 1.25, 2.25]), [[0, 1, 2], [4, 5, 3], [0, 2, 1], [5, 1, 3]]),
                                1.0, (0.0, 0.0, 0.0)),
    }
