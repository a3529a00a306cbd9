"""numpy restatement of the surface extraction of csrc/nfl_surface.hip (marching tetrahedra on a regular lattice), for
tests/test_geometry_cpu.py and tests/test_geometry_gpu.py.  It depends on numpy alone, not on the product package.

The same split, ownership, order, fp32 formulae and conventions as the kernels (include/nerf_fl_amd.h, "surface"):

* lattice (nz, ny, nx) fp32, x fastest; a point is inside when value >= iso (NaN: outside);
* a corner of a cell is the bit mask c = dx | dy << 1 | dz << 2; every cell is split into the six Kuhn tetrahedra
  (0, a, a | b, 7), (a, b, c) running over the permutations of the axis bits (1, 2, 4) in lexicographic order;
* an edge joins corners lo and hi with lo a subset of hi; it belongs to the lattice point at corner lo and has the type
  m = hi ^ lo in 1..7; a crossing edge carries one vertex; vertices are ordered by (owner point, m), triangles by
  (cell, tetrahedron, place in TRI_TABLE);
* TRI_TABLE is built here from geometry (orientation: the triangle normal points from inside to outside); the kernels
  carry a printed copy of it (`python tests/geometry_ref.py` prints it).
"""
import itertools

import numpy as np

TETS = tuple(itertools.permutations((1, 2, 4)))     # lexicographic: (1,2,4) (1,4,2) (2,1,4) (2,4,1) (4,1,2) (4,2,1)
F = np.float32


def tet_corners(t):
    a, b, _ = TETS[t]
    return (0, a, a | b, 7)


def _corner_xyz(c):
    return np.array([c & 1, (c >> 1) & 1, (c >> 2) & 1], dtype=np.float64)


def _build_table():
    """TRI_TABLE[t][k]: the triangles of tetrahedron t when bit j of k says that its corner j is inside; a triangle is
    three edge codes (lo << 3 | m)."""
    table = []
    for t in range(6):
        cs = tet_corners(t)
        per_case = []
        for k in range(16):
            ins = [j for j in range(4) if (k >> j) & 1]
            out = [j for j in range(4) if not (k >> j) & 1]
            if len(ins) == 1:
                tris = [[(ins[0], o) for o in out]]
            elif len(ins) == 3:
                tris = [[(i, out[0]) for i in ins]]
            elif len(ins) == 2:
                (a, b), (c, d) = ins, out
                tris = [[(a, c), (a, d), (b, d)], [(a, c), (b, d), (b, c)]]
            else:
                tris = []
            way = (np.mean([_corner_xyz(cs[j]) for j in out], axis=0) - np.mean([_corner_xyz(cs[j]) for j in ins], axis=0)
                   if tris else None)
            coded = []
            for tri in tris:
                p = [0.5 * (_corner_xyz(cs[i]) + _corner_xyz(cs[j])) for i, j in tri]
                if np.dot(np.cross(p[1] - p[0], p[2] - p[0]), way) < 0:
                    tri = [tri[0], tri[2], tri[1]]
                code = []
                for i, j in tri:
                    lo, hi = sorted((cs[i], cs[j]))
                    assert lo & hi == lo
                    code.append(lo << 3 | (hi ^ lo))
                coded.append(tuple(code))
            per_case.append(tuple(coded))
        table.append(tuple(per_case))
    return tuple(table)


TRI_TABLE = _build_table()


def gradient(lat, spacing):
    """(3, nz, ny, nx) fp32: central differences (v[i+1] - v[i-1]) / (2 s), one-sided (v[i+1] - v[i]) / s at the border."""
    lat = np.asarray(lat, dtype=F)
    g = np.empty((3,) + lat.shape, dtype=F)
    with np.errstate(all="ignore"):
        for k, axis in enumerate((2, 1, 0)):          # x, y, z
            v = np.moveaxis(lat, axis, 0)
            out = np.empty_like(v)
            s = F(spacing[k])
            out[1:-1] = (v[2:] - v[:-2]) / (F(2) * s)
            out[0] = (v[1] - v[0]) / s
            out[-1] = (v[-1] - v[-2]) / s
            g[k] = np.moveaxis(out, 0, axis)
    return g


def extract(lat, iso, lo, spacing):
    """-> dict(vertices (V, 3) fp32, normals (V, 3) fp32, triangles (T, 3) int32) of the lattice `lat` (nz, ny, nx) whose
    point (x, y, z) lies at lo + (x, y, z) * spacing (lo, spacing: 3 numbers in x, y, z order, used in fp32)."""
    lat = np.ascontiguousarray(lat, dtype=F)
    nz, ny, nx = lat.shape
    iso, lo, sp = F(iso), np.asarray(lo, dtype=F), np.asarray(spacing, dtype=F)
    with np.errstate(invalid="ignore"):
        inside = lat >= iso
    cross = np.zeros((nz, ny, nx, 7), dtype=bool)
    for m in range(1, 8):
        dx, dy, dz = m & 1, (m >> 1) & 1, (m >> 2) & 1
        a = inside[:nz - dz, :ny - dy, :nx - dx]
        b = inside[dz:, dy:, dx:]
        cross[:nz - dz, :ny - dy, :nx - dx, m - 1] = a != b
    flat = cross.reshape(-1)
    vid = (np.cumsum(flat, dtype=np.int64) - flat).reshape(cross.shape)       # vertex of edge (point, m) where it crosses
    z, y, x, e = np.nonzero(cross)                                            # sorted by (point, m)
    m = e + 1
    ia = np.stack([x, y, z], axis=1)
    ib = ia + np.stack([m & 1, (m >> 1) & 1, (m >> 2) & 1], axis=1)
    va, vb = lat[z, y, x], lat[ib[:, 2], ib[:, 1], ib[:, 0]]
    g = gradient(lat, sp)
    with np.errstate(all="ignore"):
        t = (iso - va) / (vb - va)
        t = np.fmin(np.fmax(t, F(0)), F(1))[:, None]
        pa = lo + ia.astype(F) * sp
        pb = lo + ib.astype(F) * sp
        vertices = pa + t * (pb - pa)
        ga = g[:, z, y, x].T
        gb = g[:, ib[:, 2], ib[:, 1], ib[:, 0]].T
        n = -(ga + t * (gb - ga))
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
        normals = np.where(length > 0, n / length, F(0)).astype(F)
    # triangles
    ci = inside[:-1, :-1, :-1]
    corner = [inside[(c >> 2) & 1:nz - 1 + ((c >> 2) & 1), (c >> 1) & 1:ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
              for c in range(8)]
    cz, cy, cx = np.meshgrid(np.arange(nz - 1), np.arange(ny - 1), np.arange(nx - 1), indexing="ij")
    cell = (cz * (ny - 1) + cy) * (nx - 1) + cx
    keys, tris = [], []
    for ti in range(6):
        cs = tet_corners(ti)
        case = sum(corner[cs[j]].astype(np.int64) << j for j in range(4))
        for k in range(1, 15):
            sel = case == k
            if not sel.any():
                continue
            zz, yy, xx = cz[sel], cy[sel], cx[sel]
            for j, tri in enumerate(TRI_TABLE[ti][k]):
                ids = [vid[zz + ((code >> 5) & 1), yy + ((code >> 4) & 1), xx + ((code >> 3) & 1), (code & 7) - 1]
                       for code in tri]
                tris.append(np.stack(ids, axis=1))
                keys.append((cell[sel] * 6 + ti) * 2 + j)
    assert ci.shape == cell.shape
    if tris:
        tris, keys = np.concatenate(tris), np.concatenate(keys)
        triangles = tris[np.argsort(keys, kind="stable")].astype(np.int32)
    else:
        triangles = np.zeros((0, 3), dtype=np.int32)
    return {"vertices": vertices.astype(F).reshape(-1, 3), "normals": normals.reshape(-1, 3), "triangles": triangles}


def sphere_lattice(n, r0=0.6, lo=-1.0, hi=1.0):
    """r0 - |p| on an n^3 lattice over [lo, hi]^3 -> (lattice fp32, lo (3,), spacing (3,)); the points are placed in fp32
    as the extraction places them."""
    s = F((hi - lo) / (n - 1))
    c = (F(lo) + np.arange(n, dtype=F) * s).astype(np.float64)
    zz, yy, xx = np.meshgrid(c, c, c, indexing="ij")
    lat = (r0 - np.sqrt(xx * xx + yy * yy + zz * zz)).astype(F)
    return lat, np.full(3, lo, dtype=F), np.full(3, s, dtype=F)


def c_table():
    """The table as the initialiser of `uint8_t [6][16][6]` (unused places 0)."""
    rows = []
    for t in range(6):
        cases = []
        for k in range(16):
            codes = [c for tri in TRI_TABLE[t][k] for c in tri]
            codes += [0] * (6 - len(codes))
            cases.append("{" + ",".join(f"{c:2d}" for c in codes) + "}")
        rows.append("    {" + ", ".join(cases[:8]) + ",\n     " + ", ".join(cases[8:]) + "}")
    return ",\n".join(rows)


if __name__ == "__main__":
    print(c_table())
