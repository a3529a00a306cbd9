"""The definitions of include/nerf_fl_amd.h, "mesh distance", restated in numpy: one numpy operation per header operation,
fp32 where the header is fp32, so that the GPU tests can hold the kernels to the bit (the library is built with
-ffp-contract=off).  Brute-force closest point with the (dd, index) order, the cell function and the grid rows as sets, the
sample counts and points from the same hash, the reduction row in its fixed order; and mesh_distance put together from them
the way nerf_fl_amd.meshdist does, for the analytic checks.  No torch, no library."""
import numpy as np

F = np.float32
U64 = np.uint64
INF = F(np.inf)
COLUMNS, WITHIN, SUM_DOT, MAX_TAU = 13, 4, 12, 8
TWO_M24 = F(2.0 ** -24)


def mix(x):
    """The finaliser of splitmix64 on uint64 arrays (sums and products wrap)."""
    x = np.asarray(x, dtype=U64).copy()
    with np.errstate(over="ignore"):
        x ^= x >> U64(30)
        x *= U64(0xBF58476D1CE4E5B9)
        x ^= x >> U64(27)
        x *= U64(0x94D049BB133111EB)
        x ^= x >> U64(31)
    return x


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def usable(ver, tri):
    """(T,) bool: three indices in range and nine finite coordinates."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    V = len(ver)
    ok = ((tri >= 0) & (tri < V)).all(axis=1)
    if V:
        ok &= np.isfinite(ver[np.clip(tri, 0, V - 1)]).all(axis=(1, 2))
    return ok


def outside(ver, tri):
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    return int((~((tri >= 0) & (tri < len(ver))).all(axis=1)).sum())


# ---- the grid

def cellf(x, lo, cell, n):
    with np.errstate(all="ignore"):
        f = np.floor((np.asarray(x, dtype=F) - F(lo)) / F(cell))
    return np.fmin(np.fmax(f, F(0)), F(n - 1)).astype(np.int64)


def grid_rows(ver, tri, lo, cell, dims):
    """The rows of the grid as sorted lists, a list per cell in cell order; the totals (entries, outside)."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    nx, ny, nz = dims
    rows = [[] for _ in range(nx * ny * nz)]
    ok = usable(ver, tri)
    for t in np.nonzero(ok)[0]:
        c = ver[tri[t]]
        i0 = [int(cellf(c[:, k].min(), lo[k], cell, dims[k])) for k in range(3)]
        i1 = [int(cellf(c[:, k].max(), lo[k], cell, dims[k])) for k in range(3)]
        for z in range(i0[2], i1[2] + 1):
            for y in range(i0[1], i1[1] + 1):
                for x in range(i0[0], i1[0] + 1):
                    rows[(z * ny + y) * nx + x].append(int(t))
    return rows, (sum(len(r) for r in rows), outside(ver, tri))


# ---- point and triangle

def point_triangle(p, a, b, c):
    """The seven regions for queries p (N, 3) and ONE triangle (a, b, c): q (N, 3), uvw (N, 3), dd (N,), region (N,) 1..7."""
    p32 = np.asarray(p, dtype=F).reshape(-1, 3)
    a32, b32, c32 = (np.asarray(v, dtype=F).reshape(1, 3) for v in (a, b, c))
    p, a, b, c = (v.astype(np.float64) for v in (p32, a32, b32, c32))     # the regions and the parameters are fp64
    one = np.float64(1)
    with np.errstate(all="ignore"):
        ab, ac, bc = b - a, c - a, c - b
        ap, bp, cp = p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
        s3, s5, s6 = d1 / (d1 - d3), d2 / (d2 - d6), (d4 - d3) / ((d4 - d3) + (d5 - d6))
        den = one / ((va + vb) + vc)
        s7, r7 = vb * den, vc * den
        o, z = np.ones_like(d1), np.zeros_like(d1)
        col = lambda s: s[:, None]
        qs = [a + z[:, None], b + z[:, None], a + col(s3) * ab, c + z[:, None], a + col(s5) * ac, b + col(s6) * bc,
              (a + col(s7) * ab) + col(r7) * ac]
        ws = [(o, z, z), (z, o, z), (one - s3, s3, z), (z, z, o), (one - s5, z, s5), (z, one - s6, s6), ((one - s7) - r7, s7, r7)]
        region = np.select(conds, [1, 2, 3, 4, 5, 6], default=7)
        q = np.zeros_like(p)
        uvw = np.zeros_like(p)
        for k in range(7):
            m = region == k + 1
            q[m] = qs[k][m]
            uvw[m] = np.stack(ws[k], axis=1)[m]
        q, p, a, b, c = q.astype(F), p32, a32, b32, c32                       # and back: the clamp and the distance are fp32
        tri = np.concatenate([a, b, c])
        mn, mx = tri.min(axis=0)[None], tri.max(axis=0)[None]
        q = np.where(q < mn, mn, np.where(q > mx, mx, q)).astype(F)
        e = p - q
        dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
    return q, uvw.astype(F), dd.astype(F), region


def closest(points, ver, tri, max_distance=np.inf, normals=None):
    """Brute force, the (dd, index) order: distance, triangle, point, bary (and dot with `normals`)."""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    N = len(p)
    with np.errstate(all="ignore"):
        limit = F(max_distance) * F(max_distance)
    best = np.full(N, INF, dtype=F)
    best_t = np.full(N, -1, dtype=np.int32)
    best_q, best_w = np.full((N, 3), np.nan, dtype=F), np.full((N, 3), np.nan, dtype=F)
    asks = np.isfinite(p).all(axis=1)
    for t in np.nonzero(usable(ver, tri))[0]:                           # ascending: a tie keeps the lower index
        q, uvw, dd, _ = point_triangle(p, *ver[tri[t]])
        take = asks & (dd <= limit) & (dd < INF) & (dd < best)
        best[take], best_t[take], best_q[take], best_w[take] = dd[take], t, q[take], uvw[take]
    found = best_t >= 0
    out = {"distance": np.where(found, np.sqrt(best), INF).astype(F), "triangle": best_t, "point": best_q, "bary": best_w}
    if normals is not None:
        nq = np.asarray(normals, dtype=F).reshape(-1, 3)
        d = np.full(N, np.nan, dtype=F)
        if found.any():
            d[found] = dot(nq[found], face_normals(ver, tri)[best_t[found]])
        out["dot"] = d
    return out


def face_normals(ver, tri):
    """(T, 3): cross(ab, ac) / its length, zeros where that is zero (or the triangle is not usable)."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    ok = usable(ver, tri)
    c = ver[np.where(ok[:, None], tri, 0)] if len(ver) else np.zeros((len(tri), 3, 3), F)
    with np.errstate(all="ignore"):
        cr = cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        ln = np.sqrt(dot(cr, cr))
        n = np.where((ok & (ln > 0))[:, None], cr / ln[:, None], F(0))
    return n.astype(F)


# ---- surface samples

def sample_counts(ver, tri, density, seed):
    """m (T,) int32, the hashes ht (T,) and the totals (samples, outside, too dense)."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    T = len(tri)
    ok = usable(ver, tri)
    c = ver[np.where(ok[:, None], tri, 0)] if len(ver) else np.zeros((T, 3, 3), F)
    with np.errstate(all="ignore"):
        cr = cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        ln = np.sqrt(dot(cr, cr))
        ok = ok & (ln > 0) & np.isfinite(ln)
        ht = mix(mix(np.array([seed], dtype=U64)) + np.arange(T, dtype=U64))
        ut = (ht >> U64(40)).astype(F) * TWO_M24
        x = (F(0.5) * ln) * F(density) + ut
        dense = ok & ~(x < F(2.0 ** 24))
        m = np.where(ok & ~dense, np.floor(x), 0).astype(np.int32)
    return m, ht, (int(m.sum(dtype=np.int64)), outside(ver, tri), int(dense.sum()))


def samples(ver, tri, density, seed):
    """points (N, 3), triangles (N,), normals (N, 3): the samples in triangle order."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    m, ht, _ = sample_counts(ver, tri, density, seed)
    t = np.repeat(np.arange(len(tri)), m)
    j = np.arange(len(t)) - np.repeat(np.cumsum(m) - m, m)
    with np.errstate(over="ignore"):
        hj = mix(ht[t] + (j + 1).astype(U64))
    r1 = ((hj >> U64(40)).astype(F) + F(0.5)) * TWO_M24
    r2 = (((hj >> U64(16)) & U64(0xFFFFFF)).astype(F) + F(0.5)) * TWO_M24
    fold = r1 + r2 > F(1)
    r1, r2 = np.where(fold, F(1) - r1, r1), np.where(fold, F(1) - r2, r2)
    c = ver[tri[t]] if len(t) else np.zeros((0, 3, 3), F)
    e1, e2 = c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]
    pts = (c[:, 0] + r1[:, None] * e1) + r2[:, None] * e2
    cr = cross(e1, e2)
    nrm = cr / np.sqrt(dot(cr, cr))[:, None]
    return pts.astype(F), t.astype(np.int32), nrm.astype(F)


# ---- the reduction

def _fold(red):
    """(256, COLUMNS) folded by halving into row 0; the maximum column by fmax."""
    red = red.copy()
    off = 128
    while off:
        lo, hi = red[:off], red[off:2 * off]
        s = lo + hi
        s[:, 3] = np.fmax(lo[:, 3], hi[:, 3])
        red[:off] = s
        off //= 2
    return red[0]


def reduce_row(distance, dot_=None, taus=()):
    """The (13,) fp64 row of nfl_meshdist_reduce, in the kernel's order of additions."""
    d = np.asarray(distance, dtype=F).reshape(-1)
    n = len(d)
    G = min((n + 255) // 256, 1024)
    if G == 0:
        return np.zeros(COLUMNS)
    with np.errstate(invalid="ignore"):
        counts = d < INF
    x = d.astype(np.float64)
    terms = np.zeros((n, COLUMNS))
    terms[:, 0], terms[:, 1], terms[:, 2], terms[:, 3] = 1.0, x, x * x, x
    for k, tau in enumerate(taus):
        with np.errstate(invalid="ignore"):
            terms[:, WITHIN + k] = d <= F(tau)
    if dot_ is not None:
        terms[:, SUM_DOT] = np.abs(np.asarray(dot_, dtype=F).reshape(-1).astype(np.float64))
    terms[~counts] = 0.0                                                # a missing element adds nothing (and fmax(., 0) = .)
    J = (n + G * 256 - 1) // (G * 256)
    pad = np.zeros((J * G * 256, COLUMNS))
    pad[:n] = terms
    pad = pad.reshape(J, G, 256, COLUMNS)                               # element (g + j G) * 256 + t
    live = (np.arange(J * G * 256) < n).reshape(J, G, 256) & np.pad(counts, (0, J * G * 256 - n)).reshape(J, G, 256)
    acc = np.zeros((G, 256, COLUMNS))
    for j in range(J):
        s = acc + pad[j]
        s[:, :, 3] = np.fmax(acc[:, :, 3], pad[j][:, :, 3])
        acc = np.where(live[j][:, :, None], s, acc)                     # a skipped element leaves -0.0 + 0.0 alone, too
    parts = np.stack([_fold(acc[g]) for g in range(G)])
    fin = np.zeros((256, COLUMNS))
    for i in range(G):                                                  # thread i % 256 adds rows i, i + 256, ... in order
        t = i % 256
        s = fin[t] + parts[i]
        s[3] = np.fmax(fin[t][3], parts[i][3])
        fin[t] = s
    return _fold(fin)


# ---- meshes of the analytic checks, and mesh_distance as nerf_fl_amd.meshdist puts it together

def square(shift=(0.0, 0.0, 0.0)):
    """The unit square [0, 1]^2 x {0} of two triangles, moved by `shift`; normals +z."""
    ver = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], dtype=F) + np.asarray(shift, dtype=F)
    return {"vertices": ver.astype(F), "normals": np.tile(F([0, 0, 1]), (4, 1)),
            "triangles": np.array([[0, 1, 2], [0, 2, 3]], dtype=np.int32)}


def total_area(ver, tri):
    ok = usable(ver, tri)
    c = np.asarray(ver, dtype=np.float64)[np.asarray(tri)[ok]]
    return float((0.5 * np.linalg.norm(np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]), axis=1)).sum())


def mesh_distance(a, b, n=1000, thresholds=(), max_distance=None, seed=0, points="samples"):
    limit = np.inf if max_distance is None else max_distance

    def one_way(src, dst):
        if points == "samples":
            p, _, nrm = samples(src["vertices"], src["triangles"], n / total_area(src["vertices"], src["triangles"]), seed)
        else:
            p, nrm = src["vertices"], src["normals"]
        got = closest(p, dst["vertices"], dst["triangles"], limit, nrm)
        return reduce_row(got["distance"], got["dot"], thresholds), len(p), got

    rab, na, gab = one_way(a, b)
    rba, nb, _ = one_way(b, a)

    def side(r, total):
        cnt = r[0]
        return {"mean": r[1] / cnt if cnt else np.nan, "rms": np.sqrt(r[2] / cnt) if cnt else np.nan, "max": r[3], "n": total,
                "missing": int(total - cnt)}, (r[12] / cnt if cnt else np.nan)

    ab, nc_ab = side(rab, na)
    ba, nc_ba = side(rba, nb)
    prec = [rab[4 + k] / na for k in range(len(thresholds))]
    rec = [rba[4 + k] / nb for k in range(len(thresholds))]
    fs = [2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(prec, rec)]
    return {"a_to_b": ab, "b_to_a": ba, "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "hausdorff": max(ab["max"], ba["max"]),
            "normal_consistency": 0.5 * (nc_ab + nc_ba), "precision": prec, "recall": rec, "fscore": fs,
            "distances_a_to_b": gab["distance"]}


# ---- what the two analytic squares must give, on the restatement (test_meshdist_cpu.py) and on the device (test_meshdist_gpu.py)

def check_shifted_along_the_normal(r, d=0.25):
    for side in ("a_to_b", "b_to_a"):
        assert r[side]["missing"] == 0 and r[side]["n"] > 0
        for k in ("mean", "rms", "max"):
            assert abs(r[side][k] - d) <= 1e-6, (side, k, r[side][k])
    assert abs(r["chamfer"] - d) <= 1e-6 and abs(r["hausdorff"] - d) <= 1e-6
    assert r["fscore"] == [0.0, 1.0] and r["precision"] == [0.0, 1.0] and r["recall"] == [0.0, 1.0]
    assert abs(r["normal_consistency"] - 1.0) <= 1e-6


def check_shifted_in_the_plane(side, s=0.5):
    """One direction between the unit square and its copy moved by s along x: the distance of a point at x is max(s - x, 0),
    so its mean is s^2 / 2 and its variance s^3 / 3 - s^4 / 4."""
    n = side["n"]
    se = np.sqrt((s ** 3 / 3 - s ** 4 / 4) / n)
    assert side["missing"] == 0 and abs(side["mean"] - s * s / 2) <= 5 * se, (side, se)
    assert side["max"] <= s and side["max"] >= s - 10 * (1.0 / (n * 1.0))         # the expected gap to the edge is 1 / (n x 1)
