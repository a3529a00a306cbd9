"""The definitions of include/nerf_fl_amd.h, "mesh solid", restated in numpy on top of meshcast_ref.py (the ray test, the walk) and
meshdist_ref.py (the closest point, cellf): THE CROSSINGS by brute force and by the count-mode walk, slab by slab, with THE
ONCE-ONLY RULE; the votes and the inside flag along THE DIRECTIONS; and what nerf_fl_amd/solid.py composes of them -- the lattice
points, the signed distance, the lattice value.  No torch, no library."""
import os

import numpy as np

import meshcast_ref as cref
import meshdist_ref as dref

F = np.float32
INF = F(np.inf)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# THE DIRECTIONS, copied from the header: component k of direction j is sign * sqrt(PRIMES[j][k]) rounded to fp32
PRIMES = ((29, 3, 7), (5, 31, 2), (11, 13, 37), (41, 17, 19), (23, 53, 43), (47, 59, 67), (73, 61, 71))
DIRECTIONS = F([[5.38516474, 1.73205078, 2.64575124], [-2.23606801, 5.56776428, -1.41421354],
                [3.31662488, -3.60555124, 6.08276272], [-6.40312433, -4.12310553, 4.35889912],
                [4.79583168, -7.28010988, -6.55743837], [-6.85565472, -7.68114567, -8.18535233],
                [8.54400349, 7.81024981, -8.42614937]])


# ---- THE CROSSINGS

def crossings(rays, ver, tri, box=None):
    """Brute force, which is the definition: (N,) int32, the usable triangles whose ray test accepts the ray."""
    r = np.asarray(rays, dtype=F).reshape(-1, 8)
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    count = np.zeros(len(r), dtype=np.int32)
    for t in np.nonzero(dref.usable(ver, tri))[0]:
        count += cref.ray_triangle(r, *ver[tri[t]], box=box)[0]
    return count


def walk_count(ray, lo, cell, dims, box, rows, tests, r, once=True):
    """The count-mode walk for ray number r.  THE WALK with no hit held runs to its end: meshcast_ref.walk over rows that list
    nothing tells the cells it reads, in order.  Every triangle of every such cell is tried (`tests` is meshcast_ref.table's),
    and an accepted hit counts in the cell of its own point qf alone -- THE ONCE-ONLY RULE, which `once=False` leaves out."""
    visits = []
    cref.walk(ray, lo, cell, dims, box, {}, {}, r, cref.FIRST, visits)
    assert len(set(visits)) == len(visits)                                    # no cell is read twice
    count = 0
    for c in visits:
        for t in rows.get(c, ()):
            hit, _, _, qf = tests[t]
            if not hit[r]:
                continue
            x, y, z = (int(dref.cellf(qf[r, k], lo[k], cell, dims[k])) for k in range(3))
            if not once or (z * dims[1] + y) * dims[0] + x == c:
                count += 1
    return count


def crossings_grid(rays, ver, tri, lo, cell, dims, once=True):
    """The grid count: crossings()'s integers, found by the count-mode walk."""
    r = np.asarray(rays, dtype=F).reshape(-1, 8)
    lo, cell = [float(F(x)) for x in lo], float(F(cell))
    box = cref.box_of(lo, cell, dims)
    rows, tests = cref.rows_of(ver, tri, lo, cell, dims), cref.table(r, ver, tri, box)
    count = np.zeros(len(r), dtype=np.int32)
    for n in np.nonzero(cref.valid(r))[0]:
        count[n] = walk_count(r[n], lo, cell, dims, box, rows, tests, n, once)
    return count


# ---- INSIDE

def rays_from(points, j):
    """The ray [p, DIRECTIONS[j], 0, +inf] of every point."""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    return np.concatenate([p, np.tile(DIRECTIONS[j], (len(p), 1)), np.zeros((len(p), 1), F), np.full((len(p), 1), INF)], axis=1).astype(F)


def parities(points, ver, tri, K, box=None, cull=True):
    """(K, N) int: whether direction j < K crosses an odd number of triangles from each point; a non-finite point is no ray: 0.

    `cull` spares the ray test where it cannot accept, and changes no count.  An accepted hit has tf >= near = 0, so its
    point on the ray r[k] = o[k] + t * d[k] lies on the side of o[k] that d[k] points to; qf[k] lies in the triangle's
    bounding box and within tol of r[k], and tol <= 2^-19 * (2 * max|o| + max|vertex|) (|t d[k]| <= |o[k]| + |qf[k]| + tol).  A
    triangle whose box ends more than that before o[k], against the direction, on any axis is therefore never crossed."""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    rays = np.concatenate([rays_from(p, j) for j in range(K)])
    if not cull:
        return (crossings(rays, ver, tri, box) & 1).reshape(K, len(p))
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    count = np.zeros(len(rays), dtype=np.int32)
    o, up = rays[:, :3].astype(np.float64), rays[:, 3:6] > 0
    with np.errstate(invalid="ignore"):
        slack = cref.TWO_M19 * (2.0 * np.abs(o).max(axis=1, keepdims=True) + float(np.abs(ver[np.isfinite(ver)]).max(initial=0.0)))
    for t in np.nonzero(dref.usable(ver, tri))[0]:
        c = ver[tri[t]].astype(np.float64)
        with np.errstate(invalid="ignore"):
            can = (np.where(up, c.max(axis=0)[None] - o, o - c.min(axis=0)[None]) >= -slack).all(axis=1)
        idx = np.nonzero(can)[0]
        if len(idx):
            count[idx] += cref.ray_triangle(rays[idx], *ver[tri[t]], box=box)[0]
    return (count & 1).reshape(K, len(p))


def majority(points, odd, K):
    """(inside (N,) bool, votes (N,) uint8) of the first K rows of parities()."""
    assert K in (1, 3, 5, 7) and len(odd) >= K
    finite = np.isfinite(np.asarray(points, dtype=F).reshape(-1, 3)).all(axis=1)
    votes = odd[:K].sum(axis=0)
    return finite & (2 * votes > K), np.where(finite, votes, 255).astype(np.uint8)


def inside(points, ver, tri, K, box=None, cull=True):
    """(inside (N,) bool, votes (N,) uint8): the parity of the crossings along the first K directions, and their majority."""
    return majority(points, parities(points, ver, tri, K, box, cull), K)


# ---- what solid.py composes

def lattice_points(lo, hi, res):
    """(nz, ny, nx, 3) fp32: geometry.lattice_points."""
    sp = [(h - l) / (n - 1) for l, h, n in zip(lo, hi, res)]
    x, y, z = (np.arange(res[k], dtype=F) * F(sp[k]) + F(lo[k]) for k in range(3))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx, yy, zz], axis=-1).astype(F)


def signed_distance(points, ver, tri, K, box, max_distance=np.inf):
    """(signed distance (N,) fp32, inside, votes): meshdist_ref.closest's distance, negated where inside."""
    flag, votes = inside(points, ver, tri, K, box)
    d = dref.closest(points, ver, tri, max_distance)["distance"]
    return np.where(flag, -d, d).astype(F), flag, votes


def lattice_value(sd, trunc):
    """clamp(sd * fp32(-1 / trunc), -1, 1) in fp32: positive inside."""
    with np.errstate(all="ignore"):
        return np.clip(np.asarray(sd, dtype=F) * F(-1.0 / trunc), F(-1), F(1)).astype(F)


def default_trunc(lo, hi, res):
    return 3.0 * max((h - l) / (n - 1) for l, h, n in zip(lo, hi, res))


# ---- the meshes and points that test_meshsolid_cpu.py and test_meshsolid_gpu.py share

def soup():
    """(ver, tri, rays, whole): meshcast_ref's 40 triangles and its rays of seven kinds -- near = 0 and far = +inf for most -- and
    behind them, because the random rays with cut bounds of that set seldom have a crossing to lose, every ray of the set
    that crosses the soup at two parameters or more, twice again: once with far, once with near, half way between its first
    two crossings.  `whole` names the ray each of these was cut from."""
    ver, tri = cref.soup40()
    rays = cref.soup_rays(ver, tri)
    tests = cref.table(rays, ver, tri, None)
    hit, tf = np.stack([tests[t][0] for t in tests]), np.stack([tests[t][1] for t in tests])
    cut, whole = [], []
    for n in range(len(rays)):
        ts = np.unique(tf[hit[:, n], n])
        if len(ts) >= 2 and np.isfinite(ts[:2]).all():
            mid = F(0.5 * (float(ts[0]) + float(ts[1])))
            if ts[0] < mid < ts[1]:
                cut += [np.concatenate([rays[n, :7], [mid]]), np.concatenate([rays[n, :6], [mid], rays[n, 7:]])]
                whole += [n, n]
    return ver, tri, np.concatenate([rays, np.array(cut, dtype=F)]).astype(F), np.array(whole)


def ball():
    """geom_gpu_util.ball_mesh(0.8, 17) as extract_surface emits it, kept as a fixture so that the CPU tests have it too;
    test_meshsolid_gpu.py holds the fixture to the device's bits."""
    z = np.load(os.path.join(GOLDEN, "meshsolid_ball_08_17.npz"))
    return z["vertices"].astype(F), z["triangles"].astype(np.int32)


def ball_lattice():
    """The restated composition at the 17^3 lattice points over [-1, 1]^3 for the ball, before the lattice value: the points,
    trunc, the signed distance within trunc, the flags and the votes of three directions.  Computed by
    tests/golden/make_meshsolid_golden.py with the functions above (half a minute: too long for every run of the suite);
    test_meshsolid_cpu.py checks it against the analytic ball everywhere and against a fresh computation at some points."""
    box, res = ((-1.0,) * 3, (1.0,) * 3), (17, 17, 17)
    z = np.load(os.path.join(GOLDEN, "meshsolid_lattice_17.npz"))
    return dict(lo=box[0], hi=box[1], res=res, pts=lattice_points(*box, res).reshape(-1, 3), trunc=default_trunc(*box, res),
                sd=z["sd"].astype(F), inside=z["inside"].astype(bool), votes=z["votes"].astype(np.uint8))


def ball_points(n=200, seed=3):
    """n points with |p| < 0.7 (inside the ball of radius 0.8, whatever its facets cut off) and n with 0.9 < |p| < 1.3."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(2 * n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    r = np.concatenate([0.69 * rng.random(n) ** (1 / 3), rng.uniform(0.91, 1.3, n)])
    return (d * r[:, None]).astype(F)


def box_mesh(lo, hi):
    """The closed axis-aligned box [lo, hi], 12 triangles wound outward."""
    c = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for k in (0, 1) for j in (0, 1) for i in (0, 1)], dtype=F)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    tri = np.array([t for a, b, cc, d in quads for t in ((a, b, cc), (a, cc, d))], dtype=np.int32)
    return c, tri


def box_points(scene, seed=1):
    """Of cref.scene_box (the box [-1, 1]^3): its centre, points near its corners inside, and as many outside it."""
    rng = np.random.default_rng(seed)
    s = np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], dtype=np.float64)
    inner = np.concatenate([[[0, 0, 0]], scene["point"], 0.97 * s + rng.uniform(-0.02, 0.02, (8, 3))])
    outer = np.concatenate([1.03 * s + rng.uniform(-0.02, 0.02, (8, 3)), [[1.1, 0.1, 0.2], [0.3, -1.2, 0.9]]])
    return inner.astype(F), outer.astype(F)
