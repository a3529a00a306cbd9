"""The definitions of include/nerf_fl_amd.h, "mesh cast", restated in numpy: one operation per header operation, fp64 where
the header is fp64 and np.float32 where it rounds, so that the GPU tests can hold the kernels to the bit (the library is built
with -ffp-contract=off).  The ray test; the brute cast with the (tf, index) order; the grid cast by THE WALK of the header, slab
by slab, with the same bounds and the same stopping rule (Python floats are IEEE doubles, every operation rounded on its own);
the occlusion directions and counts.  No torch, no library."""
import math

import numpy as np

import meshdist_ref as dref

F = np.float32
D = np.float64
U64 = np.uint64
INF = F(np.inf)
FIRST, ANY = 0, 1
TWO_M19, TWO_M20, TWO_M21, TWO_M23, TWO_M40, TWO_M148 = 2.0 ** -19, 2.0 ** -20, 2.0 ** -21, 2.0 ** -23, 2.0 ** -40, 2.0 ** -148
MAX_DIRECTIONS, ATTEMPTS = 4096, 8


# ---- the grid's faces and box

def face(lo, cell, i):
    """(F, S) of the face at index i of an axis that starts at lo: fp64."""
    lo, ic = float(F(lo)), float(i) * float(F(cell))
    return lo + ic, TWO_M21 * (abs(lo) + ic)


def box_of(lo, cell, dims):
    """The closed box of a grid in fp64: (lo (3,), hi (3,))."""
    return (np.array([face(lo[k], cell, 0)[0] for k in range(3)]), np.array([face(lo[k], cell, dims[k])[0] for k in range(3)]))


def valid(rays):
    """(N,) bool: a ray that can hit something."""
    r = np.asarray(rays, dtype=F).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        return np.isfinite(r[:, :6]).all(axis=1) & (r[:, 6] <= r[:, 7]) & (r[:, 3:6] != 0).any(axis=1)


# ---- THE RAY TEST

def ray_triangle(rays, a, b, c, box=None):
    """Rays (N, 8) against ONE usable triangle: hit (N,) bool, tf (N,), bary (N, 3), qf (N, 3); the last three mean something
    where hit."""
    r = np.asarray(rays, dtype=F).reshape(-1, 8)
    a32, b32, c32 = (np.asarray(v, dtype=F).reshape(1, 3) for v in (a, b, c))
    O, Dr, near, far = r[:, :3].astype(D), r[:, 3:6].astype(D), r[:, 6], r[:, 7]
    A, B, C = a32.astype(D), b32.astype(D), c32.astype(D)
    one = D(1)
    with np.errstate(all="ignore"):
        e1, e2 = B - A, C - A
        p = dref.cross(Dr, e2)
        det = dref.dot(e1, p)
        s = O - A
        u = dref.dot(s, p) / det
        q = dref.cross(s, e1)
        v, t = dref.dot(Dr, q) / det, dref.dot(e2, q) / det
        ok = (det != 0) & ~np.isnan(det) & (u >= 0) & (v >= 0) & (u + v <= one)
        tf = t.astype(F)
        ok &= np.isfinite(tf) & (near <= tf) & (tf <= far)
        Q = (A + u[:, None] * e1) + v[:, None] * e2
        tri = np.concatenate([a32, b32, c32])
        mn, mx = tri.min(axis=0)[None], tri.max(axis=0)[None]
        qf = Q.astype(F)
        qf = np.where(qf < mn, mn, np.where(qf > mx, mx, qf)).astype(F)
        td = t[:, None] * Dr
        rr = O + td
        tol = TWO_M20 * (np.abs(O) + np.abs(td)).max(axis=1)
        qd = qf.astype(D)
        ok &= (np.abs(rr - qd) <= tol[:, None]).all(axis=1)                 # THE CONSISTENCY CONDITION
        if box is not None:
            ok &= ((qd >= box[0][None]) & (qd <= box[1][None])).all(axis=1)   # THE BOX RULE
        bary = np.stack([(one - u) - v, u, v], axis=1).astype(F)
    return ok & valid(r), tf, bary, qf


def _empty(N):
    return {"t": np.full(N, INF, dtype=F), "triangle": np.full(N, -1, dtype=np.int32),
            "bary": np.full((N, 3), np.nan, dtype=F), "point": np.full((N, 3), np.nan, dtype=F)}


def cast(rays, ver, tri, box=None, mode=FIRST):
    """Brute force, the (tf, index) order.  mode=ANY: `t` alone, 0 or +inf."""
    r = np.asarray(rays, dtype=F).reshape(-1, 8)
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    out = _empty(len(r))
    for t in np.nonzero(dref.usable(ver, tri))[0]:                         # ascending: a tie keeps the lower index
        hit, tf, bary, qf = ray_triangle(r, *ver[tri[t]], box=box)
        take = hit & (tf < out["t"])
        out["t"][take], out["triangle"][take], out["bary"][take], out["point"][take] = tf[take], t, bary[take], qf[take]
    return out if mode == FIRST else {"t": np.where(out["triangle"] >= 0, F(0), INF).astype(F)}


# ---- THE WALK

def table(rays, ver, tri, box):
    """The ray test of every ray against every usable triangle, once: {triangle: (hit, tf, bary, qf)}.  The test is a function of
    the ray, the triangle and the box alone, so the walk below may look its results up instead of repeating them."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    return {int(t): ray_triangle(rays, *ver[tri[t]], box=box) for t in np.nonzero(dref.usable(ver, tri))[0]}


def rows_of(ver, tri, lo, cell, dims):
    """The grid's rows as a dict {cell number: [triangles]} of the cells that list any."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    rows = {}
    for t in np.nonzero(dref.usable(ver, tri))[0]:
        c = ver[tri[t]]
        i0 = [int(dref.cellf(c[:, k].min(), lo[k], cell, dims[k])) for k in range(3)]
        i1 = [int(dref.cellf(c[:, k].max(), lo[k], cell, dims[k])) for k in range(3)]
        for z in range(i0[2], i1[2] + 1):
            for y in range(i0[1], i1[1] + 1):
                for x in range(i0[0], i1[0] + 1):
                    rows.setdefault((z * dims[1] + y) * dims[0] + x, []).append(int(t))
    return rows


def _down(x):
    with np.errstate(over="ignore"):
        f = F(x)
    return np.nextafter(f, F(-np.inf)) if float(f) > x else f


def _up(x):
    with np.errstate(over="ignore"):
        f = F(x)
    return np.nextafter(f, F(np.inf)) if float(f) < x else f


def _cell1(x32, lo32, cell32, n):
    with np.errstate(all="ignore"):
        f = np.floor((x32 - lo32) / cell32)
    return int(min(max(f, F(0)), F(n - 1)))


def _floor(x):
    return x if math.isinf(x) else float(math.floor(x))


def walk(ray, lo, cell, dims, box, rows, tests, r, mode=FIRST, visits=None):
    """THE WALK for ray number r (`ray`: its 8 floats): (tf, triangle) of the answer, (+inf, -1) without one.  `tests` is
    table()'s; `visits`, a list, receives the cells in the order they are read."""
    o, d = [float(x) for x in ray[:3]], [float(x) for x in ray[3:6]]
    near, far = float(ray[6]), float(ray[7])
    lo32, cell32 = [F(x) for x in lo], F(cell)
    m, am = 0, abs(d[0])
    if abs(d[1]) > am:
        m, am = 1, abs(d[1])
    if abs(d[2]) > am:
        m = 2
    k1 = 0 if m == 2 else m + 1
    k2 = 0 if k1 == 2 else k1 + 1
    omax = max(abs(o[0]), abs(o[1]), abs(o[2]))
    bmax = max(max(abs(float(box[0][k])), abs(float(box[1][k]))) for k in range(3))
    E = TWO_M19 * (2.0 * omax + bmax)
    tn = near - (abs(near) * TWO_M23 + TWO_M148)
    tfar = far + (abs(far) * TWO_M23 + TWO_M148)
    up = d[m] > 0.0
    nm = dims[m]
    Sn = face(lo[m], cell, nm)[1]
    r0, Et, lom = o[m] + tn * d[m], E + Sn, float(box[0][m])
    c64 = float(cell32)
    guess = _floor(((r0 - Et) - lom) / c64) - 2.0 if up else _floor(((r0 + Et) - lom) / c64) + 2.0
    i = int(min(max(guess, 0.0), float(nm - 1)))
    best_tf, best_t = INF, -1

    def span(k, ta, tb):
        xa, xb = o[k] + ta * d[k], o[k] + tb * d[k]
        return (_cell1(_down(min(xa, xb) - E), lo32[k], cell32, dims[k]), _cell1(_up(max(xa, xb) + E), lo32[k], cell32, dims[k]))

    while 0 <= i < nm:
        (F0, S0), (F1, S1) = face(lo[m], cell, i), face(lo[m], cell, i + 1)
        low, high = (F0 - S0) - E, (F1 + S1) + E
        te, tx = ((low if up else high) - o[m]) / d[m], ((high if up else low) - o[m]) / d[m]
        if te > tfar:
            break
        if best_t >= 0 and best_tf < _down(te - abs(te) * TWO_M40):
            break
        if not tx < tn:
            ta, tb = max(te, tn), min(tx, tfar)
            a0, a1 = span(k1, ta, tb)
            b0, b1 = span(k2, ta, tb)
            for j2 in range(b0, b1 + 1):
                for j1 in range(a0, a1 + 1):
                    x, y, z = ((i, j1, j2), (j2, i, j1), (j1, j2, i))[m]
                    c = (z * dims[1] + y) * dims[0] + x
                    if visits is not None:
                        visits.append(c)
                    for t in rows.get(c, ()):
                        hit, tf, _, _ = tests[t]
                        if hit[r] and (tf[r] < best_tf or (tf[r] == best_tf and t < best_t)):
                            best_tf, best_t = tf[r], t
                        if mode == ANY and best_t >= 0:
                            return best_tf, best_t
        i += 1 if up else -1
    return best_tf, best_t


def cast_grid(rays, ver, tri, lo, cell, dims, mode=FIRST):
    """The grid cast: cast()'s dict, found by THE WALK.  Also returns the largest number of cells one ray read."""
    r = np.asarray(rays, dtype=F).reshape(-1, 8)
    lo, cell = [float(F(x)) for x in lo], float(F(cell))
    box = box_of(lo, cell, dims)
    rows, tests = rows_of(ver, tri, lo, cell, dims), table(r, ver, tri, box)
    out, ok, most = _empty(len(r)), valid(r), 0
    for n in np.nonzero(ok)[0]:
        visits = []
        _, t = walk(r[n], lo, cell, dims, box, rows, tests, n, mode, visits)
        most = max(most, len(visits))
        if t >= 0:
            _, tf, bary, qf = tests[t]
            out["t"][n], out["triangle"][n], out["bary"][n], out["point"][n] = tf[n], t, bary[n], qf[n]
    if mode == ANY:
        out = {"t": np.where(out["triangle"] >= 0, F(0), INF).astype(F)}
    return out, most


# ---- occlusion

def directions(seed, i, normal, K):
    """(K, 3) fp32: DIRECTION j = 0 .. K - 1 of point i with normal `normal`."""
    n = np.asarray(normal, dtype=F).reshape(3)
    with np.errstate(over="ignore"):
        h = dref.mix(dref.mix(dref.mix(np.array([seed], dtype=U64)) + U64(i)) + np.arange(K, dtype=U64))
    x, y, s = np.zeros(K, dtype=F), np.zeros(K, dtype=F), np.zeros(K, dtype=F)
    todo = np.ones(K, dtype=bool)
    for attempt in range(ATTEMPTS):
        with np.errstate(over="ignore"):
            ha = dref.mix(h + U64(attempt + 1))
        cx = (ha >> U64(40)).astype(F) * F(TWO_M23) - F(1)
        cy = ((ha >> U64(16)) & U64(0xFFFFFF)).astype(F) * F(TWO_M23) - F(1)
        cs = cx * cx + cy * cy
        take = todo & (cs < F(1))
        x[take], y[take], s[take] = cx[take], cy[take], cs[take]
        todo &= ~take
    z = np.sqrt(F(1) - s)
    with np.errstate(all="ignore"):
        sg = np.copysign(F(1), n[2])
        a = F(-1) / (sg + n[2])
        b = (n[0] * n[1]) * a
        t1 = np.array([F(1) + ((sg * n[0]) * n[0]) * a, sg * b, -(sg * n[0])], dtype=F)
        t2 = np.array([b, sg + (n[1] * n[1]) * a, -n[1]], dtype=F)
        d = (x[:, None] * t1[None] + y[:, None] * t2[None]) + z[:, None] * n[None]
    return d.astype(F)


def occlusion(points, normals, ver, tri, lo, cell, dims, K, radius, bias, seed):
    """hits (N,) int32 and open (N,) fp32.  Counted with the brute cast inside the grid's box: by THE CONTRACT the walk, which
    the kernel uses, hits exactly when it does."""
    p, nrm = np.asarray(points, dtype=F).reshape(-1, 3), np.asarray(normals, dtype=F).reshape(-1, 3)
    box = box_of([float(F(x)) for x in lo], float(F(cell)), dims)
    hits, opn = np.full(len(p), -1, dtype=np.int32), np.full(len(p), np.nan, dtype=F)
    ok = [i for i in range(len(p)) if np.isfinite(p[i]).all() and np.isfinite(nrm[i]).all() and nrm[i].any()]
    if not ok:
        return hits, opn
    rays = []
    for i in ok:
        with np.errstate(all="ignore"):
            o = p[i] + F(bias) * nrm[i]
        rays.append(np.concatenate([np.tile(o, (K, 1)), directions(seed, i, nrm[i], K), np.zeros((K, 1), F),
                                    np.full((K, 1), F(radius))], axis=1).astype(F))
    hit = (cast(np.concatenate(rays), ver, tri, box, ANY)["t"] == 0).reshape(len(ok), K)
    hits[ok] = hit.sum(axis=1)
    opn[ok] = (F(K) - hits[ok].astype(F)) / F(K)
    return hits, opn


# ---- the scenes and rays that test_meshcast_cpu.py and test_meshcast_gpu.py share

ORIGINS = {"round": (-3.0, -2.0, -7.0), "odd": (-3.1, -2.3, -7.7)}           # the second: offsets fp32 does not hold
CELLS = (0.1, 0.2, 0.25, 1.0 / 3.0, 1.0)
SPAN = (8.4, 4.6, 6.9)


def dims_of(cell):
    return [int(np.ceil(s / cell)) for s in SPAN]


def configs():
    """(name, lo, cell, dims): five cell sizes at two origins, one cell holding everything, and one that does not."""
    out = [((o, c), ORIGINS[o], c, dims_of(c)) for o in sorted(ORIGINS) for c in CELLS]
    return out + [(("all", 100.0), (-50.0, -50.0, -50.0), 100.0, [1, 1, 1]), (("part", 100.0), ORIGINS["odd"], 100.0, [1, 1, 1])]


def soup40():
    """The 40 triangles of test_meshdist_gpu.py: 36 of the seeded soup, a unit square of two at z = -4 (a tie along their
    shared edge), and one triangle twice (a tie everywhere)."""
    import meshcolor_ref as mref
    ver, tri = mref.soup(40, 7)
    ver, tri = ver.copy(), tri.copy()
    ver[3 * 36:3 * 36 + 3] = [[4, 0, -4], [5, 0, -4], [5, 1, -4]]
    ver[3 * 37:3 * 37 + 3] = [[4, 0, -4], [5, 1, -4], [4, 1, -4]]
    tri[39] = tri[38]
    return ver, tri


def soup_rays(ver, tri, seed=5):
    """About 400 rays of seven kinds: random; axis-aligned; through vertices; through edges (the square's shared edge among
    them); starting on cell faces of every configuration; lying in a cell plane; with near and far that cut hits off -- and
    a handful that can hit nothing."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array([-3.5, -2.5, -7.5]), np.array([5.5, 2.5, -0.5])
    inf = np.inf
    rays = []

    def add(o, d, near=0.0, far=inf):
        rays.append(np.concatenate([np.asarray(o, dtype=F), np.asarray(d, dtype=F), F([near, far])]))

    def aimed(target, back=3.0):                                              # a ray through `target`, in fp32
        d = rng.normal(size=3)
        o = (np.asarray(target, dtype=D) - back * d / np.linalg.norm(d)).astype(F)
        return o, np.asarray(target, dtype=F) - o

    for _ in range(70):                                                       # 1 random: anywhere, and at the triangles
        add(rng.uniform(lo, hi), rng.normal(size=3))
    for t in rng.integers(0, len(tri), 60):
        w = rng.dirichlet(np.ones(3))
        add(*aimed(w @ ver[tri[t]].astype(D), back=rng.uniform(0.5, 6.0)))
    for k in range(3):                                                        # 2 axis-aligned, from outside and from inside
        for s in (1.0, -1.0):
            for _ in range(6):
                o = rng.uniform(lo, hi)
                o[k] = -12.0 * s if rng.random() < 0.5 else o[k]
                add(o, np.eye(3)[k] * s * rng.choice([1.0, 0.5, 3.0]))
    for v in rng.choice(len(ver), 30, replace=False):                         # 3 through vertices
        add(*aimed(ver[v]))
    for t in rng.choice(len(tri), 24, replace=False):                         # 4 through edges
        a, b = ver[tri[t][0]].astype(D), ver[tri[t][1]].astype(D)
        add(*aimed(a + rng.random() * (b - a)))
    for x in (0.25, 0.5, 0.75):                                               # the square's shared edge, head-on and aslant
        add([4 + x, x, -3], [0, 0, -1])
        add([4 + x, x, -5], [0, 0, 2])
        add([4 + x - 0.5, x, -3.5], [1, 0, -1])
    for _, glo, cell, dims in configs():                                      # 5 starting on cell faces, 6 lying in a cell plane
        for i in (0, 1, dims[0] // 2, dims[0]):
            f = [F(glo[k]) + F(min(i, dims[k])) * F(cell) for k in range(3)]
            add(f, rng.normal(size=3))
            k = int(rng.integers(3))
            o, d = rng.uniform(lo, hi).astype(F), rng.normal(size=3)
            o[k], d[k] = f[k], 0.0
            add(o, d)
    for _ in range(50):                                                       # 7 near and far
        o, d = rng.uniform(lo, hi), rng.normal(size=3)
        a, b = np.sort(rng.uniform(-2.0, 6.0, 2))
        add(o, d, a, b)
    add([0, 0, 0], [0, 0, -1], -inf, inf)
    add([0, 0, -9], [0.1, 0.05, 1], -inf, 0.0)
    add([0, 0, 0], [0, 0, -1], 2.0, 2.0)
    add([0, 0, 0], [0, 0, 0])                                                 # nothing to hit with
    add([0, 0, 0], [0, 0, -1], 3.0, 2.0)
    add([np.nan, 0, 0], [0, 0, -1])
    add([0, 0, 0], [0, np.inf, -1])
    add([0, 0, 0], [0, 0, -1], np.nan, inf)
    add([0, 0, 0], [0, 0, -1], 0.0, np.nan)
    return np.stack(rays).astype(F)


def _quads(quads):
    """Quads (each four corners in order) as a mesh of two triangles each."""
    ver = np.array([c for q in quads for c in q], dtype=F)
    tri = np.array([[4 * i + a, 4 * i + b, 4 * i + c] for i in range(len(quads)) for a, b, c in ((0, 1, 2), (0, 2, 3))], dtype=np.int32)
    return ver, tri


def scene_square():
    """A lone square, and a point on it with its normal up: open = 1."""
    ver, tri = _quads([[(-1, -1, 0), (1, -1, 0), (1, 1, 0), (-1, 1, 0)]])
    return dict(ver=ver, tri=tri, lo=(-1.5, -1.5, -0.5), cell=0.5, dims=[6, 6, 4], point=F([[0.1, 0.2, 0.0]]), normal=F([[0, 0, 1]]))


def scene_box():
    """A closed box, and a point inside it: open = 0."""
    c = [(x, y, z) for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)]
    faces = [(0, 1, 3, 2), (4, 5, 7, 6), (0, 1, 5, 4), (2, 3, 7, 6), (0, 2, 6, 4), (1, 3, 7, 5)]
    ver, tri = _quads([[c[i] for i in f] for f in faces])
    nrm = F([[0.36, 0.48, 0.8]])
    return dict(ver=ver, tri=tri, lo=(-1.25, -1.25, -1.25), cell=0.5, dims=[5, 5, 5], point=F([[0.1, -0.2, 0.3]]), normal=nrm)


def scene_wall():
    """A point on a floor, 0.01 from the foot of a wall 10 high and 40 wide: the wall takes the half of the hemisphere towards
    it, but for the cap of directions steeper than 1000 : 1 -- a cosine-weighted share of 1e-6."""
    ver, tri = _quads([[(-20, -20, 0), (20, -20, 0), (20, 20, 0), (-20, 20, 0)], [(0.01, -20, 0), (0.01, 20, 0), (0.01, 20, 10), (0.01, -20, 10)]])
    return dict(ver=ver, tri=tri, lo=(-20.5, -20.5, -0.5), cell=1.0, dims=[41, 41, 11], point=F([[0, 0, 0]]), normal=F([[0, 0, 1]]))
