"""The definitions of include/nerf_fl_amd.h, "registration", restated in numpy: one numpy operation per header operation, fp64
where the header is fp64 (all of it but the face normal), so that the GPU tests can hold the kernels to the bit (the library
is built with -ffp-contract=off).  The moments row in its fixed order of additions, both solves, apply, and the ICP loop over
meshdist_ref.closest, put together the way nerf_fl_amd.registration does; the height field and the displaced problems the CPU
and the GPU tests share.  No torch, no library."""
import numpy as np

import meshdist_ref as dref

F = np.float32
D = np.float64
INF = F(np.inf)
POINT, PLANE = 0, 1
OK, FEW, SINGULAR = 0, 1, 2
COUNT, SUM_DD, SUM_P, SUM_Q, SUM_PP, SUM_QQ, SUM_PQ, ATA, ATB, SUM_RR, COLUMNS = 0, 1, 2, 5, 8, 9, 10, 19, 47, 54, 55
IDENTITY = np.array([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])

# Bounds the CPU and the GPU tests share.  MEASURED on this restatement and not derived, each with a margin; the measurements
# are in the docstring of tests/test_registration_cpu.py, which prints them anew
RECOVERED = (6e-6, 8e-8, 3e-8)              # degrees, translation, scale after 8 iterations of plane mode: 10 x the measured
PLANE_VS_LSTSQ = 100 * 6.2e-17              # an unknown of the plane solve against numpy.linalg.lstsq: 100 x the measured
POINT_VS_SVD = 100 * 1.4e-15                # one of the 13 doubles of the point solve against the SVD solution: 100 x the measured
REGISTERED_CHAMFER = 10 * 5.9e-9            # Chamfer distance of the displaced height field to itself once registered: 10 x


# ---- apply

def apply(x, T, vectors=False):
    """nfl_register_apply: (N, 3) fp32 under the 13 doubles T."""
    x = np.asarray(x, dtype=F).reshape(-1, 3).astype(D)
    T = np.asarray(T, dtype=D)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        for k in range(3):
            y = (T[1 + 3 * k] * x[:, 0] + T[2 + 3 * k] * x[:, 1]) + T[3 + 3 * k] * x[:, 2]
            out[:, k] = y if vectors else T[0] * y + T[10 + k]
        return out.astype(F)


# ---- the moments row

def unit_face_normals(ver, tri):
    """(T, 3) fp32 and (T,) bool: cross(ab, ac) / len in fp32, and whether the triangle is usable with 0 < len < inf."""
    ver, tri = np.asarray(ver, dtype=F).reshape(-1, 3), np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    if len(ver) == 0 or len(tri) == 0:
        return np.zeros((len(tri), 3), F), np.zeros(len(tri), bool)
    ok = dref.usable(ver, tri)
    c = ver[np.where(ok[:, None], tri, 0)]
    with np.errstate(all="ignore"):
        cr = dref.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
        ln = np.sqrt(dref.dot(cr, cr))
        has = ok & (ln > 0) & (ln < INF)
        nf = np.where(has[:, None], cr / ln[:, None], F(0)).astype(F)
    return nf, has


def fixed_order_sum(terms):
    """(n, K) fp64, the rows of elements that do not count all +0.0 -> (K,): nfl_meshdist_reduce's order of additions.  Adding
    +0.0 where the kernel adds nothing gives the kernel's bits: a sum that starts at +0.0 is never -0.0."""
    n, K = terms.shape
    G = min((n + 255) // 256, 1024)
    if G == 0:
        return np.zeros(K)
    J = (n + G * 256 - 1) // (G * 256)
    pad = np.zeros((J * G * 256, K))
    pad[:n] = terms
    pad = pad.reshape(J, G, 256, K)                                     # element (g + j G) * 256 + t
    acc = np.zeros((G, 256, K))
    for j in range(J):
        acc = acc + pad[j]

    def fold(red):
        red = red.copy()
        off = 128
        while off:
            red[..., :off, :] = red[..., :off, :] + red[..., off:2 * off, :]
            off //= 2
        return red[..., 0, :]

    parts = fold(acc)                                                   # (G, K)
    fin = np.zeros((256, K))
    for i in range(G):                                                  # thread i % 256 adds rows i, i + 256, ... in order
        fin[i % 256] = fin[i % 256] + parts[i]
    return fold(fin)


def counting(points, closest, triangle, distance, ver, tri, max_distance):
    """(n,) bool: the pairs that count, and the unit normals of their triangles (zeros elsewhere)."""
    P, Q = np.asarray(points, dtype=F).reshape(-1, 3), np.asarray(closest, dtype=F).reshape(-1, 3)
    ok = np.isfinite(P).all(axis=1) & np.isfinite(Q).all(axis=1)
    if distance is not None:
        d = np.asarray(distance, dtype=F).reshape(-1)
        with np.errstate(invalid="ignore"):
            ok &= (d < INF) & (d <= F(max_distance))
    N = np.zeros((len(P), 3), F)
    if triangle is not None:
        t = np.asarray(triangle, dtype=np.int32).reshape(-1)
        nf, has = unit_face_normals(ver, tri)
        inside = (t >= 0) & (t < len(has))
        ok &= inside
        if len(has):
            ok &= has[np.where(inside, t, 0)]
            N = np.where(ok[:, None], nf[np.where(inside, t, 0)], F(0))
    return ok, N


def moments(points, closest, triangle, distance, ver, tri, mode, max_distance, centre):
    """The (55,) fp64 row of nfl_register_moments."""
    P, Q = np.asarray(points, dtype=F).reshape(-1, 3).astype(D), np.asarray(closest, dtype=F).reshape(-1, 3).astype(D)
    n = len(P)
    ok, N = counting(points, closest, triangle, distance, ver, tri, max_distance)
    c = np.asarray(centre, dtype=D)
    terms = np.zeros((n, COLUMNS))
    with np.errstate(all="ignore"):
        p, q, e = P - c, Q - c, P - Q
        dd = (e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]
        if distance is not None:
            d = np.asarray(distance, dtype=F).reshape(-1).astype(D)
            dd = d * d
        terms[:, COUNT], terms[:, SUM_DD] = 1.0, dd
        if mode == POINT:
            terms[:, SUM_P:SUM_P + 3], terms[:, SUM_Q:SUM_Q + 3] = p, q
            terms[:, SUM_PP] = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
            terms[:, SUM_QQ] = (q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]
            for i in range(3):
                for j in range(3):
                    terms[:, SUM_PQ + 3 * i + j] = p[:, i] * q[:, j]
        else:
            N = N.astype(D)
            a = [p[:, 1] * N[:, 2] - p[:, 2] * N[:, 1], p[:, 2] * N[:, 0] - p[:, 0] * N[:, 2], p[:, 0] * N[:, 1] - p[:, 1] * N[:, 0],
                 N[:, 0], N[:, 1], N[:, 2], (p[:, 0] * N[:, 0] + p[:, 1] * N[:, 1]) + p[:, 2] * N[:, 2]]
            r = (N[:, 0] * e[:, 0] + N[:, 1] * e[:, 1]) + N[:, 2] * e[:, 2]
            at = ATA
            for i in range(7):
                for j in range(i, 7):
                    terms[:, at] = a[i] * a[j]
                    at += 1
            for i in range(7):
                terms[:, ATB + i] = a[i] * r
            terms[:, SUM_RR] = r * r
    terms = np.where(ok[:, None], terms, 0.0)
    return fixed_order_sum(terms)


# ---- the solves

def rot(w, x, y, z):
    xx, yy, zz, xy, xz, yz, wx, wy, wz = x * x, y * y, z * z, x * y, x * z, y * z, w * x, w * y, w * z
    two, one = D(2), D(1)
    return np.array([one - two * (yy + zz), two * (xy - wz), two * (xz + wy),
                     two * (xy + wz), one - two * (xx + zz), two * (yz - wx),
                     two * (xz - wy), two * (yz + wx), one - two * (xx + yy)])


def mul(R, x):
    return [(R[3 * i] * x[0] + R[3 * i + 1] * x[1]) + R[3 * i + 2] * x[2] for i in range(3)]


def solve_point(row, with_scale, c):
    """(ds, dR (9,), dt [3]) or None: POINT of the header."""
    n = row[COUNT]
    mp, mq = [row[SUM_P + k] / n for k in range(3)], [row[SUM_Q + k] / n for k in range(3)]
    M = [[row[SUM_PQ + 3 * i + j] - row[SUM_P + i] * mq[j] for j in range(3)] for i in range(3)]
    A = np.zeros((4, 4))
    A[0, 0] = (M[0][0] + M[1][1]) + M[2][2]
    A[1, 1] = (M[0][0] - M[1][1]) - M[2][2]
    A[2, 2] = (M[1][1] - M[0][0]) - M[2][2]
    A[3, 3] = (M[2][2] - M[0][0]) - M[1][1]
    A[0, 1] = A[1, 0] = M[1][2] - M[2][1]
    A[0, 2] = A[2, 0] = M[2][0] - M[0][2]
    A[0, 3] = A[3, 0] = M[0][1] - M[1][0]
    A[1, 2] = A[2, 1] = M[0][1] + M[1][0]
    A[1, 3] = A[3, 1] = M[2][0] + M[0][2]
    A[2, 3] = A[3, 2] = M[1][2] + M[2][1]
    V = np.eye(4)
    one = D(1)
    for _ in range(12):
        for P, Q in ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)):
            g = A[P, Q]
            if g == 0.0:
                continue
            theta = (A[Q, Q] - A[P, P]) / (D(2) * g)
            sgn = one if theta >= 0.0 else -one
            t = sgn / (np.abs(theta) + np.sqrt(theta * theta + one))
            cs = one / np.sqrt(t * t + one)
            sn = t * cs
            A[P, P] = A[P, P] - t * g
            A[Q, Q] = A[Q, Q] + t * g
            A[P, Q] = A[Q, P] = 0.0
            for r in range(4):
                if r != P and r != Q:
                    arp, arq = A[r, P], A[r, Q]
                    A[r, P] = A[P, r] = cs * arp - sn * arq
                    A[r, Q] = A[Q, r] = sn * arp + cs * arq
            for r in range(4):
                vrp, vrq = V[r, P], V[r, Q]
                V[r, P] = cs * vrp - sn * vrq
                V[r, Q] = sn * vrp + cs * vrq
    best, v = A[0, 0], V[:, 0].copy()
    for m in range(1, 4):
        if A[m, m] > best:
            best, v = A[m, m], V[:, m].copy()
    k = one / np.sqrt(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
    v = v * k
    if v[0] < 0.0:
        v = -v
    dR = rot(v[0], v[1], v[2], v[3])
    ds = one
    if with_scale:
        den = row[SUM_PP] - ((row[SUM_P] * mp[0] + row[SUM_P + 1] * mp[1]) + row[SUM_P + 2] * mp[2])
        if not den > 0.0:
            return None
        num = D(0)
        for i in range(3):
            for j in range(3):
                num = num + dR[3 * i + j] * M[j][i]
        ds = num / den
        if not ds > 0.0:
            return None
    y = mul(dR, [mp[k] + c[k] for k in range(3)])
    return ds, dR, [(mq[i] + c[i]) - ds * y[i] for i in range(3)]


def plane_unknowns(row, m):
    """x (m,) of the leading m x m system A x = -b by the header's Cholesky, or None when a pivot is not > 0."""
    start = lambda j: ATA + 7 * j - j * (j - 1) // 2
    L = np.zeros((m, m))
    for j in range(m):
        d = row[start(j)]
        for k in range(j):
            d = d - L[j, k] * L[j, k]
        if not d > 0.0:
            return None
        L[j, j] = np.sqrt(d)
        for i in range(j + 1, m):
            v = row[start(j) + (i - j)]
            for k in range(j):
                v = v - L[i, k] * L[j, k]
            L[i, j] = v / L[j, j]
    y, x = np.zeros(m), np.zeros(m)
    for i in range(m):
        v = -row[ATB + i]
        for k in range(i):
            v = v - L[i, k] * y[k]
        y[i] = v / L[i, i]
    for i in range(m - 1, -1, -1):
        v = y[i]
        for k in range(i + 1, m):
            v = v - L[k, i] * x[k]
        x[i] = v / L[i, i]
    return x


def solve_plane(row, with_scale, c):
    """(ds, dR, dt) or None: PLANE of the header."""
    x = plane_unknowns(row, 7 if with_scale else 6)
    if x is None:
        return None
    one = D(1)
    h0, h1, h2 = D(0.5) * x[0], D(0.5) * x[1], D(0.5) * x[2]
    k = one / np.sqrt(((one + h0 * h0) + h1 * h1) + h2 * h2)
    dR = rot(k, h0 * k, h1 * k, h2 * k)
    ds = one
    if with_scale:
        ds = one + x[6]
        if not ds > 0.0:
            return None
    yc = mul(dR, c)
    return ds, dR, [(c[i] + x[3 + i]) - ds * yc[i] for i in range(3)]


def solve(row, mode, with_scale, min_pairs, centre, T):
    """nfl_register_solve: (the new 13 doubles, the history row of 4)."""
    row, T, c = np.asarray(row, dtype=D), np.asarray(T, dtype=D).copy(), [D(v) for v in centre]
    with np.errstate(all="ignore"):
        count = row[COUNT]
        rms = np.sqrt(row[SUM_DD] / count)
        status = OK
        if not count >= D(min_pairs):
            status = FEW
        else:
            step = solve_point(row, with_scale, c) if mode == POINT else solve_plane(row, with_scale, c)
            new = None
            if step is not None:
                ds, dR, dt = step
                new = np.empty(13)
                new[0] = ds * T[0]
                for i in range(3):
                    for j in range(3):
                        new[1 + 3 * i + j] = (dR[3 * i] * T[1 + j] + dR[3 * i + 1] * T[4 + j]) + dR[3 * i + 2] * T[7 + j]
                y = mul(dR, T[10:13])
                for i in range(3):
                    new[10 + i] = ds * y[i] + dt[i]
                if not np.isfinite(new).all():
                    new = None
            if new is None:
                status = SINGULAR
            else:
                T = new
    return T, np.array([count, rms, D(status), T[0]])


# ---- the loop, as nerf_fl_amd.registration.register_mesh runs it

def box_centre(p):
    p = np.asarray(p, dtype=F).reshape(-1, 3)
    p = p[np.isfinite(p).all(axis=1)].astype(D)
    if len(p) == 0:
        return [0.0, 0.0, 0.0]
    lo, hi = p.min(axis=0), p.max(axis=0)
    return [float(0.5 * (lo[k] + hi[k])) for k in range(3)]


def register(src, ver, tri, initial=None, mode=PLANE, scale=False, iterations=30, max_distance=None, min_pairs=6):
    """(the 13 doubles, the (iterations, 4) history) of the ICP loop on the points `src` against the mesh (ver, tri)."""
    T = IDENTITY.copy() if initial is None else np.asarray(initial, dtype=D).copy()
    limits = max_distance if isinstance(max_distance, (list, tuple)) else [max_distance] * iterations
    limits = [np.inf if m is None else m for m in limits]
    moved = apply(src, T)
    centre = box_centre(moved)
    history = np.zeros((iterations, 4))
    for it in range(iterations):
        if it:
            moved = apply(src, T)
        got = dref.closest(moved, ver, tri, limits[it])
        row = moments(moved, got["point"], got["triangle"], got["distance"], ver, tri, mode, limits[it], centre)
        T, history[it] = solve(row, mode, scale, min_pairs, centre, T)
    return T, history


def fit(points, targets, scale=False):
    """nerf_fl_amd.registration.fit_transform: the 13 doubles and the history row."""
    centre = box_centre(points)
    row = moments(points, targets, None, None, None, None, POINT, np.inf, centre)
    return solve(row, POINT, scale, 3, centre, IDENTITY)


# ---- transforms on the host, in fp64

def rotation(axis, degrees):
    """Rodrigues' formula: the (3, 3) rotation by `degrees` about `axis`."""
    a = np.asarray(axis, dtype=D)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.deg2rad(degrees)
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def pack(s, R, t):
    return np.concatenate([[s], np.asarray(R, dtype=D).reshape(9), np.asarray(t, dtype=D).reshape(3)])


def inverse(T):
    s, R, t = T[0], np.asarray(T[1:10]).reshape(3, 3), np.asarray(T[10:13])
    return pack(1.0 / s, R.T, -(R.T @ t) / s)


def angle_between(Ra, Rb):
    """The angle of Ra Rb^T in degrees."""
    c = (np.trace(np.asarray(Ra).reshape(3, 3) @ np.asarray(Rb).reshape(3, 3).T) - 1.0) / 2.0
    return float(np.rad2deg(np.arccos(np.clip(c, -1.0, 1.0))))


def errors(T, truth):
    """(angle in degrees, |t - t*|, |s - s*|) between two transforms.  A small angle is taken from the skew part of
    Ra Rb^T (arccos of a number next to 1 resolves 1e-8 rad at best)."""
    Ra, Rb = np.asarray(T[1:10]).reshape(3, 3), np.asarray(truth[1:10]).reshape(3, 3)
    E = Ra @ Rb.T
    w = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    small = float(np.rad2deg(np.arcsin(min(np.linalg.norm(w), 1.0))))
    ang = small if small < 1.0 else angle_between(Ra, Rb)
    return ang, float(np.linalg.norm(np.asarray(T[10:13]) - np.asarray(truth[10:13]))), float(abs(T[0] - truth[0]))


def umeyama(P, Q, scale):
    """numpy's SVD solution of min sum |s R P + t - Q|^2 (Umeyama 1991), in fp64: the 13 doubles."""
    P, Q = np.asarray(P, dtype=D), np.asarray(Q, dtype=D)
    mp, mq = P.mean(axis=0), Q.mean(axis=0)
    Pc, Qc = P - mp, Q - mq
    U, S, Vt = np.linalg.svd(Qc.T @ Pc)
    d = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        d[2] = -1.0
    R = U @ np.diag(d) @ Vt
    s = float((S * d).sum() / (Pc * Pc).sum()) if scale else 1.0
    return pack(s, R, mq - s * R @ mp)


# ---- the surface of the tests.  NOT a ball: a rotation of a ball about its centre is not observable

def height_field(n):
    """The mesh z = 0.3 sin(2.1 x + 0.3) cos(1.7 y) + 0.15 x y + 0.1 x^2 on [-1, 1]^2 with n x n vertices, two triangles a
    cell, wound so that the face normals point up; vertex normals from the gradient."""
    g = np.linspace(-1.0, 1.0, n)
    x, y = np.meshgrid(g, g, indexing="xy")
    z = 0.3 * np.sin(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * x * y + 0.1 * x * x
    zx = 0.63 * np.cos(2.1 * x + 0.3) * np.cos(1.7 * y) + 0.15 * y + 0.2 * x
    zy = -0.51 * np.sin(2.1 * x + 0.3) * np.sin(1.7 * y) + 0.15 * x
    nrm = np.stack([-zx, -zy, np.ones_like(z)], axis=-1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    i = (np.arange(n - 1)[:, None] * n + np.arange(n - 1)[None, :]).reshape(-1)         # the corner (row, column) of a cell
    tri = np.concatenate([np.stack([i, i + 1, i + n + 1], axis=1), np.stack([i, i + n + 1, i + n], axis=1)])
    return {"vertices": np.stack([x, y, z], axis=-1).reshape(-1, 3).astype(F), "normals": nrm.reshape(-1, 3).astype(F),
            "triangles": np.ascontiguousarray(tri, dtype=np.int32)}


def inner_mesh(mesh, bound=0.7):
    """The triangles of `mesh` whose corners all have |x|, |y| < bound, over the same vertices."""
    ver, tri = mesh["vertices"], mesh["triangles"]
    keep = (np.abs(ver[tri][:, :, :2]) < bound).all(axis=(1, 2))
    return dict(mesh, triangles=np.ascontiguousarray(tri[keep]))


def inner_samples(mesh, n, seed):
    """About n points on the inner triangles of `mesh`, drawn as nerf_fl_amd.meshdist.sample_surface(n=, seed=) draws them."""
    inner = inner_mesh(mesh)
    density = n / dref.total_area(inner["vertices"], inner["triangles"])
    return dref.samples(inner["vertices"], inner["triangles"], density, seed)[0]


def displaced(mesh, truth):
    """`mesh` under the INVERSE of the 13 doubles `truth` (fp64, rounded to fp32 once): `truth` brings it back."""
    inv = inverse(truth)
    s, R, t = inv[0], inv[1:10].reshape(3, 3), inv[10:13]
    return dict(mesh, vertices=(s * mesh["vertices"].astype(D) @ R.T + t).astype(F),
                normals=(mesh["normals"].astype(D) @ R.T).astype(F))


def problem(degrees, scale=1.0, axis=(0.3, -0.5, 0.8), translation=(0.05, -0.04, 0.03), n=600, seed=0, size=13):
    """(target mesh, source mesh, source points, truth): the inner part of height_field(size), displaced by the inverse of the
    similarity `truth` = (scale, the rotation by `degrees` about `axis`, `translation`), and about n samples of it."""
    target = height_field(size)
    truth = pack(scale, rotation(axis, degrees), translation)
    source = displaced(inner_mesh(target), truth)
    density = n / dref.total_area(source["vertices"], source["triangles"])
    return target, source, dref.samples(source["vertices"], source["triangles"], density, seed)[0], truth


DISPLACED_CHAMFER = 0.03                    # the translation of whole_problem() alone is 0.07 long, the turn moves a corner 0.2


def whole_problem(degrees=8.0, scale=1.04, axis=(0.3, -0.5, 0.8), translation=(0.05, -0.04, 0.03), size=13):
    """(target mesh, source mesh, truth): ALL of height_field(size) displaced by the inverse of `truth`."""
    target = height_field(size)
    truth = pack(scale, rotation(axis, degrees), translation)
    return target, displaced(target, truth), truth
