"""numpy fp32 restatement of nfl_tsdf_fuse, nfl_tsdf_resolve and nfl_tsdf_support (include/nerf_fl_amd.h, "depth fusion"),
operation for operation: every product, sum, quotient and square root is one fp32 numpy operation, in the header's order, so
the kernels (built with -ffp-contract=off) are held to it bit for bit.  The camera, its transform, the dot and the table are
meshcolor_ref's: the projections are nfl_mesh_blend's.

Also the fixture the tests share: the analytic depth map of a sphere, and the six cameras that look at it."""
import numpy as np

import meshcolor_ref as mref

F = np.float32


def lattice_points(lo, spacing, res):
    """(nz, ny, nx, 3) fp32: lo[k] + index[k] * spacing[k], the product and the sum rounded separately."""
    lo, sp = np.asarray(lo, dtype=F), np.asarray(spacing, dtype=F)
    x, y, z = (lo[k] + np.arange(res[k], dtype=F) * sp[k] for k in range(3))
    zz, yy, xx = np.meshgrid(z, y, x, indexing="ij")
    return np.stack([xx, yy, zz], axis=-1)


def fuse(cams, depths, lo, spacing, res, trunc, pixel_weights=None, image_weights=None, acc=None, views=None):
    """nfl_tsdf_fuse over `cams` in order.  depths[n], pixel_weights[n]: (H, W) fp32 of camera n; image_weights[n] its
    weight.  res = (nx, ny, nz).  Continues `acc` (nz, ny, nx, 2) and `views` (nz, ny, nx) when given.  Returns (acc, views)."""
    nx, ny, nz = res
    p = lattice_points(lo, spacing, res).reshape(-1, 3)
    P = p.shape[0]
    acc = np.zeros((P, 2), dtype=F) if acc is None else np.array(acc, dtype=F).reshape(P, 2)
    views = np.zeros(P, dtype=np.int32) if views is None else np.array(views, dtype=np.int32).reshape(P)
    trunc = F(trunc)
    for n, cam in enumerate(cams):
        wi = F(1.0) if image_weights is None else F(image_weights[n])
        if not wi > 0:                                                                  # 1
            continue
        W, H, m = cam["width"], cam["height"], cam["c2w"]
        with np.errstate(all="ignore"):
            q = mref.to_camera(cam, p)
            s = -q[:, 2]
            u = cam["cx"] + cam["fx"] * (q[:, 0] / s)
            v = cam["cy"] - cam["fy"] * (q[:, 1] / s)
            ok = (s > 0) & (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1))      # 2, 3
            us, vs = np.where(ok, u, F(0.0)), np.where(ok, v, F(0.0))
            ix, iy = np.floor(us + F(0.5)).astype(np.int64), np.floor(vs + F(0.5)).astype(np.int64)
            D = np.asarray(depths[n], dtype=F).reshape(H, W)[iy, ix]
            wp = F(1.0) if pixel_weights is None else np.asarray(pixel_weights[n], dtype=F).reshape(H, W)[iy, ix]
            w = wi * wp
            ok &= (w > 0) & (D > 0)                                                     # 4
            e = [m[4 * k + 3] - p[:, k] for k in range(3)]
            dist = np.sqrt(mref.dot(e[0], e[1], e[2], e[0], e[1], e[2]))
            phi = (dist - D) / trunc
            ok &= ~(phi > 1)                                                            # 5
            phi = np.fmax(phi, F(-1.0))
            w = np.broadcast_to(w, (P,)).astype(F)
            add = np.stack([w * phi, w], axis=1)
        acc[ok] = acc[ok] + add[ok]
        views[ok] += 1
    return acc.reshape(nz, ny, nx, 2), views.reshape(nz, ny, nx)


def resolve(acc, views, min_weight, min_views=1, fill=-1.0):
    """nfl_tsdf_resolve: (lattice fp32, known uint8), shaped as `views`."""
    acc, views = np.asarray(acc, dtype=F), np.asarray(views, dtype=np.int32)
    with np.errstate(all="ignore"):
        known = (acc[..., 1] >= F(min_weight)) & (views >= min_views)
        lattice = np.where(known, acc[..., 0] / acc[..., 1], F(fill)).astype(F)
    return lattice, known.astype(np.uint8)


def support(vertices, known, lo, spacing):
    """nfl_tsdf_support: (V,) uint8, 1 where the eight lattice points around the vertex (those of its edge, face or cell)
    are all known."""
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    known = np.asarray(known)
    nz, ny, nx = known.shape
    lo, sp = np.asarray(lo, dtype=F), np.asarray(spacing, dtype=F)
    with np.errstate(all="ignore"):
        g = (ver - lo) / sp
        inside = (np.isfinite(g) & (g >= 0) & (g <= np.array([nx - 1, ny - 1, nz - 1], dtype=F))).all(axis=1)
    g = np.where(inside[:, None], g, F(0.0))
    a, b = np.floor(g).astype(np.int64), np.ceil(g).astype(np.int64)
    out = inside.copy()
    for cz in (a, b):
        for cy in (a, b):
            for cx in (a, b):
                out &= known[cz[:, 2], cy[:, 1], cx[:, 0]] != 0
    return out.astype(np.uint8)


# ---- the fixture: a sphere seen by six cameras -----------------------------------------------------------------------------

EYES = [(3, 0, 0), (0, 3, 0), (0, 0, 3), (-3, 0, 0), (0, -3, 0), (0, 0, -3)]
RADIUS = 0.8
BOX = (-1.2, 1.2)


def sphere_depth(cam, radius=RADIUS, centre=(0.0, 0.0, 0.0)):
    """(H, W) fp32: the distance from the camera centre to the sphere along every pixel's ray, +inf where it misses
    (computed in fp64 and rounded once: it is an input, not a restatement)."""
    dx, dy = mref.pixel_rays(cam)
    d = np.stack([dx, dy, -np.ones_like(dx)], axis=1).astype(np.float64)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    m = cam["c2w"].astype(np.float64).reshape(3, 4)
    d = d @ m[:, :3].T
    oc = m[:, 3] - np.asarray(centre, dtype=np.float64)
    b = d @ oc
    disc = b * b - (oc @ oc - radius * radius)
    with np.errstate(invalid="ignore"):
        t = -b - np.sqrt(disc)
    return np.where((disc >= 0) & (t > 0), t, np.inf).astype(F).reshape(cam["height"], cam["width"])


def sphere_cameras(size=33):
    """The six cameras at distance 3 on the axes, looking at the origin.  The frame holds the whole box [-1.2, 1.2]^3: its
    nearest face is 1.8 from the camera and 1.2 wide each way, tan = 2 / 3, and 0.7 * (size - 1) / 2 pixels of focal
    length put the frame's edge at tan = 1 / 1.4 > 2 / 3."""
    f, c = 0.7 * (size - 1), (size - 1) / 2
    up = lambda eye: (0.0, 0.0, 1.0) if eye[2] == 0 else (0.0, 1.0, 0.0)
    return [mref.camera(size, size, f, f, c, c, mref.look_at(eye, up=up(eye))) for eye in EYES]


def sphere_fixture(n=17, cells=3, size=33):
    """The issue's fixture: an n^3 lattice over [-1.2, 1.2]^3, trunc = `cells` spacings, the six cameras and their analytic
    depth maps.  Returns a dict: cams, depths, lo (3,), spacing (3,), res, trunc -- lo and spacing as the fp32 the kernels
    are given."""
    s = F((BOX[1] - BOX[0]) / (n - 1))
    cams = sphere_cameras(size)
    return {"cams": cams, "depths": [sphere_depth(c) for c in cams], "lo": np.full(3, BOX[0], dtype=F),
            "spacing": np.full(3, s, dtype=F), "res": (n, n, n), "trunc": F(cells) * s}


def surface_conditions(mesh, kept, radius, spacing, trunc):
    """What the issue's prototype claimed, measured on a mesh and its support flags: a dict of the figures the tests assert."""
    ver, tri = np.asarray(mesh["vertices"], dtype=np.float64), np.asarray(mesh["triangles"], dtype=np.int64)
    r = np.linalg.norm(ver, axis=1)
    kept = np.asarray(kept).astype(bool)
    kt = kept[tri].all(axis=1)
    used = np.zeros(len(ver), dtype=bool)
    used[tri[kt].reshape(-1)] = True
    V, T = int(kept.sum()), int(kt.sum())
    edges = np.sort(np.concatenate([tri[kt][:, [0, 1]], tri[kt][:, [1, 2]], tri[kt][:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    wall = r < radius - float(trunc) / 2
    return {"wall_unfiltered": int(wall.sum()), "wall_kept": int((wall & kept).sum()), "V": V, "T": T,
            "euler": V - 3 * T // 2 + T, "every_edge_twice": bool((counts == 2).all()), "T_even": T % 2 == 0,
            "orphans": int((kept & ~used).sum()),
            "worst_spacings": float(np.abs(r[kept] - radius).max() / float(spacing)) if V else 0.0}
