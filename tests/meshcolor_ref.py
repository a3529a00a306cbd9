"""numpy fp32 restatement of nfl_mesh_depth and nfl_mesh_blend (include/nerf_fl_amd.h, "mesh colour"), operation for
operation: every product, sum, quotient and square root is one fp32 numpy operation, in the header's order, so the kernels
(built with -ffp-contract=off) are held to it bit for bit.  The depth map brute-forces every triangle against every
pixel: that is what the definition says, and it owes nothing to the boxes the raster kernel walks.

A camera is a dict with the fields of nfl_image_rec that matter here: width, height, fx, fy, cx, cy, c2w (12 floats)."""
import numpy as np

F = np.float32
RECORD = np.dtype([("pix0", "<i8"), ("byte0", "<i8"), ("width", "<i4"), ("height", "<i4"), ("channels", "<i4"),
                   ("id", "<i4"), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("near", "<f4"),
                   ("far", "<f4"), ("c2w", "<f4", (12,))])


def camera(width, height, fx, fy, cx, cy, c2w=None):
    c2w = np.eye(4)[:3] if c2w is None else np.asarray(c2w, dtype=np.float64)[:3, :4]
    return {"width": int(width), "height": int(height), "fx": F(fx), "fy": F(fy), "cx": F(cx), "cy": F(cy),
            "c2w": c2w.astype(F).reshape(12)}


def cameras_of(table):
    """The cameras of a RECORD table (an ImageBank's host_table)."""
    return [camera(r["width"], r["height"], r["fx"], r["fy"], r["cx"], r["cy"], r["c2w"].reshape(3, 4)) for r in table]


def table_of(cams, channels=3):
    """A RECORD table for `cams`, pixels back to back (a free camera's record simply owns no pixels of a bank)."""
    t = np.zeros(len(cams), dtype=RECORD)
    pix = byte = 0
    for r, c in zip(t, cams):
        r["pix0"], r["byte0"], r["width"], r["height"], r["channels"] = pix, byte, c["width"], c["height"], channels
        r["fx"], r["fy"], r["cx"], r["cy"], r["c2w"] = c["fx"], c["fy"], c["cx"], c["cy"], c["c2w"]
        pix += c["width"] * c["height"]
        byte += c["width"] * c["height"] * channels
    return t


def dot(a0, a1, a2, x0, x1, x2):
    return (a0 * x0 + a1 * x1) + a2 * x2


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def to_camera(cam, p):
    """q (..., 3) = R^T (p - t) for world points p (..., 3)."""
    m = cam["c2w"]
    p = np.asarray(p, dtype=F)
    w = [p[..., k] - m[4 * k + 3] for k in range(3)]
    return np.stack([dot(m[c], m[4 + c], m[8 + c], w[0], w[1], w[2]) for c in range(3)], axis=-1)


def pixel_rays(cam):
    """(dx, dy) of every pixel, row-major (height * width,); dz is -1."""
    i = np.tile(np.arange(cam["width"], dtype=F), cam["height"])
    j = np.repeat(np.arange(cam["height"], dtype=F), cam["width"])
    return (i - cam["cx"]) / cam["fx"], -((j - cam["cy"]) / cam["fy"])


def intersect(a, b, c, dx, dy, dtype=F):
    """Moeller-Trumbore from the origin, in the header's order: camera-space vertices a, b, c (T, 3) against rays
    (dx, dy, -1) (P,).  Returns hit (T, P) bool, tau (T, P), u, v.  dtype=np.float64 gives the same algorithm in fp64."""
    a, b, c = (np.asarray(x, dtype=dtype) for x in (a, b, c))
    dx, dy = np.asarray(dx, dtype=dtype)[None, :], np.asarray(dy, dtype=dtype)[None, :]
    dz = dtype(-1.0)
    tv = [-a[:, k, None] for k in range(3)]
    e1 = [(b[:, k] - a[:, k])[:, None] for k in range(3)]
    e2 = [(c[:, k] - a[:, k])[:, None] for k in range(3)]
    qv = cross(tv, e1)
    tnum = dot(e2[0], e2[1], e2[2], qv[0], qv[1], qv[2])
    pv = cross((dx, dy, dz), e2)
    det = dot(e1[0], e1[1], e1[2], pv[0], pv[1], pv[2])
    with np.errstate(all="ignore"):
        inv = dtype(1.0) / det
        u = dot(tv[0], tv[1], tv[2], pv[0], pv[1], pv[2]) * inv
        v = dot(dx, dy, dz, qv[0], qv[1], qv[2]) * inv
        tau = tnum * inv
        hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1) & (tau > 0)
    return hit, tau, u, v


def depth_map(vertices, triangles, cam, dtype=F, chunk=256):
    """(height, width) depth of the mesh seen by `cam`: +inf where no triangle is hit."""
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    H, W = cam["height"], cam["width"]
    out = np.full(H * W, np.inf, dtype=dtype)
    V = ver.shape[0]
    tri = tri[((tri >= 0) & (tri < V)).all(axis=1)]
    if V == 0 or tri.shape[0] == 0:
        return out.reshape(H, W)
    with np.errstate(all="ignore"):
        q = to_camera(cam, ver)
        a, b, c = q[tri[:, 0]], q[tri[:, 1]], q[tri[:, 2]]
        ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
        a, b, c = a[ok], b[ok], c[ok]
        dx, dy = pixel_rays(cam)
        dx, dy = dx.astype(dtype), dy.astype(dtype)
        length = np.sqrt((dx * dx + dy * dy) + dtype(1.0))
        for t0 in range(0, a.shape[0], chunk):
            s = slice(t0, t0 + chunk)
            hit, tau, _, _ = intersect(a[s], b[s], c[s], dx, dy, dtype)
            d = np.where(hit, tau * length[None, :], dtype(np.inf))
            out = np.minimum(out, d.min(axis=0))
    return out.reshape(H, W)


def run_depth(vertices, triangles, cams):
    """The depth buffer of a run of cameras: their maps back to back, as nfl_mesh_depth lays them out."""
    if not cams:
        return np.zeros(0, dtype=F)
    return np.concatenate([depth_map(vertices, triangles, c).reshape(-1) for c in cams])


def pixel_rgb(image):
    """(H, W, 3) fp32 colours of a uint8 (H, W, 3|4) image: nfl_pixel_rgb."""
    im = np.asarray(image)
    c = im[..., :3].astype(F) / F(255.0)
    if im.shape[2] == 4:
        al = im[..., 3:4].astype(F) / F(255.0)
        c = c * al + (F(1.0) - al)
    return c


def blend(vertices, normals, cams, images, depths, depth_tol, image_weights=None, min_cos=0.0, weighting="cos",
          center=None, reject=None, sums=None, views=None):
    """nfl_mesh_blend over `cams` in order.  images[n]: uint8 (H, W, 3|4); depths[n]: (H, W) fp32.  Continues `sums`
    (V, 4) and `views` (V,) when given.  Returns (sums, views)."""
    p = np.asarray(vertices, dtype=F).reshape(-1, 3)
    nr = np.asarray(normals, dtype=F).reshape(-1, 3)
    V = p.shape[0]
    sums = np.zeros((V, 4), dtype=F) if sums is None else np.array(sums, dtype=F)
    views = np.zeros(V, dtype=np.int32) if views is None else np.array(views, dtype=np.int32)
    flat = (nr == 0).all(axis=1)
    depth_tol, min_cos = F(depth_tol), F(min_cos)
    for n, cam in enumerate(cams):
        wi = F(1.0) if image_weights is None else F(image_weights[n])
        if not wi > 0:
            continue
        W, H, m = cam["width"], cam["height"], cam["c2w"]
        with np.errstate(all="ignore"):
            q = to_camera(cam, p)
            s = -q[:, 2]
            u = cam["cx"] + cam["fx"] * (q[:, 0] / s)
            v = cam["cy"] - cam["fy"] * (q[:, 1] / s)
            ok = (s > 0) & (u >= 0) & (u <= F(W - 1)) & (v >= 0) & (v <= F(H - 1))
            e = [m[4 * k + 3] - p[:, k] for k in range(3)]
            dist = np.sqrt(dot(e[0], e[1], e[2], e[0], e[1], e[2]))
            cos = np.where(flat, F(1.0), dot(nr[:, 0], nr[:, 1], nr[:, 2], e[0], e[1], e[2]) / dist)
            ok &= cos > min_cos
            us, vs = np.where(ok, u, F(0.0)), np.where(ok, v, F(0.0))
            ix, iy = np.floor(us + F(0.5)).astype(np.int64), np.floor(vs + F(0.5)).astype(np.int64)
            ok &= dist <= np.asarray(depths[n], dtype=F)[iy, ix] + depth_tol
            xf, yf = np.floor(us), np.floor(vs)
            tx, ty = us - xf, vs - yf
            sx, sy = F(1.0) - tx, F(1.0) - ty
            xa, ya = xf.astype(np.int64), yf.astype(np.int64)
            xb, yb = np.minimum(xa + 1, W - 1), np.minimum(ya + 1, H - 1)
            rgb = pixel_rgb(images[n])
            c = ((rgb[ya, xa] * sx[:, None] + rgb[ya, xb] * tx[:, None]) * sy[:, None]
                 + (rgb[yb, xa] * sx[:, None] + rgb[yb, xb] * tx[:, None]) * ty[:, None])
            if center is not None:
                ok &= np.abs(c - np.asarray(center, dtype=F)).max(axis=1) <= F(reject)
            w = wi * cos if weighting == "cos" else np.full(V, wi, dtype=F)
            add = np.concatenate([w[:, None] * c, w[:, None]], axis=1)
        sums[ok] = sums[ok] + add[ok]
        views[ok] += 1
    return sums, views


def colors_of(sums, views, fallback=0.5):
    """colors (V, 3) = sum_rgb / sum_w clamped to [0, 1] where views > 0, `fallback` elsewhere."""
    seen = views > 0
    out = np.empty((sums.shape[0], 3), dtype=F)
    out[:] = np.asarray(fallback, dtype=F)
    with np.errstate(all="ignore"):
        out[seen] = np.clip(sums[seen, :3] / sums[seen, 3:4], F(0.0), F(1.0))
    return out


def soup(n_triangles=400, seed=7):
    """The seeded triangle soup of the tests, in camera space of the identity camera: vertices (3 T, 3) fp32, triangles
    (T, 3) int32.  Centres uniform in [-2, 2] x [-1, 1] x [-6, -2], vertices at centre + N(0, 0.25)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform([-2.0, -1.0, -6.0], [2.0, 1.0, -2.0], size=(n_triangles, 3))
    ver = (centres[:, None, :] + rng.normal(0.0, 0.25, size=(n_triangles, 3, 3))).astype(F).reshape(-1, 3)
    return ver, np.arange(3 * n_triangles, dtype=np.int32).reshape(-1, 3)


SOUP_CAMERA = dict(width=65, height=33, fx=40.0, fy=40.0, cx=32.25, cy=16.5)


def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, 1.0, 0.0)):
    """(3, 4) camera-to-world of a camera at `eye` looking along its -z at `target`."""
    eye, target, up = (np.asarray(x, dtype=np.float64) for x in (eye, target, up))
    z = eye - target
    z /= np.linalg.norm(z)
    x = np.cross(up, z)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    return np.stack([x, y, z, eye], axis=1)
