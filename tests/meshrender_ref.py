"""numpy fp32 restatement of nfl_mesh_visibility and nfl_mesh_shade (include/nerf_fl_amd.h, "mesh render"), operation for
operation: camera, pixel rays, `intersect` and the soup are those of tests/meshcolor_ref.py, every product, sum, quotient
and square root is one fp32 numpy operation in the header's order, so the kernels (built with -ffp-contract=off) are held
to it bit for bit.  The visibility buffer brute-forces every triangle against every pixel and owes nothing to the boxes the
raster kernel walks.  dtype=np.float64 gives the same algorithm in fp64 (on the fp32 camera coordinates and rays, as
meshcolor_ref.depth_map does)."""
import numpy as np

import meshcolor_ref as mref

F = mref.F
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
MODES = ("color", "normal", "facing")


def _camera_triangles(vertices, triangles, cam):
    """(a, b, c, orig): camera-space corners of the triangles that can hit at all -- indices in range, nine finite camera
    coordinates -- and their ORIGINAL numbers, ascending."""
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V = ver.shape[0]
    orig = np.nonzero(((tri >= 0) & (tri < V)).all(axis=1))[0]
    if V == 0 or orig.size == 0:
        z = np.zeros((0, 3), dtype=F)
        return z, z, z, orig[:0]
    with np.errstate(all="ignore"):
        q = mref.to_camera(cam, ver)
    a, b, c = (q[tri[orig, k]] for k in range(3))
    ok = np.isfinite(a).all(axis=1) & np.isfinite(b).all(axis=1) & np.isfinite(c).all(axis=1)
    return a[ok], b[ok], c[ok], orig[ok]


def nearest(vertices, triangles, cam, dtype=F, chunk=256):
    """(distance (P,), triangle (P,) int64) of every pixel, row-major: the smallest distance below +inf over all HITS and the
    lowest ORIGINAL index among the triangles that reach it; +inf and -1 where there is none."""
    P = cam["height"] * cam["width"]
    best, who = np.full(P, np.inf, dtype=dtype), np.full(P, -1, dtype=np.int64)
    a, b, c, orig = _camera_triangles(vertices, triangles, cam)
    if orig.size == 0:
        return best, who
    with np.errstate(all="ignore"):
        dx, dy = mref.pixel_rays(cam)
        dx, dy = dx.astype(dtype), dy.astype(dtype)
        length = np.sqrt((dx * dx + dy * dy) + dtype(1.0))
        for t0 in range(0, orig.size, chunk):
            s = slice(t0, t0 + chunk)
            hit, tau, _, _ = mref.intersect(a[s], b[s], c[s], dx, dy, dtype)
            d = np.where(hit, tau * length[None, :], dtype(np.inf))
            k = d.argmin(axis=0)                            # the lowest index on a tie
            dk = d[k, np.arange(P)]
            better = dk < best                              # strictly: an earlier chunk keeps a tie
            best = np.where(better, dk, best)
            who = np.where(better, orig[s][k], who)
    return best, who


def visibility(vertices, triangles, cam):
    """(height, width) uint64 words of nfl_mesh_visibility: (bits(distance) << 32) | triangle, 2^64 - 1 where nothing is hit."""
    d, tr = nearest(vertices, triangles, cam)
    words = (d.astype(F).view(np.uint32).astype(np.uint64) << np.uint64(32)) | (tr & 0xFFFFFFFF).astype(np.uint64)
    return np.where(tr >= 0, words, EMPTY).reshape(cam["height"], cam["width"])


def run_visibility(vertices, triangles, cams):
    if not cams:
        return np.zeros(0, dtype=np.uint64)
    return np.concatenate([visibility(vertices, triangles, c).reshape(-1) for c in cams])


def to_bytes(c):
    """(uint8)(clamp(c, 0, 1) * 255): truncation, NaN -> 0."""
    c = np.asarray(c, dtype=F)
    with np.errstate(all="ignore"):
        x = np.where(c > 0, np.where(c < 1, c, F(1.0)), F(0.0)).astype(F)
        return (x * F(255.0)).astype(np.uint8)


def shade_at(vertices, triangles, cam, winner, mode="color", attr=None, background=(1.0, 1.0, 1.0), dtype=F):
    """nfl_mesh_shade of one camera given the triangle number of every pixel (`winner` (P,) integers; anything that is not
    the index of a triangle with its three indices in range is uncovered).  Returns a dict: rgb (P, 3), rgb_u8 (P, 3),
    depth (P,), triangle (P,) int32, and u, v (P,) for the tests (0 where uncovered)."""
    assert mode in MODES
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    V, T = ver.shape[0], tri.shape[0]
    P = cam["height"] * cam["width"]
    winner = np.asarray(winner, dtype=np.int64).reshape(P)
    rgb = np.empty((P, 3), dtype=dtype)
    rgb[:] = np.asarray(background, dtype=F).astype(dtype)
    depth = np.full(P, np.inf, dtype=dtype)
    who = np.full(P, -1, dtype=np.int32)
    uu, vv = np.zeros(P, dtype=dtype), np.zeros(P, dtype=dtype)
    ok = (winner >= 0) & (winner < T)
    idx = tri[np.where(ok, winner, 0)] if T else np.zeros((P, 3), dtype=np.int64)
    ok &= ((idx >= 0) & (idx < V)).all(axis=1)
    if ok.any():
        pix = np.nonzero(ok)[0]
        idx = idx[pix]
        with np.errstate(all="ignore"):
            q = mref.to_camera(cam, ver)
            a, b, c = (q[idx[:, k]].astype(dtype) for k in range(3))
            dx, dy = mref.pixel_rays(cam)
            dx, dy, dz = dx[pix].astype(dtype), dy[pix].astype(dtype), dtype(-1.0)
            tv = [-a[:, k] for k in range(3)]
            e1 = [b[:, k] - a[:, k] for k in range(3)]
            e2 = [c[:, k] - a[:, k] for k in range(3)]
            qv = mref.cross(tv, e1)
            tnum = mref.dot(e2[0], e2[1], e2[2], qv[0], qv[1], qv[2])
            pv = mref.cross((dx, dy, dz), e2)
            det = mref.dot(e1[0], e1[1], e1[2], pv[0], pv[1], pv[2])
            inv = dtype(1.0) / det
            u = mref.dot(tv[0], tv[1], tv[2], pv[0], pv[1], pv[2]) * inv
            v = mref.dot(dx, dy, dz, qv[0], qv[1], qv[2]) * inv
            tau = tnum * inv
            dist = tau * np.sqrt((dx * dx + dy * dy) + dz * dz)
            w0 = (dtype(1.0) - u) - v
            if mode == "facing":
                n = mref.cross(e1, e2)
                g = np.abs(mref.dot(n[0], n[1], n[2], dx, dy, dz)) / (np.sqrt(mref.dot(n[0], n[1], n[2], n[0], n[1], n[2]))
                                                                       * np.sqrt(mref.dot(dx, dy, dz, dx, dy, dz)))
                g = np.where(np.isnan(g), dtype(0.0), g)
                col = np.stack([g, g, g], axis=1)
            else:
                at = np.asarray(attr, dtype=F).reshape(-1, 3).astype(dtype)
                A, B, C = (at[idx[:, k]] for k in range(3))
                m = [(w0 * A[:, k] + u * B[:, k]) + v * C[:, k] for k in range(3)]
                if mode == "normal":
                    length = np.sqrt(mref.dot(m[0], m[1], m[2], m[0], m[1], m[2]))
                    m = [np.where(length > 0, dtype(0.5) * (m[k] / length) + dtype(0.5), dtype(0.5)) for k in range(3)]
                col = np.stack(m, axis=1)
        good = det != 0                                      # False for NaN too
        pix = pix[good]
        rgb[pix], depth[pix], who[pix] = col[good], dist[good], winner[pix]
        uu[pix], vv[pix] = u[good], v[good]
    return {"rgb": rgb, "rgb_u8": to_bytes(rgb), "depth": depth, "triangle": who, "u": uu, "v": vv}


def shade(vertices, triangles, cam, words, mode="color", attr=None, background=(1.0, 1.0, 1.0)):
    """nfl_mesh_shade of one camera's visibility words (any shape, height * width of them)."""
    words = np.asarray(words, dtype=np.uint64).reshape(-1)
    winner = np.where(words == EMPTY, np.int64(-1), (words & np.uint64(0xFFFFFFFF)).astype(np.int64))
    return shade_at(vertices, triangles, cam, winner, mode, attr, background)


def render(vertices, triangles, cam, mode="color", attr=None, background=(1.0, 1.0, 1.0)):
    """visibility + shade of one camera; `words` (P,) added to the dict."""
    words = visibility(vertices, triangles, cam).reshape(-1)
    return dict(shade(vertices, triangles, cam, words, mode, attr, background), words=words)


def run_render(vertices, triangles, cams, mode="color", attr=None, background=(1.0, 1.0, 1.0)):
    """The outputs of a run of cameras back to back, as the kernels lay them out."""
    outs = [render(vertices, triangles, c, mode, attr, background) for c in cams]
    return {k: np.concatenate([o[k] for o in outs]) for k in ("words", "rgb", "rgb_u8", "depth", "triangle")}
