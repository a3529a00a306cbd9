"""numpy fp32 restatement of the texture atlas (include/nerf_fl_amd.h, "mesh atlas"): the layout, nfl_atlas_points,
nfl_atlas_resolve, nfl_mesh_shade_atlas and geometry.bake_texture, operation for operation in the header's order, so the
kernels (built with -ffp-contract=off) are held to it bit for bit.  Built on tests/meshcolor_ref.py (camera, blend) and
tests/meshrender_ref.py (visibility, the recomputation of u, v and the distance).  dtype=np.float64 gives the same
algorithm in fp64 where a test wants the arithmetic's error."""
import math

import numpy as np

import meshcolor_ref as mref
import meshrender_ref as rref

F = mref.F
# the worst difference of the fp32 restatement of the textured render from the fp64 restatement of the vertex-colour
# interpolation on soup(400, 7) at 65 x 33 (2.46e-6, measured by tests/test_atlas_cpu.py, which asserts it)
SOUP_FIGURE = 2.5e-6


def layout(n_triangles, cell, cols=None):
    """geometry.atlas_layout, restated."""
    cells = max((int(n_triangles) + 1) // 2, 1)
    if cols is None:
        cols = math.isqrt(cells - 1) + 1
    rows = (cells + cols - 1) // cols
    return {"cell": int(cell), "cols": int(cols), "rows": rows, "width": cols * cell, "height": rows * cell}


def texels(lay, first=0, count=None, dtype=F):
    """(tr, half, u, v, i, j) of texels first .. first + count - 1: triangle 2 k + h and the extrapolated barycentrics."""
    C, cols, W, H = lay["cell"], lay["cols"], lay["width"], lay["height"]
    count = W * H - first if count is None else count
    e = np.arange(first, first + count, dtype=np.int64)
    X, Y = e % W, e // W
    k = (Y // C) * cols + X // C
    i, j = X % C, Y % C
    h = (i + j > C - 1).astype(np.int64)
    L = dtype(C - 5)
    u = np.where(h == 1, (C - 2) - i, i - 1).astype(dtype) / L
    v = np.where(h == 1, (C - 2) - j, j - 1).astype(dtype) / L
    return 2 * k + h, h, u, v, i, j


def owners(triangles, n_vertices, tr):
    """(owner (n,) bool, idx (n, 3)): a texel has an owner when tr < T and the triangle's indices lie in [0, V)."""
    tri = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    T = tri.shape[0]
    ok = tr < T
    idx = tri[np.where(ok, tr, 0)] if T else np.zeros((tr.shape[0], 3), dtype=np.int64)
    ok = ok & ((idx >= 0) & (idx < n_vertices)).all(axis=1)
    return ok, np.where(ok[:, None], idx, 0)


def mix(w0, u, v, A, B, C):
    return (w0[:, None] * A + u[:, None] * B) + v[:, None] * C


def points(vertices, normals, triangles, lay, first=0, count=None):
    """nfl_atlas_points: (points (n, 3), normals (n, 3))."""
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    nrm = np.asarray(normals, dtype=F).reshape(-1, 3)
    tr, _, u, v, _, _ = texels(lay, first, count)
    ok, idx = owners(triangles, ver.shape[0], tr)
    n = tr.shape[0]
    p, m = np.full((n, 3), np.nan, dtype=F), np.zeros((n, 3), dtype=F)
    if ok.any() and ver.shape[0]:
        with np.errstate(all="ignore"):
            w0 = (F(1.0) - u) - v
            pp = mix(w0, u, v, ver[idx[:, 0]], ver[idx[:, 1]], ver[idx[:, 2]])
            mm = mix(w0, u, v, nrm[idx[:, 0]], nrm[idx[:, 1]], nrm[idx[:, 2]])
            length = np.sqrt(mref.dot(mm[:, 0], mm[:, 1], mm[:, 2], mm[:, 0], mm[:, 1], mm[:, 2]))
            mm = np.where((length > 0)[:, None], mm / length[:, None], F(0.0)).astype(F)
        p[ok], m[ok] = pp[ok], mm[ok]
    return p, m


def resolve(triangles, n_vertices, lay, sums, views, vertex_colors=None, fallback=(0.5, 0.5, 0.5), background=(0.0, 0.0, 0.0),
            first=0, count=None):
    """nfl_atlas_resolve: (texture (n, 3) fp32, texture_u8 (n, 3), seen (n,) uint8)."""
    sums, views = np.asarray(sums, dtype=F).reshape(-1, 4), np.asarray(views, dtype=np.int32).reshape(-1)
    count = views.shape[0] if count is None else count
    tr, _, u, v, _, _ = texels(lay, first, count)
    ok, idx = owners(triangles, n_vertices, tr)
    tex = np.empty((count, 3), dtype=F)
    tex[:] = np.asarray(background, dtype=F)
    seen = ok & (views > 0)
    unseen = ok & ~seen
    with np.errstate(all="ignore"):
        tex[seen] = np.fmin(np.fmax(sums[seen, :3] / sums[seen, 3:4], F(0.0)), F(1.0))
        if vertex_colors is not None:
            col = np.asarray(vertex_colors, dtype=F).reshape(-1, 3)
            w0 = (F(1.0) - u) - v
            tex[unseen] = mix(w0, u, v, col[idx[:, 0]], col[idx[:, 1]], col[idx[:, 2]])[unseen]
        else:
            tex[unseen] = np.asarray(fallback, dtype=F)
    return tex, rref.to_bytes(tex), seen.astype(np.uint8)


def lookup(atlas, lay, tr, u, v, dtype=F):
    """The bilinear lookup of nfl_mesh_shade_atlas at barycentrics (u, v) of triangles tr (all below 2 cols rows): (n, 3).
    `atlas` (H, W, 3) fp32, or uint8 converted by c / 255.0f.  Also returns the four texel addresses (n, 4, 2) as (x, y) and
    their weights (n, 4), for the layout tests."""
    C, cols = lay["cell"], lay["cols"]
    atlas = np.asarray(atlas)
    if atlas.dtype == np.uint8:
        atlas = atlas.astype(F) / F(255.0)
    atlas = atlas.astype(dtype)
    tr = np.asarray(tr, dtype=np.int64)
    u, v = np.asarray(u, dtype=dtype), np.asarray(v, dtype=dtype)
    L, last = dtype(C - 5), dtype(C - 1)
    with np.errstate(all="ignore"):
        lx, ly = dtype(1.0) + u * L, dtype(1.0) + v * L
        odd = (tr & 1) == 1
        lx, ly = np.where(odd, last - lx, lx), np.where(odd, last - ly, ly)
        lx, ly = np.fmin(np.fmax(lx, dtype(0.0)), last), np.fmin(np.fmax(ly, dtype(0.0)), last)
        xf, yf = np.floor(lx), np.floor(ly)
        tx, ty = lx - xf, ly - yf
        sx, sy = dtype(1.0) - tx, dtype(1.0) - ty
        xa, ya = xf.astype(np.int64), yf.astype(np.int64)
        xb, yb = np.minimum(xa + 1, C - 1), np.minimum(ya + 1, C - 1)
        k = tr >> 1
        ox, oy = (k % cols) * C, (k // cols) * C
        c00, c10 = atlas[oy + ya, ox + xa], atlas[oy + ya, ox + xb]
        c01, c11 = atlas[oy + yb, ox + xa], atlas[oy + yb, ox + xb]
        c = ((c00 * sx[:, None] + c10 * tx[:, None]) * sy[:, None] + (c01 * sx[:, None] + c11 * tx[:, None]) * ty[:, None])
    where = np.stack([np.stack([ox + x, oy + y], 1) for x, y in ((xa, ya), (xb, ya), (xa, yb), (xb, yb))], axis=1)
    weight = np.stack([sx * sy, tx * sy, sx * ty, tx * ty], axis=1)
    return c, where, weight


def shade(vertices, triangles, cam, words, atlas, lay, background=(1.0, 1.0, 1.0)):
    """nfl_mesh_shade_atlas of one camera's visibility words: rgb, rgb_u8, depth, triangle as meshrender_ref.shade gives them."""
    words = np.asarray(words, dtype=np.uint64).reshape(-1)
    winner = np.where(words == rref.EMPTY, np.int64(-1), (words & np.uint64(0xFFFFFFFF)).astype(np.int64))
    V = np.asarray(vertices).reshape(-1, 3).shape[0]
    base = rref.shade_at(vertices, triangles, cam, winner, "color", np.zeros((V, 3), dtype=F), background)
    cov = base["triangle"] >= 0
    rgb = base["rgb"].copy()
    if cov.any():
        c, _, _ = lookup(atlas, lay, base["triangle"][cov].astype(np.int64), base["u"][cov], base["v"][cov])
        rgb[cov] = c
    return {"rgb": rgb, "rgb_u8": rref.to_bytes(rgb), "depth": base["depth"], "triangle": base["triangle"]}


def render(vertices, triangles, cam, atlas, lay, background=(1.0, 1.0, 1.0)):
    words = rref.visibility(vertices, triangles, cam).reshape(-1)
    return dict(shade(vertices, triangles, cam, words, atlas, lay, background), words=words)


def bake(vertices, normals, triangles, cams, images, depth_tol, cell=16, cols=None, vertex_colors=None,
         fallback=(0.5, 0.5, 0.5), background=(0.0, 0.0, 0.0), reject=None, depths=None, **blend_kw):
    """geometry.bake_texture over `cams` (all selected, in order): the dict it returns, as arrays.  `depths`: the depth maps
    of the mesh per camera, computed here when not given."""
    ver = np.asarray(vertices, dtype=F).reshape(-1, 3)
    T = np.asarray(triangles).reshape(-1, 3).shape[0]
    lay = layout(T, cell, cols)
    if depths is None:
        depths = [mref.depth_map(ver, triangles, c) for c in cams]
    p, m = points(ver, normals, triangles, lay)
    sums, views = mref.blend(p, m, cams, images, depths, depth_tol, **blend_kw)
    tex, tex8, seen = resolve(triangles, ver.shape[0], lay, sums, views, vertex_colors, fallback, background)
    if reject is not None:
        sums, views = mref.blend(p, m, cams, images, depths, depth_tol, center=tex, reject=reject, **blend_kw)
        tex2, tex82, seen = resolve(triangles, ver.shape[0], lay, sums, views, vertex_colors, fallback, background)
        lost = (seen == 0)[:, None]
        tex, tex8 = np.where(lost, tex, tex2), np.where(lost, tex8, tex82)
    H, W = lay["height"], lay["width"]
    return dict(lay, texture=tex.reshape(H, W, 3), texture_u8=tex8.reshape(H, W, 3), seen=seen.reshape(H, W).astype(bool),
                views=views.reshape(H, W))


# ---- the closed loop of the tests: a cube of 12 large triangles whose appearance is finer than a triangle ------------------

CUBE_EYES = [(3, 0, 0), (0, 3, 0), (0, 0, 3), (-3, 0, 0), (0, -3, 0), (0, 0, -3)]


def cube(half=0.8):
    """A closed cube as a mesh has it after an extraction that does not smooth over creases: every face with its own four
    vertices and its own normal (24 vertices, 12 triangles wound outwards)."""
    ver, nrm, tri = [], [], []
    for axis in range(3):
        for sign in (-1.0, 1.0):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            n = np.zeros(3)
            n[axis] = sign
            corners = []
            for sa, sb in ((-1, -1), (1, -1), (1, 1), (-1, 1)):
                p = np.zeros(3)
                p[axis], p[a], p[b] = sign * half, sa * half, sb * half * sign          # the sign keeps the winding outwards
                corners.append(p)
            k = len(ver)
            ver += corners
            nrm += [n] * 4
            tri += [(k, k + 1, k + 2), (k, k + 2, k + 3)]
    return np.array(ver, dtype=F), np.array(nrm, dtype=F), np.array(tri, dtype=np.int32)


# six more, each looking at a corner region: every face is seen by several of them, at different angles
OBLIQUE_EYES = [(2.2, 1.5, 1.0), (-1.0, 2.2, 1.5), (1.5, -1.0, 2.2), (-2.2, -1.5, -1.0), (1.0, -2.2, -1.5), (-1.5, 1.0, -2.2)]


def cube_cameras(width=48, height=40, focal=50.0, eyes=CUBE_EYES):
    """Six cameras looking at the origin: on the axes at distance 3 by default, as the banks of the mesh tests."""
    K = np.array([[focal, 0, width / 2 - 0.25], [0, focal, height / 2 - 0.5], [0, 0, 1]])
    poses = [mref.look_at(e, up=(0.0, 0.0, 1.0) if e[2] == 0 else (0.0, 1.0, 0.0)) for e in eyes]
    cams = [mref.camera(width, height, focal, focal, K[0, 2], K[1, 2], p) for p in poses]
    return cams, np.stack(poses), np.stack([K] * len(poses))


def source_atlas(ver, nrm, tri, cell=32):
    """A procedural source atlas: stripes about a third of a cube edge wide, a function of the surface position, so that it
    is continuous over the edges of the triangles and much finer than any of them.  uint8 (H, W, 3) with its layout."""
    lay = layout(tri.shape[0], cell)
    p, _ = points(ver, nrm, tri, lay)
    p = np.nan_to_num(p.astype(np.float64))
    c = np.stack([0.5 + 0.4 * np.sin(6.0 * p[:, 0] + 2.0 * p[:, 1]), 0.5 + 0.4 * np.sin(6.0 * p[:, 1] - 2.0 * p[:, 2]),
                  0.5 + 0.4 * np.sin(6.0 * p[:, 2] + 2.0 * p[:, 0])], axis=1)
    return dict(lay, texture_u8=rref.to_bytes(c.astype(F)).reshape(lay["height"], lay["width"], 3))


def psnr_covered(frames, truth, covered):
    """PSNR of uint8 frames against uint8 truth over the covered pixels of all of them together."""
    se = n = 0.0
    for f, t, c in zip(frames, truth, covered):
        d = f[c].astype(np.float64) / 255 - t[c].astype(np.float64) / 255
        se, n = se + (d ** 2).sum(), n + d.size
    return -10 * np.log10(se / n)


def closed_loop(depth_tol=0.05, cell=16):
    """The loop of the tests, walked by the restatement alone: the cube rendered with the source atlas from six cameras into
    uint8 images; from those a baked atlas and, beside it, vertex colours (meshcolor_ref.blend); both rendered again.
    Returns a dict of everything, the two PSNRs over the covered pixels among it."""
    ver, nrm, tri = cube()
    cams, poses, Ks = cube_cameras()
    src = source_atlas(ver, nrm, tri)
    first = [render(ver, tri, c, src["texture_u8"], src) for c in cams]
    H, W = cams[0]["height"], cams[0]["width"]
    images = [r["rgb_u8"].reshape(H, W, 3) for r in first]
    depths = [mref.depth_map(ver, tri, c) for c in cams]
    sums, views = mref.blend(ver, nrm, cams, images, depths, depth_tol)
    colors = mref.colors_of(sums, views)
    baked = bake(ver, nrm, tri, cams, images, depth_tol, cell=cell, vertex_colors=colors, depths=depths)
    textured = [render(ver, tri, c, baked["texture"], baked) for c in cams]
    vertexed = [rref.render(ver, tri, c, "color", colors) for c in cams]
    cov = [r["triangle"] >= 0 for r in first]
    truth = [r["rgb_u8"] for r in first]
    return dict(ver=ver, nrm=nrm, tri=tri, cams=cams, poses=poses, Ks=Ks, source=src, first=first, images=images,
                colors=colors, vertex_views=views, baked=baked, textured=textured, vertexed=vertexed,
                psnr_textured=psnr_covered([r["rgb_u8"] for r in textured], truth, cov),
                psnr_vertex=psnr_covered([r["rgb_u8"] for r in vertexed], truth, cov))
