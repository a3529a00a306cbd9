"""CPU-side checks of the texture atlas (nerf_fl_amd.geometry.atlas_layout / bake_texture / render_mesh(texture=) / write_obj,
csrc/nfl_atlas.hip): the C entry points refuse bad arguments before any launch (their structs and signatures are held to
the header in tests/test_abi_cpu.py); the numpy
restatement (tests/atlas_ref.py), which the GPU tests hold the kernels to bit for bit, is itself checked on the properties
the layout is built for and on hand cases whose expected numbers are written out; write_obj is read back by a parser of the
test's own.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import atlas_ref as aref
import meshcolor_ref as mref
import meshrender_ref as rref
from abi_probe import L  # noqa: F401  (a fixture)
from nerf_fl_amd import _lib, geometry

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL = -1
CELLS = [6, 7, 16, 33]


# ---- sources and validation ------------------------------------------------------------------------------------------------

def test_the_unit_sits_on_the_shared_headers():
    header = open(os.path.join(ROOT, "include", "nerf_fl_amd.h")).read()
    assert header.index("---- mesh render") < header.index("---- mesh atlas") < header.index("---- hierarchical sampling")
    assert (_lib.ATLAS_MIN_CELL, _lib.ATLAS_MAX_CELL) == (6, 1024)
    # the new unit sits on the shared headers, and the two units beside it do not know of it
    csrc = os.path.join(ROOT, "nerf_fl_amd", "csrc")
    text = open(os.path.join(csrc, "nfl_atlas.hip")).read()
    for h in ("nfl_geom.h", "nfl_meshray.h", "nfl_pixel.h"):
        assert f'#include "{h}"' in text
    assert "nmc_ray<false>" in text and not re.search(r"NFL_DEV \w+ nmc_", text)
    for unit in ("nfl_meshcolor.hip", "nfl_meshrender.hip"):
        assert "atlas" not in open(os.path.join(csrc, unit)).read()


def _points_args():
    a = _lib.AtlasPointsArgs()
    a.d_vertices, a.d_vertex_normals, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 0x2000, 0x3000, 30, 10
    a.cell, a.cols, a.rows, a.first_texel, a.n_texels = 16, 3, 2, 5, 100
    a.d_points, a.d_normals = 0x4000, 0x5000
    return a


def _resolve_args():
    a = _lib.AtlasResolveArgs()
    a.d_triangles, a.n_vertices, a.n_triangles = 0x3000, 30, 10
    a.cell, a.cols, a.rows, a.first_texel, a.n_texels = 16, 3, 2, 5, 100
    a.d_sum, a.d_views, a.d_vertex_colors = 0x6000, 0x7000, 0x8000
    a.d_texture, a.d_texture_u8, a.d_seen = 0x9000, 0xA001, 0xB003
    return a


def _shade_args():
    a = _lib.MeshShadeAtlasArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 0x2000, 30, 10
    a.d_table, a.n_images, a.first, a.count, a.d_vis, a.n_vis = 0x3000, 4, 1, 2, 0x4000, 100
    a.d_atlas, a.d_atlas_u8, a.cell, a.cols, a.rows = 0x5000, None, 16, 3, 2
    a.d_rgb, a.d_rgb_u8, a.d_depth, a.d_triangle = 0x6000, 0x7001, 0x8000, 0x9000
    return a


# what all three refuse of the atlas: (field, value); 48 x 32 texels hold 12 triangles
BAD_LAYOUT = [("cell", 5), ("cell", 1025), ("cell", 0), ("cell", -16), ("cols", 0), ("cols", -1), ("rows", 0), ("rows", -2),
              ("n_triangles", 13), ("cols", 1 << 22), ("rows", 1 << 22)]
BAD_MESH = [("n_vertices", -1), ("n_vertices", 1 << 31), ("n_triangles", -1), ("n_triangles", (1 << 31) // 3 + 1)]
BAD_RANGE = [("first_texel", -1), ("n_texels", -1), ("first_texel", 48 * 32 + 1), ("n_texels", 48 * 32 - 4),
             ("n_texels", 1 << 40), ("first_texel", 1 << 62)]


def _refused(fn, make, cases):
    for field, bad in cases:
        a = make()
        setattr(a, field, bad)
        assert fn(C.byref(a), None) == EINVAL, (field, bad)


def test_points_refuses_before_any_launch(L):
    """Every pointer is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    f = L.nfl_atlas_points
    assert f(None, None) == EINVAL
    _refused(f, _points_args, BAD_LAYOUT + BAD_MESH + BAD_RANGE)
    _refused(f, _points_args, [(p, None) for p in ("d_vertices", "d_vertex_normals", "d_triangles", "d_points", "d_normals")])
    _refused(f, _points_args, [("d_vertices", 0x1002), ("d_vertex_normals", 0x2001), ("d_triangles", 0x3003), ("d_points", 0x4002),
                               ("d_normals", 0x5001)])
    a = _points_args()                                               # the largest atlas: 2^31 - 1 texels are too few for 46341^2
    a.cell, a.cols, a.rows = 6, 7724, 7724
    assert f(C.byref(a), None) == EINVAL
    a = _points_args()                                               # nothing to do: NFL_OK without a launch
    a.n_texels = 0
    assert f(C.byref(a), None) == 0
    a.first_texel = 48 * 32                                          # an empty range at the very end
    assert f(C.byref(a), None) == 0


def test_resolve_refuses_before_any_launch(L):
    f = L.nfl_atlas_resolve
    assert f(None, None) == EINVAL
    _refused(f, _resolve_args, BAD_LAYOUT + BAD_MESH + BAD_RANGE)
    _refused(f, _resolve_args, [(p, None) for p in ("d_triangles", "d_sum", "d_views")])
    _refused(f, _resolve_args, [("d_triangles", 0x3002), ("d_sum", 0x6008), ("d_sum", 0x6004), ("d_views", 0x7002),
                                ("d_vertex_colors", 0x8001), ("d_texture", 0x9002)])
    a = _resolve_args()
    a.n_texels = 0
    assert f(C.byref(a), None) == 0
    a.d_vertex_colors = a.d_texture = a.d_texture_u8 = a.d_seen = None           # all optional
    assert f(C.byref(a), None) == 0


def test_shade_atlas_refuses_before_any_launch(L):
    f = L.nfl_mesh_shade_atlas
    assert f(None, None) == EINVAL
    _refused(f, _shade_args, BAD_LAYOUT + BAD_MESH)
    _refused(f, _shade_args, [(p, None) for p in ("d_vertices", "d_triangles", "d_table", "d_vis", "d_atlas")])      # no atlas at all
    a = _shade_args()                                                # both atlases
    a.d_atlas_u8 = 0x5800
    assert f(C.byref(a), None) == EINVAL
    _refused(f, _shade_args, [("d_vertices", 0x1002), ("d_triangles", 0x2001), ("d_table", 0x3004), ("d_vis", 0x4004),
                              ("d_atlas", 0x5002), ("d_rgb", 0x6001), ("d_depth", 0x8002), ("d_triangle", 0x9003)])
    _refused(f, _shade_args, [("n_images", 0), ("first", -1), ("count", -1), ("first", 3), ("count", 4), ("first", 5),
                              ("n_vis", -1), ("n_vis", (1 << 38) + 1)])
    for u8 in (False, True):                                         # nothing to do: NFL_OK, with either kind of atlas
        a = _shade_args()
        a.n_vis = 0
        if u8:
            a.d_atlas, a.d_atlas_u8 = None, 0x5801                   # bytes: any address
        assert f(C.byref(a), None) == 0


# ---- the layout ----------------------------------------------------------------------------------------------------------

def test_atlas_layout_and_its_refusals():
    assert geometry.atlas_layout(1, 6) == dict(cell=6, cols=1, rows=1, width=6, height=6)
    assert geometry.atlas_layout(0, 6) == dict(cell=6, cols=1, rows=1, width=6, height=6)
    assert geometry.atlas_layout(3, 6, 1) == dict(cell=6, cols=1, rows=2, width=6, height=12)
    assert geometry.atlas_layout(3, 6, 2) == dict(cell=6, cols=2, rows=1, width=12, height=6)
    assert geometry.atlas_layout(6108, 16) == dict(cell=16, cols=56, rows=55, width=896, height=880)     # 3054 cells
    assert geometry.atlas_layout(19, 7)["cols"] == 4 and geometry.atlas_layout(18, 7)["cols"] == 3        # 10 and 9 cells
    for T in (0, 1, 2, 3, 17, 18, 19, 513, 6108):
        for cols in (None, 1, 3):
            lay = geometry.atlas_layout(T, 7, cols)
            assert lay == aref.layout(T, 7, cols) and 2 * lay["cols"] * lay["rows"] >= T
            assert lay["rows"] == 1 or 2 * lay["cols"] * (lay["rows"] - 1) < T            # no empty row
    for bad in (dict(cell=5), dict(cell=1025), dict(cell=16, cols=0), dict(cell=1024, cols=1), dict(n_triangles=-1)):
        with pytest.raises(ValueError):
            geometry.atlas_layout(**dict(dict(n_triangles=100000, cell=16), **bad))


@pytest.mark.parametrize("C_", CELLS)
def test_every_texel_has_exactly_one_half(C_):
    lay = aref.layout(5, C_, 2)                                      # 2 x 2 cells, triangle 5 absent
    tr, h, u, v, i, j = aref.texels(lay)
    W, H = lay["width"], lay["height"]
    assert tr.shape == (W * H,) and set(np.unique(h)) == {0, 1} and tr.min() == 0 and tr.max() == 7
    for t in range(8):
        mine = tr == t
        assert mine.sum() == (C_ * (C_ + 1) // 2 if t % 2 == 0 else C_ * (C_ - 1) // 2)
        X, Y = np.nonzero(mine.reshape(H, W))[1], np.nonzero(mine.reshape(H, W))[0]
        k = t // 2
        assert (X // C_ == k % 2).all() and (Y // C_ == k // 2).all()            # all in the triangle's own cell
    # half 1 is half 0 turned by 180 degrees: the texel (C - 1 - i, C - 1 - j) of half 1 has the barycentrics of (i, j) of
    # half 0
    cell0 = (tr // 2 == 0)
    uv = {(int(a), int(b)): (c, d, int(e)) for a, b, c, d, e in zip(i[cell0], j[cell0], u[cell0], v[cell0], h[cell0])}
    for (a, b), (c, d, e) in uv.items():
        if e == 1:
            assert uv[(C_ - 1 - a, C_ - 1 - b)] == (c, d, 0)
    assert uv[(1, 1)] == (0.0, 0.0, 0) and uv[(C_ - 4, 1)] == (1.0, 0.0, 0) and uv[(1, C_ - 4)] == (0.0, 1.0, 0)
    assert uv[(C_ - 2, C_ - 2)] == (0.0, 0.0, 1) and uv[(3, C_ - 2)] == (1.0, 0.0, 1) and uv[(C_ - 2, 3)] == (0.0, 1.0, 1)


def _inside(n=40):
    """Barycentrics covering a triangle, its edges and corners included: a lattice and seeded random points."""
    g = np.linspace(0.0, 1.0, n + 1)
    u, v = np.meshgrid(g, g)
    keep = u + v <= 1.0 + 1e-12
    rng = np.random.default_rng(5)
    r = rng.uniform(size=(4000, 2))
    r = np.where((r.sum(axis=1) > 1)[:, None], 1 - r, r)
    return np.concatenate([u[keep], r[:, 0]]), np.concatenate([np.minimum(v[keep], 1 - u[keep]), r[:, 1]])


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("C_", CELLS)
def test_a_lookup_inside_a_triangle_stays_in_its_half_and_reproduces_an_affine_attribute(C_, dtype):
    """For points of a triangle (edges included) the bilinear lookup reads, with non-zero weight, only texels of its own half
    of its own cell; corner texels hold the corner's attribute exactly; and an attribute affine over the triangle comes back.
    The bound: about twenty roundings, each at most half an ulp of a magnitude up to 8 (C = 6 extrapolates the gutter to
    u = 4, colours within [0, 1]), so 64 ulps of 1 -- the 3e-16 seen in fp64 and the 3e-7 in fp32 are well inside."""
    T = 7
    lay = aref.layout(T, C_, 3)
    rng = np.random.default_rng(C_)
    tri = np.arange(3 * T).reshape(T, 3)
    col = rng.uniform(size=(3 * T, 3)).astype(F)
    n = lay["width"] * lay["height"]
    tex32, _, _ = aref.resolve(tri, 3 * T, lay, np.zeros((n, 4)), np.zeros(n), col)
    tex32 = tex32.reshape(lay["height"], lay["width"], 3)
    uv = geometry.atlas_uv(lay, T)
    assert uv.shape == (T, 3, 2)
    for t in range(T):                                               # corner texels: the corner's colour, bit for bit
        for c in range(3):
            x, y = uv[t, c].astype(int)
            assert np.array_equal(tex32[y, x], col[tri[t, c]]), (t, c)
    # the texels in `dtype`: the resolve's interpolation of the vertex colours, triangle 7 of seven left at zero
    tr_all, _, tu, tv, _, _ = aref.texels(lay, dtype=dtype)
    own, idx = aref.owners(tri, 3 * T, tr_all)
    cd = col.astype(dtype)
    tex = np.where(own[:, None], aref.mix((dtype(1.0) - tu) - tv, tu, tv, cd[idx[:, 0]], cd[idx[:, 1]], cd[idx[:, 2]]), dtype(0.0))
    assert tex.dtype == dtype and (dtype != np.float32 or np.array_equal(tex[own], tex32.reshape(-1, 3)[own]))
    tex = tex.reshape(lay["height"], lay["width"], 3)
    tr_all = tr_all.reshape(lay["height"], lay["width"])
    u, v = _inside()
    worst = 0.0
    for t in range(T):
        c, where, weight = aref.lookup(tex, lay, np.full(u.shape, t), u, v, dtype)
        read = weight > 0
        assert (tr_all[where[..., 1], where[..., 0]][read] == t).all(), t         # its own half of its own cell
        A, B, Cc = (col[tri[t, k]].astype(np.float64) for k in range(3))
        exact = (1 - u - v)[:, None] * A + u[:, None] * B + v[:, None] * Cc
        worst = max(worst, np.abs(c.astype(np.float64) - exact).max())
    print(f"C = {C_}, {np.dtype(dtype).name}: an affine attribute comes back to {worst:.2e}")
    assert worst <= 64 * np.finfo(dtype).eps


def test_forged_barycentrics_stay_inside_the_cell():
    lay = aref.layout(4, 7, 2)
    tex = np.arange(lay["height"] * lay["width"] * 3, dtype=F).reshape(lay["height"], lay["width"], 3)
    u = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 5.0, -3.0, 0.5], dtype=F)
    for t in range(4):
        for uu, vv in ((u, u[::-1]), (u, u)):
            c, where, _ = aref.lookup(tex, lay, np.full(8, t), uu, vv)
            k = t // 2
            assert (where[..., 0] // 7 == k % 2).all() and (where[..., 1] // 7 == k // 2).all()
    c, where, weight = aref.lookup(tex, lay, np.array([0, 1]), np.array([np.nan, np.nan], F), np.array([np.nan, np.nan], F))
    assert where[0, 0].tolist() == [0, 0] and where[1, 0].tolist() == [0, 0]      # NaN -> local (0, 0) in both halves
    assert np.array_equal(c[0], tex[0, 0])


# ---- hand cases ---------------------------------------------------------------------------------------------------------

# the unit right triangle in the plane z = 0: with C = 6, L = 1, texel (i, j) of half 0 IS the point (i - 1, j - 1, 0)
VER = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], dtype=F)
NRM = np.array([[0, 0, 2.0]] * 3, dtype=F)
COL = np.array([[0.9, 0.1, 0.2], [0.2, 0.8, 0.1], [0.1, 0.3, 0.7]], dtype=F)


def test_one_triangle_cell_6():
    lay = aref.layout(1, 6)
    p, m = aref.points(VER, NRM, [[0, 1, 2]], lay)
    p, m = p.reshape(6, 6, 3), m.reshape(6, 6, 3)
    for j in range(6):
        for i in range(6):
            if i + j <= 5:
                assert p[j, i].tolist() == [i - 1.0, j - 1.0, 0.0] and m[j, i].tolist() == [0.0, 0.0, 1.0], (i, j)
            else:                                                    # half 1 of cell 0: triangle 1 of a mesh of one
                assert np.isnan(p[j, i]).all() and m[j, i].tolist() == [0.0, 0.0, 0.0], (i, j)
    assert p.dtype == F and m.dtype == F
    # resolve: a seen texel, a seen one out of gamut, an unseen one with and without vertex colours, an ownerless one
    sums, views = np.zeros((36, 4), F), np.zeros(36, np.int32)
    sums[7], views[7] = [0.5, 1.0, 3.0, 2.0], 2                       # texel (1, 1)
    sums[8], views[8] = [-1.0, np.nan, 0.25, 1.0], 1                  # texel (2, 1)
    sums[35], views[35] = [1.0, 1.0, 1.0, 1.0], 5                     # ownerless, whatever the views say
    tex, tex8, seen = aref.resolve([[0, 1, 2]], 3, lay, sums, views, COL, background=(0.25, 0.5, 0.75))
    assert tex[7].tolist() == [0.25, 0.5, 1.0] and tex8[7].tolist() == [63, 127, 255] and seen[7] == 1
    assert tex[8].tolist() == [0.0, 0.0, 0.25] and tex8[8].tolist() == [0, 0, 63] and seen[8] == 1
    assert tex[35].tolist() == [0.25, 0.5, 0.75] and tex8[35].tolist() == [63, 127, 191] and seen[35] == 0
    assert np.array_equal(tex[13], COL[2]) and np.array_equal(tex[9], (F(-1) * COL[0] + F(2) * COL[1]) + F(0) * COL[2])
    assert seen.sum() == 2 and seen.dtype == np.uint8
    # texel (0, 0): u = v = -1, w0 = 3: extrapolated, not clamped
    assert np.array_equal(tex[0], (F(3) * COL[0] + F(-1) * COL[1]) + F(-1) * COL[2])
    assert tex[0, 0] == pytest.approx(3 * 0.9 - 0.2 - 0.1, abs=1e-6) and tex8[0].tolist() == [255, 0, 0]
    flat, _, _ = aref.resolve([[0, 1, 2]], 3, lay, sums, views, None, fallback=(0.1, 0.2, 0.3), background=(0.25, 0.5, 0.75))
    assert flat[0].tolist() == [F(0.1), F(0.2), F(0.3)] and flat[7].tolist() == [0.25, 0.5, 1.0] and flat[35].tolist() == [0.25, 0.5, 0.75]


def test_three_triangles_in_one_and_two_columns():
    ver = np.concatenate([VER, VER + 10, VER + 20]).astype(F)
    nrm = np.concatenate([NRM] * 3)
    tri = np.arange(9).reshape(3, 3)
    for cols, (W, H) in ((1, (6, 12)), (2, (12, 6))):
        lay = aref.layout(3, 6, cols)
        assert (lay["width"], lay["height"], lay["rows"]) == (W, H, 3 - cols)
        p, _ = aref.points(ver, nrm, tri, lay)
        p = p.reshape(H, W, 3)
        assert p[1, 1].tolist() == [0, 0, 0] and p[4, 4].tolist() == [10, 10, 10] and p[4, 3].tolist() == [11, 10, 10]
        x0, y0 = (0, 6) if cols == 1 else (6, 0)                     # cell 1
        assert p[y0 + 1, x0 + 1].tolist() == [20, 20, 20] and p[y0 + 2, x0 + 1].tolist() == [20, 21, 20]
        assert np.isnan(p[y0 + 4, x0 + 4]).all() and np.isnan(p[y0 + 5, x0 + 1]).all()      # triangle 3 of three
        assert np.isnan(p).all(axis=2).sum() == 15
        # a range in the middle equals the same rows of the whole
        q, _ = aref.points(ver, nrm, tri, lay, first=17, count=31)
        assert np.array_equal(q.view(np.uint32), p.reshape(-1, 3)[17:48].view(np.uint32))


def test_bad_index_zero_normal_and_nan_colours():
    lay = aref.layout(2, 6)
    ver = np.concatenate([VER, VER + 10]).astype(F)
    nrm = np.array([[1, 0, 0], [-1, 0, 0], [0, 0, 0]] * 2, dtype=F)
    tri = np.array([[0, 1, 2], [3, 4, 6]])                            # triangle 1 names vertex 6 of six
    p, m = aref.points(ver, nrm, tri, lay)
    p, m = p.reshape(6, 6, 3), m.reshape(6, 6, 3)
    assert np.isnan(p[4, 4]).all() and np.isnan(p).all(axis=2).sum() == 15       # the bad triangle owns nothing
    # the normal at (u, v) is ((1 - u - v) - u, 0, 0): zero on the line 2 u + v = 1, so at texel (1, 2) (u = 0, v = 1)
    assert m[2, 1].tolist() == [0, 0, 0] and m[1, 1].tolist() == [1, 0, 0] and m[1, 2].tolist() == [-1, 0, 0]
    tex, tex8, seen = aref.resolve(tri, 6, lay, np.zeros((36, 4)), np.zeros(36), np.full((6, 3), 0.5), background=(1.0, 0.0, 0.0))
    assert tex.reshape(6, 6, 3)[4, 4].tolist() == [1.0, 0.0, 0.0] and tex.reshape(6, 6, 3)[1, 1].tolist() == [0.5, 0.5, 0.5]
    tri[1] = [3, -1, 5]
    assert np.isnan(aref.points(ver, nrm, tri, lay)[0]).all(axis=1).sum() == 15
    # NaN and out-of-gamut colours: the floats keep them, the bytes clamp, NaN -> 0
    col = np.array([[np.nan, 1.5, -0.5]] * 6, dtype=F)
    tex, tex8, _ = aref.resolve([[0, 1, 2]], 6, lay, np.zeros((36, 4)), np.zeros(36), col)
    assert np.isnan(tex[7, 0]) and tex[7, 1] == 1.5 and tex[7, 2] == -0.5 and tex8[7].tolist() == [0, 255, 0]
    # a NaN texel read by the shade: NaN in the float, 0 in the byte
    c, _, _ = aref.lookup(tex.reshape(6, 6, 3), lay, np.array([0]), np.array([0.25], F), np.array([0.25], F))
    assert np.isnan(c[0, 0]) and rref.to_bytes(c)[0].tolist() == [0, 255, 0]
    # bytes -> floats: c / 255.0f
    c, _, _ = aref.lookup(np.full((6, 6, 3), 51, np.uint8), lay, np.array([0]), np.array([0.25], F), np.array([0.5], F))
    assert c[0, 0] == pytest.approx(0.2, abs=1e-7)


def test_textured_render_of_the_hand_triangle():
    """The square-on triangle of test_meshrender_cpu.py with an atlas resolved from its vertex colours: the picture of the
    vertex-colour render, and a vertex pixel reads its corner texel."""
    cam = mref.camera(9, 9, 8.0, 8.0, 4.0, 4.0)
    ver = np.array([[-1.125, -1.125, -3], [1.125, -1.125, -3], [0, 1.125, -3]], dtype=F)
    tri = np.array([[0, 1, 2]])
    for C_ in (6, 16):
        lay = aref.layout(1, C_)
        n = C_ * C_
        tex, tex8, _ = aref.resolve(tri, 3, lay, np.zeros((n, 4)), np.zeros(n), COL)
        want = rref.render(ver, tri, cam, "color", COL, (0.25, 0.5, 0.75))
        got = aref.render(ver, tri, cam, tex.reshape(C_, C_, 3), lay, (0.25, 0.5, 0.75))
        assert np.array_equal(got["triangle"], want["triangle"]) and np.array_equal(got["depth"], want["depth"])
        assert np.array_equal(got["words"], want["words"])
        assert np.abs(got["rgb"] - want["rgb"]).max() <= 1e-6
        assert got["rgb"].reshape(9, 9, 3)[7, 1] == pytest.approx(COL[0], abs=1e-6)
        assert np.array_equal(got["rgb"].reshape(9, 9, 3)[0, 0], np.array([0.25, 0.5, 0.75], F))
    # a byte atlas: colours muted so that the extrapolated gutter stays in gamut (bytes clamp it otherwise); every texel is
    # truncated by less than 1 / 255, and so is their bilinear mean
    muted = (F(0.4) + F(0.2) * COL).astype(F)
    tex, tex8, _ = aref.resolve(tri, 3, lay, np.zeros((n, 4)), np.zeros(n), muted)
    own = aref.texels(lay)[0] == 0
    assert tex[own].min() > 0.2 and tex[own].max() < 0.8
    want = rref.render(ver, tri, cam, "color", muted, (0.25, 0.5, 0.75))
    got8 = aref.render(ver, tri, cam, tex8.reshape(16, 16, 3), lay, (0.25, 0.5, 0.75))
    diff = want["rgb"] - got8["rgb"]
    assert diff.max() <= 1.0 / 255 + 1e-6 and diff.min() >= -1e-6 and np.array_equal(got8["triangle"], want["triangle"])


def test_atlas_render_fp32_against_fp64_vertex_colours_on_the_soup():
    """The figure the GPU test's bound comes from: the fp32 restatement of the textured render (atlas = the vertex colours
    interpolated at every texel, nothing seen) against the fp64 restatement of the vertex-colour interpolation, over the
    covered pixels of soup(400, 7) at 65 x 33 (the winners agree everywhere there, test_meshrender_cpu.py).  Measured:
    2.46e-6 at cell 16, the figure of the vertex-colour render itself: the error of u and v dominates both.  The GPU test bounds the device's textured render against the device's vertex-colour render by four
    times the figure asserted here."""
    ver, tri = mref.soup(400, 7)
    cam = mref.camera(**mref.SOUP_CAMERA)
    col = np.random.default_rng(11).uniform(size=(ver.shape[0], 3)).astype(F)
    lay = aref.layout(400, 16)
    n = lay["width"] * lay["height"]
    tex, _, _ = aref.resolve(tri, ver.shape[0], lay, np.zeros((n, 4)), np.zeros(n), col)
    got = aref.render(ver, tri, cam, tex.reshape(lay["height"], lay["width"], 3), lay)
    d64, w64 = rref.nearest(ver, tri, cam, dtype=np.float64)
    s64 = rref.shade_at(ver, tri, cam, w64, "color", col, dtype=np.float64)
    assert np.array_equal(got["triangle"], s64["triangle"])
    cov = got["triangle"] >= 0
    worst = np.abs(got["rgb"][cov].astype(np.float64) - s64["rgb"][cov]).max()
    print(f"soup: textured fp32 against vertex colours in fp64, worst difference {worst:.3e} over {cov.mean():.3f} of the pixels")
    assert worst <= aref.SOUP_FIGURE


def test_the_closed_loop_shows_in_the_restatement_alone():
    """A cube of 12 triangles whose appearance is stripes a third of an edge wide: baked into an atlas and rendered again it
    scores far above the same loop through vertex colours (17.9 dB against 5.5 dB).  An ordering, no threshold."""
    r = aref.closed_loop()
    print(f"closed loop, restatement: textured {r['psnr_textured']:.2f} dB, vertex colours {r['psnr_vertex']:.2f} dB, "
          f"{r['baked']['seen'].mean():.3f} of the texels seen")
    assert r["psnr_textured"] > r["psnr_vertex"]
    assert all((f["triangle"] >= 0).mean() > 0.5 for f in r["first"])


# ---- write_obj -------------------------------------------------------------------------------------------------------------

def _read_obj(path):
    v, vn, vt, faces, mtllib, usemtl = [], [], [], [], None, None
    for line in open(path):
        w = line.split()
        if not w or w[0].startswith("#"):
            continue
        if w[0] == "v":
            v.append([float(x) for x in w[1:]])
        elif w[0] == "vn":
            vn.append([float(x) for x in w[1:]])
        elif w[0] == "vt":
            vt.append([float(x) for x in w[1:]])
        elif w[0] == "f":
            faces.append([[int(x) for x in c.split("/")] for c in w[1:]])
        elif w[0] == "mtllib":
            mtllib = w[1]
        elif w[0] == "usemtl":
            usemtl = w[1]
    return np.array(v), np.array(vn), np.array(vt), np.array(faces), mtllib, usemtl


@pytest.mark.parametrize("cols", [None, 2])
def test_write_obj_read_back(tmp_path, cols):
    from PIL import Image
    ver, tri = mref.soup(7, 3)
    tri = np.array([[0, 1, 2], [2, 1, 3], [4, 5, 6], [6, 5, 7], [8, 9, 10], [10, 11, 12], [13, 14, 15]], dtype=np.int32)
    nrm = np.random.default_rng(2).normal(size=ver.shape).astype(F)
    lay = aref.layout(7, 7, cols)
    tex8 = np.random.default_rng(3).integers(0, 256, size=(lay["height"], lay["width"], 3), dtype=np.uint8)
    mesh = {"vertices": torch.from_numpy(ver), "normals": nrm, "triangles": torch.from_numpy(tri)}
    geometry.write_obj(tmp_path / "thing.obj", mesh, dict(lay, texture_u8=torch.from_numpy(tex8)))
    assert sorted(os.listdir(tmp_path)) == ["thing.mtl", "thing.obj", "thing.png"]
    v, vn, vt, faces, mtllib, usemtl = _read_obj(tmp_path / "thing.obj")
    assert mtllib == "thing.mtl" and usemtl == "thing"
    mtl = open(tmp_path / "thing.mtl").read().split()
    assert mtl[mtl.index("newmtl") + 1] == "thing" and mtl[mtl.index("map_Kd") + 1] == "thing.png"
    png = np.asarray(Image.open(tmp_path / "thing.png").convert("RGB"))
    assert np.array_equal(png, tex8)
    assert np.array_equal(v.astype(F), ver) and np.array_equal(vn.astype(F), nrm)
    assert faces.shape == (7, 3, 3) and np.array_equal(faces[:, :, 0] - 1, tri) and np.array_equal(faces[:, :, 2], faces[:, :, 0])
    assert vt.shape == (21, 2) and np.array_equal(faces[:, :, 1].reshape(-1), np.arange(1, 22))
    # the PNG sampled at each corner's vt gives that corner's texel: a viewer's u runs right, its v UP from the bottom row
    H, W = png.shape[:2]
    x, y = vt[:, 0] * W - 0.5, (1.0 - vt[:, 1]) * H - 0.5
    assert np.abs(x - np.rint(x)).max() < 1e-9 and np.abs(y - np.rint(y)).max() < 1e-9
    uv = geometry.atlas_uv(lay, 7).reshape(-1, 2)
    assert np.array_equal(np.rint(x), uv[:, 0]) and np.array_equal(np.rint(y), uv[:, 1])
    tr_all = aref.texels(lay)[0].reshape(H, W)
    assert np.array_equal(tr_all[uv[:, 1].astype(int), uv[:, 0].astype(int)], np.repeat(np.arange(7), 3))
    assert np.array_equal(png[np.rint(y).astype(int), np.rint(x).astype(int)], tex8[uv[:, 1].astype(int), uv[:, 0].astype(int)])
    # any of the three names, or the bare stem
    geometry.write_obj(str(tmp_path / "other"), mesh, dict(lay, texture_u8=tex8))
    assert os.path.exists(tmp_path / "other.obj") and os.path.exists(tmp_path / "other.png")


def test_write_obj_refusals(tmp_path):
    ver, tri = mref.soup(4, 3)
    lay = aref.layout(4, 6)
    tex8 = np.zeros((lay["height"], lay["width"], 3), np.uint8)
    mesh = {"vertices": ver, "normals": ver, "triangles": tri}
    bad_tri = tri.copy()
    bad_tri[2, 1] = 12
    for m, a in ((dict(mesh, triangles=bad_tri), dict(lay, texture_u8=tex8)),
                 (dict(mesh, triangles=-tri), dict(lay, texture_u8=tex8)),
                 (dict(mesh, normals=ver[:5]), dict(lay, texture_u8=tex8)),
                 (mesh, dict(lay, texture_u8=tex8[:, :6])),
                 (mesh, dict(lay, texture_u8=tex8.astype(F))),
                 (mesh, dict(cell=6, cols=1, texture_u8=tex8[:, :6])),           # one cell of the two that 4 triangles need
                 (mesh, dict(lay)), (mesh, dict(texture_u8=tex8, cell=6)), (mesh, None),
                 (mesh, dict(lay, texture_u8=tex8, cell=5))):
        with pytest.raises(ValueError):
            geometry.write_obj(tmp_path / "x.obj", m, a)
    assert os.listdir(tmp_path) == []


# ---- the Python layer's refusals that need no device ---------------------------------------------------------------------------

def test_extract_mesh_and_bake_texture_refuse_bad_arguments():
    with pytest.raises(ValueError, match="color_from"):
        geometry.extract_mesh({}, {}, (0, 0, 0), (1, 1, 1), (4, 4, 4), 0.5, texture=16)          # nothing to bake from
    for cell in (5, 1025):
        with pytest.raises(ValueError, match="cell"):
            geometry.extract_mesh({}, {}, (0, 0, 0), (1, 1, 1), (4, 4, 4), 0.5, texture=cell, color_from=object())
    ver, tri = mref.soup(4, 3)
    cpu = {"vertices": torch.from_numpy(ver), "normals": torch.from_numpy(ver), "triangles": torch.from_numpy(tri)}
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.bake_texture(cpu, None, 0.05)
    with pytest.raises(ValueError):
        geometry.bake_texture({"vertices": cpu["vertices"]}, None, 0.05)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.render_mesh(cpu, bank=None, image=0, texture={"texture": cpu["vertices"], "cell": 6, "cols": 1})
    for bad in (dict(), dict(cell=6, cols=1), dict(texture=None, texture_u8=None, cell=6, cols=1), 7):
        with pytest.raises(ValueError, match="texture"):
            geometry.images._atlas_of(bad, 4, torch.device("cpu"))
