"""CPU-side checks of mesh colour (nerf_fl_amd.geometry.mesh_depth / color_mesh_from_images, csrc/nfl_meshcolor.hip): the
C entry points refuse bad arguments before any launch (their structs and signatures are held to the header in
tests/test_abi_cpu.py); the numpy restatement
(tests/meshcolor_ref.py), which the GPU tests hold the kernels to bit for bit, is itself checked on hand cases whose
expected numbers are written out and, independent of its own fp32 arithmetic, against the same algorithm in fp64 on a
seeded triangle soup.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest

import meshcolor_ref as mref
from abi_probe import L, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

F = np.float32
EINVAL = -1
INF = np.inf


# ---- the image record and validation ------------------------------------------------------------------------------------------------

def test_the_restatement_reads_the_image_record_of_the_header():
    assert probe()["structs"]["nfl_image_rec"]["size"] == mref.RECORD.itemsize == C.sizeof(_lib.ImageRec) == 104
    assert _lib.BLEND_WEIGHTINGS == {"cos": 0, "uniform": 1}               # held to the header's enum in test_abi_cpu.py


def _depth_args():
    a = _lib.MeshDepthArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 0x2000, 30, 10
    a.d_table, a.n_images, a.first, a.count, a.d_depth, a.n_depth = 0x3000, 4, 1, 2, 0x4000, 100
    return a


def test_depth_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    assert L.nfl_mesh_depth(None, None) == EINVAL
    for field in ("d_vertices", "d_triangles", "d_table", "d_depth"):
        a = _depth_args()
        setattr(a, field, None)
        assert L.nfl_mesh_depth(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_vertices", 0x1002), ("d_triangles", 0x2001), ("d_table", 0x3004), ("d_depth", 0x4002)):
        a = _depth_args()
        setattr(a, field, addr)
        assert L.nfl_mesh_depth(C.byref(a), None) == EINVAL, field
    for field, bad in (("n_vertices", -1), ("n_vertices", 1 << 31), ("n_triangles", -1), ("n_triangles", (1 << 31) // 3 + 1),
                       ("n_images", 0), ("first", -1), ("count", -1), ("first", 3), ("count", 4), ("first", 5),
                       ("n_depth", -1), ("n_depth", (1 << 38) + 1)):
        a = _depth_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_depth(C.byref(a), None) == EINVAL, (field, bad)
    a = _depth_args()                                                # 2^31 workgroups of (triangle, image) pairs
    a.n_triangles, a.n_images, a.first, a.count = (1 << 31) // 3, 1 << 20, 0, 1 << 20
    assert L.nfl_mesh_depth(C.byref(a), None) == EINVAL


def _blend_args():
    a = _lib.MeshBlendArgs()
    a.d_vertices, a.d_normals, a.n_vertices, a.d_pixels, a.d_table = 0x1000, 0x2000, 30, 0x3000, 0x4000
    a.n_images, a.first, a.count, a.weighting, a.d_depth, a.n_depth = 4, 1, 2, 0, 0x5000, 100
    a.min_cos, a.depth_tol, a.reject, a.start, a.d_sum, a.d_views = 0.0, 0.1, 0.0, 1, 0x6000, 0x7000
    return a


def test_blend_refuses_before_any_launch(L):
    assert L.nfl_mesh_blend(None, None) == EINVAL
    for field in ("d_vertices", "d_normals", "d_pixels", "d_table", "d_depth", "d_sum", "d_views"):
        a = _blend_args()
        setattr(a, field, None)
        assert L.nfl_mesh_blend(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_vertices", 0x1002), ("d_normals", 0x2001), ("d_table", 0x4004), ("d_depth", 0x5002),
                        ("d_sum", 0x6008), ("d_views", 0x7002), ("d_center", 0x8001), ("d_image_weights", 0x8002)):
        a = _blend_args()
        setattr(a, field, addr)
        assert L.nfl_mesh_blend(C.byref(a), None) == EINVAL, field
    for field, bad in (("n_vertices", -1), ("n_vertices", 1 << 31), ("n_images", 0), ("first", -1), ("count", -1),
                       ("first", 3), ("count", 4), ("weighting", 2), ("weighting", -1), ("depth_tol", -0.5),
                       ("depth_tol", float("nan")), ("min_cos", float("nan")), ("min_cos", -0.25), ("n_depth", -1)):
        a = _blend_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_blend(C.byref(a), None) == EINVAL, (field, bad)
    for bad in (-0.1, float("nan")):                                 # reject matters once a centre is given
        a = _blend_args()
        a.d_center, a.reject = 0x8000, bad
        assert L.nfl_mesh_blend(C.byref(a), None) == EINVAL, bad
    # nothing to do: NFL_OK without a launch, whatever the pointers
    a = _blend_args()
    a.n_vertices = 0
    a.d_vertices = a.d_normals = a.d_sum = a.d_views = None
    assert L.nfl_mesh_blend(C.byref(a), None) == 0
    a = _blend_args()
    a.count, a.start = 0, 0
    assert L.nfl_mesh_blend(C.byref(a), None) == 0


# ---- depth: hand cases.  9 x 9 pixels, fx = fy = 8, cx = cy = 4: the ray of pixel (i, j) is ((i - 4) / 8, -(j - 4) / 8, -1),
# exact in fp32, and a point at distance 3 along the axis from the camera plane is 3 * that

CAM = dict(width=9, height=9, fx=8.0, fy=8.0, cx=4.0, cy=4.0)


def _depth(ver, tri, c2w=None):
    return mref.depth_map(np.array(ver, dtype=F), np.array(tri, dtype=np.int32), mref.camera(c2w=c2w, **CAM))


def test_triangle_square_on_at_distance_3():
    # its corners lie on the rays of pixels (0, 8), (8, 8) and (4, 0)
    d = _depth([[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]], [[0, 1, 2]])
    assert d.dtype == F and d.shape == (9, 9)
    assert d[4, 4] == 3.0                                            # the centre pixel: straight down the axis
    assert d[0, 4] == F(3.0) * np.sqrt(F(1.25))                      # through the vertex (0, 1.5, -3): 3 |(0, 0.5, -1)| = 3.3541
    assert d[8, 0] == d[8, 8] == F(3.0) * np.sqrt(F(1.5))            # the other two vertices: 3 |(0.5, 0.5, 1)|
    assert d[8, 4] == F(3.0) * np.sqrt(F(1.25))                      # through the edge y = -1.5: inclusive
    assert d[4, 2] == d[4, 6] == F(3.0) * np.sqrt(F(1.0625))         # through the midpoints (-+0.75, 0, -3) of the slanted edges
    assert d[4, 1] == INF and d[4, 7] == INF and d[0, 3] == INF      # one pixel outside them
    assert np.isfinite(d).sum() == 9 + 7 + 7 + 5 + 5 + 3 + 3 + 1 + 1  # rows 8 .. 0: the edge loses a pixel each side every 2 rows
    # the other winding is the same surface
    assert np.array_equal(d, _depth([[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]], [[0, 2, 1]]))


def test_nearer_of_two_parallel_quads_wins():
    quad = lambda z: [[-4, -4, z], [4, -4, z], [4, 4, z], [-4, 4, z]]
    ver = quad(-4.0) + quad(-2.0)
    tri = [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]]
    d = _depth(ver, tri)
    assert d[4, 4] == 2.0 and d[4, 0] == F(2.0) * np.sqrt(F(1.25))
    assert np.isfinite(d).all()                                      # the shared diagonal leaves no hole
    assert np.array_equal(d, _depth(ver, tri[::-1]))
    far_only = _depth(ver, tri[:2])
    assert far_only[4, 4] == 4.0


def test_triangles_that_hit_nothing():
    tri = [[0, 1, 2]]
    assert (_depth([[-1.5, -1.5, 3], [1.5, -1.5, 3], [0, 1.5, 3]], tri) == INF).all()           # behind the camera
    assert (_depth([[-1.5, -1.5, -3], [np.nan, -1.5, -3], [0, 1.5, -3]], tri) == INF).all()     # a NaN vertex
    assert (_depth([[-1.5, -1.5, -3], [np.inf, -1.5, -3], [0, 1.5, -3]], tri) == INF).all()
    assert (_depth([[0, -1, -3], [0, 1, -3], [0, 0, -5]], tri) == INF).all()      # edge-on in the plane x = 0: det == 0 on column 4
    assert (_depth([[-1, 0, -3], [0, 0, -3], [1, 0, -3]], tri) == INF).all()      # three points on a line
    assert (_depth([[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]], [[0, 1, 3]]) == INF).all()   # an index past the vertices
    assert (_depth(np.zeros((0, 3)), np.zeros((0, 3))) == INF).all()


def test_triangle_straddling_the_camera_plane():
    # from the edge y = -1, z = -3 up to the apex (0, 1, 1) BEHIND the camera plane: the median x = 0 crosses y = 0 at z = -1
    d = _depth([[-1, -1, -3], [1, -1, -3], [0, 1, 1]], [[0, 1, 2]])
    assert d[4, 4] == pytest.approx(1.0, rel=1e-6)
    # the part in front is seen all the way up the frame (the surface runs off to infinity there); below, it ends at the
    # edge y = -1, z = -3, which projects to row 4 + 8 / 3
    assert np.isfinite(d[:7, 4]).all() and (d[7:, 4] == INF).all()
    # the camera moved and turned: the same picture
    c2w = mref.look_at((3.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    R, t = c2w[:, :3], c2w[:, 3]
    world = (np.array([[-1, -1, -3], [1, -1, -3], [0, 1, 1]], dtype=np.float64) @ R.T + t)
    d2 = _depth(world, [[0, 1, 2]], c2w)
    assert np.array_equal(np.isfinite(d), np.isfinite(d2))
    assert np.allclose(d[np.isfinite(d)], d2[np.isfinite(d)], rtol=1e-5)


def test_depth_fp32_against_fp64_on_the_soup():
    """The restatement's fp32 against the same algorithm in fp64, on the issue's soup.  Pixels whose fp64 barycentrics come
    within 1e-5 of an edge of any triangle may be left out (at most 1 % of them); elsewhere coverage agrees exactly and the
    depth to 1e-5 relative (plain Moeller-Trumbore measured 1.3e-6, about 11 ulp; 8 x that because a grazing triangle divides
    by a small determinant)."""
    ver, tri = mref.soup(400, 7)
    cam = mref.camera(**mref.SOUP_CAMERA)
    d32 = mref.depth_map(ver, tri, cam)
    d64 = mref.depth_map(ver, tri, cam, dtype=np.float64)
    dx, dy = mref.pixel_rays(cam)
    a, b, c = (ver[tri[:, k]] for k in range(3))
    _, tau, u, v = mref.intersect(a, b, c, dx, dy, np.float64)
    e = 1e-5
    with np.errstate(all="ignore"):
        near = ((np.abs(u) < e) | (np.abs(v) < e) | (np.abs(1.0 - u - v) < e)) & (u > -e) & (v > -e) & (u + v < 1 + e) & (tau > 0)
    left_out = near.any(axis=0).reshape(d64.shape)
    covered = np.isfinite(d64)
    both = covered & ~left_out
    rel = np.abs(d32[both].astype(np.float64) - d64[both]) / d64[both]
    print(f"soup: {covered.mean():.3f} covered, {int(left_out.sum())} left out, worst relative difference {rel.max():.3e}")
    assert 0.5 < covered.mean() < 0.75
    assert left_out.mean() <= 0.01
    assert np.array_equal(np.isfinite(d32)[~left_out], covered[~left_out])
    assert rel.max() <= 1e-5


# ---- blend: hand cases on the same camera, nothing in the way unless said ---------------------------------------------------

def _image(channels=3, seed=3):
    return np.random.default_rng(seed).integers(0, 256, size=(9, 9, channels), dtype=np.uint8)


def _blend1(p, nrm=(0, 0, 1), image=None, depth=None, tol=0.0, **kw):
    image = _image() if image is None else image
    depth = np.full((9, 9), INF, dtype=F) if depth is None else depth
    sums, views = mref.blend(np.array([p], dtype=F), np.array([nrm], dtype=F), [mref.camera(**CAM)], [image], [depth], tol, **kw)
    return sums[0], int(views[0])


def test_vertex_on_a_pixel_gets_its_colour():
    im = _image()
    s, n = _blend1((3 * 2 / 8, -3 * (-1) / 8, -3), image=im, weighting="uniform")      # the ray of pixel (6, 3)
    assert n == 1 and s[3] == 1.0
    assert np.array_equal(s[:3], im[3, 6].astype(F) / F(255))
    s, n = _blend1((3 * 4 / 8, 3 * 4 / 8, -3), image=im, weighting="uniform")          # the corner pixel (8, 0): neighbours clamped
    assert n == 1 and np.array_equal(s[:3], im[0, 8].astype(F) / F(255))


def test_vertex_between_four_pixels_gets_their_mean():
    im = _image()
    s, n = _blend1((3 * (2.5 - 4) / 8, -3 * (3.5 - 4) / 8, -3), image=im, weighting="uniform")
    assert n == 1
    assert s[:3] == pytest.approx(im[3:5, 2:4].reshape(4, 3).astype(np.float64).mean(axis=0) / 255, abs=1e-6)


def test_cos_weighting_and_colors_of():
    im = np.full((9, 9, 3), (51, 102, 204), dtype=np.uint8)
    p = np.array([0.75, 0.0, -3.0])
    s, n = _blend1(p, nrm=(0, 0, 1), image=im)
    cos = 3 / np.sqrt(0.75 ** 2 + 9)                                 # normal . (t - p) / |t - p| with t = 0
    assert n == 1 and s[3] == pytest.approx(cos, rel=1e-6)
    assert mref.colors_of(s[None], np.array([n]))[0] == pytest.approx([0.2, 0.4, 0.8], abs=1e-6)
    assert np.array_equal(mref.colors_of(np.zeros((1, 4), F), np.array([0]), (0.1, 0.2, 0.3))[0], np.array([0.1, 0.2, 0.3], F))


def test_frame_limits_are_inclusive_and_one_ulp_beyond_is_out():
    assert _blend1((-1.5, 0, -3))[1] == 1                            # u = 4 + 8 * (-1.5 / 3) = 0
    assert _blend1((1.5, 0, -3))[1] == 1                             # u = 8 = width - 1
    assert _blend1((0, 1.5, -3))[1] == 1 and _blend1((0, -1.5, -3))[1] == 1
    u_of = lambda x: F(4) + F(8) * (F(x) / F(3))
    below = np.nextafter(F(-1.5), F(-2))
    assert u_of(below) < 0 and _blend1((below, 0, -3))[1] == 0
    x = F(1.5)
    while u_of(x) == F(8):                                           # the first x whose u is the float after 8
        x = np.nextafter(x, F(2))
    assert u_of(x) == np.nextafter(F(8), F(9)) and _blend1((x, 0, -3))[1] == 0
    assert _blend1((np.nextafter(x, F(0)), 0, -3))[1] == 1
    assert _blend1((0, 0, 3))[1] == 0 and _blend1((0, 0, 0))[1] == 0  # behind the camera plane, and on it
    assert _blend1((np.nan, 0, -3))[1] == 0


def test_hidden_vertex_and_depth_tol():
    quad = np.array([[-4, -4, -2], [4, -4, -2], [4, 4, -2], [-4, 4, -2]], dtype=F)
    depth = mref.depth_map(quad, np.array([[0, 1, 2], [0, 2, 3]]), mref.camera(**CAM))
    assert depth[4, 4] == 2.0
    assert _blend1((0, 0, -3), depth=depth, tol=0.5)[1] == 0          # 3 > 2 + 0.5
    assert _blend1((0, 0, -3), depth=depth, tol=1.0)[1] == 1          # the gap itself: <= is inclusive
    assert _blend1((0, 0, -3), depth=depth, tol=1.5)[1] == 1
    assert _blend1((0, 0, -2), depth=depth, tol=0.0)[1] == 1          # a vertex OF the quad sees through its own surface
    # the depth is looked up at the NEAREST pixel: u = 4.4 reads column 4, u = 4.6 column 5
    holes = np.full((9, 9), INF, dtype=F)
    holes[4, 4] = 1.0
    assert _blend1((3 * 0.4 / 8, 0, -3), depth=holes)[1] == 0 and _blend1((3 * 0.6 / 8, 0, -3), depth=holes)[1] == 1


def test_min_cos_zero_normal_and_zero_weight():
    p = (0, 0, -3)
    assert _blend1(p, nrm=(0, 0, 1))[1] == 1                         # facing the camera: cos = 1
    assert _blend1(p, nrm=(0, 0, -1))[1] == 0                        # facing away: cos = -1
    assert _blend1(p, nrm=(1, 0, 0))[1] == 0                         # side-on: cos = 0 is not > 0
    assert _blend1(p, nrm=(1, 0, 0), min_cos=-0.5, weighting="uniform")[1] == 1
    assert _blend1(p, nrm=(0.6, 0, 0.8), min_cos=0.75)[1] == 1 and _blend1(p, nrm=(0.6, 0, 0.8), min_cos=0.85)[1] == 0
    s, n = _blend1(p, nrm=(0, 0, 0))                                 # no gradient, no normal: counted with cos = 1
    assert n == 1 and s[3] == 1.0
    assert _blend1(p, image_weights=[0.0])[1] == 0
    s, n = _blend1(p, image_weights=[2.5])
    assert n == 1 and s[3] == 2.5


def test_rgba_is_blended_onto_white():
    im = np.zeros((9, 9, 4), dtype=np.uint8)
    im[4, 4] = (255, 0, 51, 128)
    s, n = _blend1((0, 0, -3), image=im, weighting="uniform")
    al = 128 / 255
    assert n == 1 and s[:3] == pytest.approx([1.0, 1 - al, 0.2 * al + 1 - al], abs=1e-6)
    im[4, 4] = (10, 20, 30, 0)                                       # fully transparent: white
    assert np.array_equal(_blend1((0, 0, -3), image=im, weighting="uniform")[0][:3], np.ones(3, F))


def test_reject_and_continued_accumulators():
    im = np.full((9, 9, 3), 200, dtype=np.uint8)
    odd = np.full((9, 9, 3), 40, dtype=np.uint8)
    cams = [mref.camera(**CAM)] * 3
    inf = np.full((9, 9), INF, dtype=F)
    p, nr = np.array([[0, 0, -3], [0.75, 0.375, -3]], dtype=F), np.array([[0, 0, 1]] * 2, dtype=F)
    s1, v1 = mref.blend(p, nr, cams, [im, odd, im], [inf] * 3, 0.0)
    assert v1.tolist() == [3, 3]
    c1 = mref.colors_of(s1, v1)
    assert c1[0] == pytest.approx([(400 + 40) / 3 / 255] * 3, abs=1e-6)
    s2, v2 = mref.blend(p, nr, cams, [im, odd, im], [inf] * 3, 0.0, center=c1, reject=0.3)
    assert v2.tolist() == [2, 2] and mref.colors_of(s2, v2)[0] == pytest.approx([200 / 255] * 3, abs=1e-6)
    # runs of 1 + 2 continue to the same bits as one run of 3
    sa, va = mref.blend(p, nr, cams[:1], [im], [inf], 0.0)
    sb, vb = mref.blend(p, nr, cams[1:], [odd, im], [inf] * 2, 0.0, sums=sa, views=va)
    assert np.array_equal(sb, s1) and np.array_equal(vb, v1)
