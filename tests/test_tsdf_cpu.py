"""CPU-side checks of depth fusion (nerf_fl_amd.fusion, csrc/nfl_tsdf.hip): the three C entry points refuse bad arguments before
any launch (their structs and signatures are held to the header in tests/test_abi_cpu.py); the module stands beside the geometry package without growing it; the numpy
restatement (tests/tsdf_ref.py), which the GPU tests hold the kernels to bit for bit, is checked on hand cases whose expected
numbers are written out; and what the issue's prototype claimed of a fused sphere -- a second wall without the support rule,
a closed surface within one spacing of the sphere with it -- holds on the fp32 restatement.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import geometry_ref as gref
import mesh_ref
import meshcolor_ref as mref
import tsdf_ref as tref
from abi_probe import L  # noqa: F401  (a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL = -1
INF, NAN = np.inf, np.nan


# ---- sources and validation ------------------------------------------------------------------------------------------------

def test_the_unit_is_built_and_has_its_section():
    assert "---- depth fusion:" in open(os.path.join(ROOT, "include", "nerf_fl_amd.h")).read()
    make = open(os.path.join(ROOT, "nerf_fl_amd", "csrc", "Makefile")).read()
    assert "nfl_tsdf.o" in make.split("all:")[0]                           # in OBJS
    assert re.search(r"^nfl_tsdf\.o:.*nfl_meshray\.h", make, flags=re.M)


def _fuse_args():
    a = _lib.TsdfFuseArgs()
    a.d_table, a.n_images, a.first, a.count, a.start = 0x1000, 4, 1, 2, 1
    a.d_depth, a.n_depth, a.d_pixel_weights, a.d_image_weights = 0x2000, 100, 0x3000, 0x4000
    a.nx, a.ny, a.nz, a.trunc = 5, 4, 3, 0.25
    a.lo[:], a.spacing[:] = (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5)
    a.d_acc, a.d_views = 0x5000, 0x6000
    return a


def test_fuse_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    assert L.nfl_tsdf_fuse(None, None) == EINVAL
    for field in ("d_table", "d_depth", "d_acc", "d_views"):
        a = _fuse_args()
        setattr(a, field, None)
        assert L.nfl_tsdf_fuse(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_table", 0x1004), ("d_depth", 0x2002), ("d_pixel_weights", 0x3001), ("d_image_weights", 0x4002),
                        ("d_acc", 0x5004), ("d_views", 0x6002)):
        a = _fuse_args()
        setattr(a, field, addr)
        assert L.nfl_tsdf_fuse(C.byref(a), None) == EINVAL, field
    for field, bad in (("n_images", 0), ("first", -1), ("count", -1), ("first", 3), ("count", 4), ("first", 5),
                       ("nx", 1), ("ny", 1), ("nz", 1), ("nx", 0), ("ny", 65536), ("nz", 65536), ("nx", (1 << 30) // 12 + 1),
                       ("trunc", 0.0), ("trunc", -0.5), ("trunc", NAN), ("n_depth", -1), ("n_depth", (1 << 38) + 1)):
        a = _fuse_args()
        setattr(a, field, bad)
        assert L.nfl_tsdf_fuse(C.byref(a), None) == EINVAL, (field, bad)
    a = _fuse_args()                                                   # nothing to do: NFL_OK without a launch
    a.count, a.start = 0, 0
    assert L.nfl_tsdf_fuse(C.byref(a), None) == 0


def _resolve_args():
    a = _lib.TsdfResolveArgs()
    a.d_acc, a.d_views, a.nx, a.ny, a.nz, a.min_views = 0x1000, 0x2000, 5, 4, 3, 1
    a.min_weight, a.fill, a.d_lattice, a.d_known = 0.5, -1.0, 0x3000, 0x4001          # the flags are bytes: any address
    return a


def test_resolve_refuses_before_any_launch(L):
    assert L.nfl_tsdf_resolve(None, None) == EINVAL
    for field in ("d_acc", "d_views", "d_lattice", "d_known"):
        a = _resolve_args()
        setattr(a, field, None)
        assert L.nfl_tsdf_resolve(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_acc", 0x1004), ("d_views", 0x2002), ("d_lattice", 0x3001)):
        a = _resolve_args()
        setattr(a, field, addr)
        assert L.nfl_tsdf_resolve(C.byref(a), None) == EINVAL, field
    for field, bad in (("nx", 1), ("ny", 1), ("nz", 1), ("ny", 65536), ("nz", 65536), ("nx", (1 << 30) // 12 + 1),
                       ("min_weight", 0.0), ("min_weight", -1.0), ("min_weight", NAN), ("min_views", 0), ("min_views", -3),
                       ("fill", NAN)):
        a = _resolve_args()
        setattr(a, field, bad)
        assert L.nfl_tsdf_resolve(C.byref(a), None) == EINVAL, (field, bad)


def _support_args():
    a = _lib.TsdfSupportArgs()
    a.d_vertices, a.n_vertices, a.d_known, a.nx, a.ny, a.nz = 0x1000, 30, 0x2001, 5, 4, 3
    a.lo[:], a.spacing[:] = (-1.0, -1.0, -1.0), (0.5, 0.5, 0.5)
    a.d_support = 0x3001
    return a


def test_support_refuses_before_any_launch(L):
    assert L.nfl_tsdf_support(None, None) == EINVAL
    for field in ("d_vertices", "d_known", "d_support"):
        a = _support_args()
        setattr(a, field, None)
        assert L.nfl_tsdf_support(C.byref(a), None) == EINVAL, field
    a = _support_args()
    a.d_vertices = 0x1002
    assert L.nfl_tsdf_support(C.byref(a), None) == EINVAL
    for field, bad in (("nx", 1), ("ny", 1), ("nz", 1), ("ny", 65536), ("nz", 65536), ("nx", (1 << 30) // 12 + 1),
                       ("n_vertices", -1), ("n_vertices", 1 << 31)):
        a = _support_args()
        setattr(a, field, bad)
        assert L.nfl_tsdf_support(C.byref(a), None) == EINVAL, (field, bad)
    a = _support_args()                                                # no vertex: NFL_OK without a launch
    a.n_vertices, a.d_vertices, a.d_support = 0, None, None
    assert L.nfl_tsdf_support(C.byref(a), None) == 0


def test_the_module_stands_beside_the_geometry_package():
    """nerf_fl_amd.fusion is a top-level module: the geometry package keeps its 7 files (test_geometry_layout_cpu.py pins
    them and its 24 names), and the one launch line stays in geometry/_call.py."""
    pkg = os.path.join(ROOT, "nerf_fl_amd")
    source = open(os.path.join(pkg, "fusion.py")).read()
    assert "_lib.check(" not in source and "C.byref(" not in source and ".tolist()" not in source
    assert re.search(r"^from \.geometry\._call import .*\b_launch\b", source, flags=re.M)
    assert sorted(n for n in os.listdir(os.path.join(pkg, "geometry")) if n.endswith(".py")) == [
        "__init__.py", "_call.py", "files.py", "images.py", "lattice.py", "mesh.py", "occupancy.py"]
    from nerf_fl_amd import fusion, geometry
    assert fusion.__all__ == ["depth_maps", "fuse_depth", "tsdf_lattice", "surface_support", "drop_unsupported", "fuse_mesh"]
    assert len(geometry.__all__) == 24 and not set(fusion.__all__) & set(geometry.__all__)
    for text in ("opaque", "CONVENTIONS"):
        assert text in fusion.depth_maps.__doc__
    assert "convention" in fusion.fuse_mesh.__doc__


# ---- the restatement: hand cases.  9 x 9 pixels, fx = fy = 8, cx = cy = 4, the camera at the origin looking down -z: the
# lattice point (x, y, -3) projects to (4 + 8 x / 3, 4 - 8 y / 3)

CAM = dict(width=9, height=9, fx=8.0, fy=8.0, cx=4.0, cy=4.0)


def _fuse1(p, D, trunc=1.0, wp=None, wi=None, **kw):
    """The accumulators of the ONE lattice point p (corner (0, 0, 0) of a 2^3 lattice that starts there), every pixel at
    depth D."""
    depth = np.full((9, 9), D, dtype=F)
    weights = None if wp is None else [np.full((9, 9), wp, dtype=F)]
    acc, views = tref.fuse([mref.camera(**CAM)], [depth], p, (8.0, 8.0, 8.0), (2, 2, 2), trunc, weights,
                           None if wi is None else [wi], **kw)
    return acc[0, 0, 0], int(views[0, 0, 0])


def test_sign_truncation_and_hidden_points():
    p = (0.0, 0.0, -3.0)
    a, n = _fuse1(p, 3.0)                                                   # on the surface
    assert n == 1 and a[0] == 0.0 and a[1] == 1.0
    a, n = _fuse1(p, 2.5)                                                  # half a trunc BEHIND it: positive
    assert n == 1 and a[0] == 0.5 and a[1] == 1.0
    a, n = _fuse1(p, 3.25)                                                  # a quarter in front: negative
    assert n == 1 and a[0] == -0.25
    a, n = _fuse1(p, 2.0)                                                   # exactly one trunc behind: still counted
    assert n == 1 and a[0] == 1.0
    assert _fuse1(p, np.nextafter(F(2.0), F(1.0)))[1] == 0                  # an ulp more: hidden, nothing known
    a, n = _fuse1(p, 4.0)                                                   # exactly one trunc in front
    assert n == 1 and a[0] == -1.0
    assert _fuse1(p, 40.0)[0][0] == -1.0                                    # far in front: free space, saturated
    a, n = _fuse1(p, INF)                                                   # the ray hit nothing: free space
    assert n == 1 and a[0] == -1.0 and a[1] == 1.0
    a, n = _fuse1(p, 3.5, trunc=2.0)
    assert n == 1 and a[0] == -0.25


def test_words_that_say_nothing_and_weights():
    p = (0.0, 0.0, -3.0)
    for D in (NAN, 0.0, -1.0, -INF):
        assert _fuse1(p, D)[1] == 0, D
    a, n = _fuse1(p, 2.5, wp=0.5, wi=3.0)
    assert n == 1 and a[0] == 0.75 and a[1] == 1.5                          # w = wi * wp; w * phi and w
    for wp, wi in ((0.0, 1.0), (-1.0, 1.0), (NAN, 1.0), (1.0, 0.0), (1.0, -2.0), (1.0, NAN)):
        assert _fuse1(p, 2.5, wp=wp, wi=wi)[1] == 0, (wp, wi)


def test_frame_limits_and_the_camera_plane():
    assert _fuse1((-1.5, 0.0, -3.0), INF)[1] == 1 and _fuse1((1.5, 0.0, -3.0), INF)[1] == 1       # u = 0 and u = 8
    assert _fuse1((0.0, 1.5, -3.0), INF)[1] == 1 and _fuse1((0.0, -1.5, -3.0), INF)[1] == 1
    assert _fuse1((np.nextafter(F(-1.5), F(-2)), 0.0, -3.0), INF)[1] == 0
    assert _fuse1((1.6, 0.0, -3.0), INF)[1] == 0
    assert _fuse1((0.0, 0.0, 3.0), INF)[1] == 0 and _fuse1((0.0, 0.0, 0.0), INF)[1] == 0          # behind the plane, and on it
    # the depth is looked up at the NEAREST pixel: u = 4.4 reads column 4, u = 4.6 column 5
    depth = np.full((9, 9), NAN, dtype=F)
    depth[4, 5] = 3.0
    for x, n in ((3 * 0.4 / 8, 0), (3 * 0.6 / 8, 1)):
        _, views = tref.fuse([mref.camera(**CAM)], [depth], (x, 0.0, -3.0), (8.0,) * 3, (2, 2, 2), 1.0)
        assert views[0, 0, 0] == n


def test_runs_continue_to_the_same_bits():
    fx = tref.sphere_fixture(9, 3, 17)
    args = (fx["lo"], fx["spacing"], fx["res"], fx["trunc"])
    w = [F(1.0), F(0.3), F(0.0), F(2.0), F(NAN), F(0.7)]
    acc, views = tref.fuse(fx["cams"], fx["depths"], *args, image_weights=w)
    a1, v1 = tref.fuse(fx["cams"][:1], fx["depths"][:1], *args, image_weights=w[:1])
    a2, v2 = tref.fuse(fx["cams"][1:4], fx["depths"][1:4], *args, image_weights=w[1:4], acc=a1, views=v1)
    a3, v3 = tref.fuse(fx["cams"][4:], fx["depths"][4:], *args, image_weights=w[4:], acc=a2, views=v2)
    assert np.array_equal(a3.view(np.uint32), acc.view(np.uint32)) and np.array_equal(v3, views)
    assert views.max() <= 4 and views.max() >= 2


def test_resolve_thresholds():
    acc = np.array([[[[0.5, 1.0], [-0.3, 0.4]], [[0.0, 0.0], [1.5, 2.0]]]] * 2, dtype=F)       # (2, 2, 2, 2)
    views = np.array([[[1, 1], [0, 3]]] * 2, dtype=np.int32)
    lat, known = tref.resolve(acc, views, 0.5)
    assert lat.dtype == F and known.dtype == np.uint8
    assert known[0].tolist() == [[1, 0], [0, 1]] and lat[0].tolist() == [[0.5, -1.0], [-1.0, 0.75]]
    lat, known = tref.resolve(acc, views, 0.4, fill=7.0)                    # >= is inclusive ... in fp32: F(0.4) >= F(0.4)
    assert known[0].tolist() == [[1, 1], [0, 1]] and lat[0, 0, 1] == F(-0.3) / F(0.4) and lat[0, 1, 0] == 7.0
    assert tref.resolve(acc, views, 0.5, min_views=2)[1][0].tolist() == [[0, 0], [0, 1]]
    assert tref.resolve(acc, views, 0.5, min_views=3)[1][0].tolist() == [[0, 0], [0, 1]]
    assert tref.resolve(acc, views, 0.5, min_views=4)[1].sum() == 0
    assert tref.resolve(acc, views, 2.5)[1].sum() == 0


def test_support_reads_the_edge_the_face_or_the_cell():
    known = np.ones((3, 3, 3), dtype=np.uint8)                              # lattice over [0, 2]^3, spacing 1
    known[1, 1, 1] = 0
    lo, sp = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    ver = [[0, 0, 0], [1, 1, 1],                                            # ON a lattice point: that point alone
           [0.5, 0, 0], [0.5, 1, 1], [1, 1.5, 1], [2, 2, 1.5],              # axis edges: the two ends
           [0.5, 0.5, 0], [0.5, 0.5, 1], [1.5, 2, 1.5],                     # face diagonals: the four corners of the face
           [0.25, 0.25, 0.25], [1.5, 1.5, 1.5], [0.5, 0.5, 2],              # body diagonals: the eight of the cell (the last: a face)
           [2, 2, 2], [2.5, 0, 0], [0, -0.25, 0], [NAN, 0, 0], [0, INF, 0], [0, 0, np.nextafter(F(2), F(3))]]
    got = tref.support(np.array(ver, dtype=F), known, lo, sp)
    assert got.dtype == np.uint8
    assert got.tolist() == [1, 0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 0, 0, 0]
    assert tref.support(np.zeros((0, 3), F), known, lo, sp).shape == (0,)


# ---- the prototype's claims, on the fp32 restatement -------------------------------------------------------------------------

@pytest.fixture(scope="module")
def fused_sphere():
    fx = tref.sphere_fixture(17, 3, 33)
    acc, views = tref.fuse(fx["cams"], fx["depths"], fx["lo"], fx["spacing"], fx["res"], fx["trunc"])
    lattice, known = tref.resolve(acc, views, 0.5)
    mesh = gref.extract(lattice, 0.0, fx["lo"], fx["spacing"])
    return fx, lattice, known, mesh, tref.support(mesh["vertices"], known, fx["lo"], fx["spacing"])


def test_analytic_depth_map():
    cam = tref.sphere_cameras(33)[2]                                        # on +z, looking down -z
    d = tref.sphere_depth(cam)
    assert d.shape == (33, 33) and d.dtype == F and d[16, 16] == F(3.0 - 0.8)
    assert d[0, 0] == INF and np.isfinite(d).sum() > 100
    # the silhouette: tan of the cone is 0.8 / sqrt(9 - 0.64), times the focal length 22.4 -> 6.2 pixels
    assert np.isfinite(d[16, 16 + 6]) and d[16, 16 + 7] == INF
    assert np.array_equal(d, d[::-1]) and np.array_equal(d, d[:, ::-1]) and np.array_equal(d, d.T)


def test_unfiltered_surface_has_a_second_wall_and_the_support_rule_removes_it(fused_sphere):
    fx, lattice, known, mesh, sup = fused_sphere
    c = tref.surface_conditions(mesh, sup, tref.RADIUS, fx["spacing"][0], fx["trunc"])
    print("fused sphere, 17^3, six 33 x 33 cameras, trunc 3 cells:", c, "known", float(known.mean()))
    assert 0 < known.mean() < 1                                             # the core of the ball is hidden from every camera
    assert c["wall_unfiltered"] >= 1
    assert c["wall_kept"] == 0


def test_kept_surface_is_closed_within_one_spacing_and_has_no_orphans(fused_sphere):
    fx, lattice, known, mesh, sup = fused_sphere
    c = tref.surface_conditions(mesh, sup, tref.RADIUS, fx["spacing"][0], fx["trunc"])
    assert c["V"] > 0 and c["euler"] == 2 and c["T_even"] and c["every_edge_twice"]
    assert c["orphans"] == 0
    assert c["worst_spacings"] <= 1.0
    # ... and the filtered mesh, as filter_mesh makes it (every vertex a component of its own), is that surface
    kept = mesh_ref.compact(np.arange(len(sup)), sup.astype(bool), mesh)
    assert kept["vertices"].shape == (c["V"], 3) and kept["triangles"].shape == (c["T"], 3)
    r = np.linalg.norm(kept["vertices"].astype(np.float64), axis=1)
    assert np.abs(r - tref.RADIUS).max() <= float(fx["spacing"][0])
    assert kept["triangles"].min() == 0 and kept["triangles"].max() == c["V"] - 1
