"""CPU-side checks of the mesh distance (nerf_fl_amd.meshdist, csrc/nfl_meshdist.hip): the nine C entry points refuse bad
arguments before any launch (their structs and signatures are held to the header in tests/test_abi_cpu.py); the module stands
beside the geometry package without growing it; the numpy restatement (tests/meshdist_ref.py), which the GPU tests hold the
kernels to bit for bit, is checked on hand cases whose expected numbers are written out, and on two squares whose distances
are known in closed form; read_ply reads back what write_ply writes.  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meshdist_ref as dref
from abi_probe import L, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL, ESMALL = -1, -4
INF, NAN = np.inf, np.nan


# ---- sources and validation ------------------------------------------------------------------------------------------------

def test_the_restatement_has_the_columns_of_the_header():
    constants = probe()["constants"]
    assert ((constants["NFL_MESHDIST_COLUMNS"], constants["NFL_MESHDIST_MAX_TAU"]) == (_lib.MESHDIST_COLUMNS, _lib.MESHDIST_MAX_TAU)
            == (dref.COLUMNS, dref.MAX_TAU))


def test_the_unit_is_built_and_has_its_section():
    assert "---- mesh distance:" in open(os.path.join(ROOT, "include", "nerf_fl_amd.h")).read()
    make = open(os.path.join(ROOT, "nerf_fl_amd", "csrc", "Makefile")).read()
    assert "nfl_meshdist.o" in make.split("all:")[0]                       # in OBJS
    assert re.search(r"^nfl_meshdist\.o:.*nfl_geom\.h.*nfl_geom_layout\.h.*nfl_trigrid\.h", make, flags=re.M)


def test_sizes(L):
    assert L.nfl_trigrid_bytes(4, 4, 4) == 64 * 4 + 64 * 8 and L.nfl_trigrid_bytes(1, 1, 1) == 32
    for bad in ((0, 4, 4), (4, 65536, 4), (1024, 1024, 1025), (-1, 1, 1)):
        assert L.nfl_trigrid_bytes(*bad) == 0, bad
    assert L.nfl_trigrid_bytes(1024, 1024, 1024) > 12 << 30
    assert L.nfl_mesh_sample_bytes(100) == 400 + 800 and L.nfl_mesh_sample_bytes(0) == 0
    assert L.nfl_mesh_sample_bytes(-1) == 0 and L.nfl_mesh_sample_bytes((2 ** 31 - 1) // 3 + 1) == 0
    assert L.nfl_meshdist_reduce_bytes(0) == 0 and L.nfl_meshdist_reduce_bytes(1) == 112 == L.nfl_meshdist_reduce_bytes(256)
    assert L.nfl_meshdist_reduce_bytes(257) == 208 and L.nfl_meshdist_reduce_bytes(70001) == 274 * 104
    assert L.nfl_meshdist_reduce_bytes(2 ** 31 - 1) == 1024 * 104 and L.nfl_meshdist_reduce_bytes(2 ** 31) == 0


def _grid_args():
    a = _lib.TriGridArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 0x2000, 30, 10
    a.lo[:], a.cell, a.dims[:] = (-1.0, -1.0, -1.0), 0.5, (4, 4, 4)
    a.d_scratch, a.scratch_bytes, a.d_totals = 0x3000, 768, 0x4000
    a.n_entries, a.d_offsets, a.d_entries = 20, 0x5000, 0x6000
    return a


def test_grid_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    for fn in (L.nfl_trigrid_count, L.nfl_trigrid_emit):
        assert fn(None, None) == EINVAL
        for field, bad in (("d_vertices", None), ("d_triangles", None), ("d_vertices", 0x1002), ("d_triangles", 0x2001),
                           ("n_vertices", -1), ("n_triangles", -1), ("n_vertices", 1 << 31), ("n_triangles", (2 ** 31 - 1) // 3 + 1),
                           ("cell", 0.0), ("cell", -1.0), ("cell", NAN), ("cell", INF), ("d_scratch", None), ("d_scratch", 0x3004)):
            a = _grid_args()
            setattr(a, field, bad)
            assert fn(C.byref(a), None) == EINVAL, (field, bad)
        for k in range(3):
            for bad in (0, -1, 65536):
                a = _grid_args()
                a.dims[k] = bad
                assert fn(C.byref(a), None) == EINVAL, (k, bad)
            for bad in (NAN, INF):
                a = _grid_args()
                a.lo[k] = bad
                assert fn(C.byref(a), None) == EINVAL, (k, bad)
        a = _grid_args()
        a.dims[:] = (1024, 1024, 1025)                                    # cells above NG_MAX_POINTS
        assert fn(C.byref(a), None) == EINVAL
        a = _grid_args()
        a.scratch_bytes = 767
        assert fn(C.byref(a), None) == ESMALL
    for field, bad in (("d_totals", None), ("d_totals", 0x4004)):
        a = _grid_args()
        setattr(a, field, bad)
        assert L.nfl_trigrid_count(C.byref(a), None) == EINVAL, (field, bad)
    for field, bad in (("n_entries", -1), ("n_entries", 1 << 31), ("d_offsets", None), ("d_offsets", 0x5004), ("d_entries", None),
                       ("d_entries", 0x6002)):
        a = _grid_args()
        setattr(a, field, bad)
        assert L.nfl_trigrid_emit(C.byref(a), None) == EINVAL, (field, bad)


def _closest_args(grid=True):
    a = _lib.MeshClosestArgs()
    a.d_points, a.n_points, a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 50, 0x2000, 0x3000, 30, 10
    if grid:
        a.d_offsets, a.d_entries, a.n_entries = 0x4000, 0x5000, 20
        a.lo[:], a.cell, a.dims[:] = (-1.0, -1.0, -1.0), 0.5, (4, 4, 4)
    a.max_distance = INF
    a.d_distance, a.d_triangle, a.d_point, a.d_bary = 0x6000, 0x7000, 0x8000, 0x9000
    return a


def test_closest_refuses_before_any_launch(L):
    assert L.nfl_mesh_closest(None, None) == EINVAL
    for grid in (True, False):
        for field, bad in (("d_points", None), ("d_points", 0x1002), ("n_points", -1), ("n_points", 1 << 31),
                           ("d_vertices", None), ("d_triangles", None), ("d_vertices", 0x2001), ("d_triangles", 0x3002),
                           ("n_vertices", -1), ("n_triangles", -1), ("n_vertices", 1 << 31), ("max_distance", 0.0),
                           ("max_distance", -1.0), ("max_distance", NAN), ("d_distance", None), ("d_triangle", None),
                           ("d_point", None), ("d_bary", None), ("d_distance", 0x6002), ("d_triangle", 0x7001),
                           ("d_point", 0x8002), ("d_bary", 0x9003), ("d_normals", 0xA000), ("d_dot", 0xB000)):
            a = _closest_args(grid)
            setattr(a, field, bad)
            assert L.nfl_mesh_closest(C.byref(a), None) == EINVAL, (grid, field, bad)
        for nrm, dot_ in ((0xA002, 0xB000), (0xA000, 0xB002)):
            a = _closest_args(grid)
            a.d_normals, a.d_dot = nrm, dot_
            assert L.nfl_mesh_closest(C.byref(a), None) == EINVAL
        a = _closest_args(grid)                                           # no query: NFL_OK without a launch
        a.n_points = 0
        assert L.nfl_mesh_closest(C.byref(a), None) == 0
    for field, bad in (("cell", 0.0), ("cell", NAN), ("cell", INF), ("d_offsets", 0x4004), ("d_entries", None), ("d_entries", 0x5002),
                       ("n_entries", -1), ("n_entries", 1 << 31)):
        a = _closest_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_closest(C.byref(a), None) == EINVAL, (field, bad)
    for k in range(3):
        for bad in (0, 65536):
            a = _closest_args()
            a.dims[k] = bad
            assert L.nfl_mesh_closest(C.byref(a), None) == EINVAL
        a = _closest_args()
        a.lo[k] = NAN
        assert L.nfl_mesh_closest(C.byref(a), None) == EINVAL


def _sample_args():
    a = _lib.MeshSampleArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles, a.seed, a.density = 0x1000, 0x2000, 30, 10, 7, 100.0
    a.d_scratch, a.scratch_bytes, a.d_totals = 0x3000, 128, 0x4000
    a.n_samples, a.d_points, a.d_sample_triangles, a.d_normals = 40, 0x5000, 0x6000, 0x7000
    return a


def test_sample_refuses_before_any_launch(L):
    assert L.nfl_mesh_sample_bytes(10) == 128
    for fn in (L.nfl_mesh_sample_count, L.nfl_mesh_sample_emit):
        assert fn(None, None) == EINVAL
        for field, bad in (("d_vertices", None), ("d_triangles", None), ("d_vertices", 0x1001), ("d_triangles", 0x2002),
                           ("n_vertices", -1), ("n_triangles", -1), ("n_vertices", 1 << 31), ("density", -1.0), ("density", NAN),
                           ("density", INF), ("d_scratch", None), ("d_scratch", 0x3004)):
            a = _sample_args()
            setattr(a, field, bad)
            assert fn(C.byref(a), None) == EINVAL, (field, bad)
        a = _sample_args()
        a.scratch_bytes = 127
        assert fn(C.byref(a), None) == ESMALL
    for field, bad in (("d_totals", None), ("d_totals", 0x4004)):
        a = _sample_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_sample_count(C.byref(a), None) == EINVAL
    for field, bad in (("n_samples", -1), ("n_samples", 1 << 31), ("d_points", None), ("d_sample_triangles", None), ("d_normals", None),
                       ("d_points", 0x5002), ("d_sample_triangles", 0x6001), ("d_normals", 0x7002)):
        a = _sample_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_sample_emit(C.byref(a), None) == EINVAL, (field, bad)
    a = _sample_args()                                                    # no sample: NFL_OK without a launch
    a.n_samples = 0
    assert L.nfl_mesh_sample_emit(C.byref(a), None) == 0


def _reduce_args():
    a = _lib.MeshDistReduceArgs()
    a.d_distance, a.d_dot, a.n, a.n_tau = 0x1000, 0x2000, 1000, 2
    a.tau[:2] = (0.1, 0.2)
    a.d_scratch, a.scratch_bytes, a.d_row = 0x3000, 4 * 104, 0x4000
    return a


def test_reduce_refuses_before_any_launch(L):
    assert L.nfl_meshdist_reduce(None, None) == EINVAL
    for field, bad in (("d_distance", None), ("d_distance", 0x1002), ("d_dot", 0x2001), ("n", -1), ("n", 1 << 31), ("n_tau", -1),
                       ("n_tau", 9), ("d_scratch", None), ("d_scratch", 0x3004), ("d_row", None), ("d_row", 0x4004)):
        a = _reduce_args()
        setattr(a, field, bad)
        assert L.nfl_meshdist_reduce(C.byref(a), None) == EINVAL, (field, bad)
    a = _reduce_args()
    a.tau[1] = NAN
    assert L.nfl_meshdist_reduce(C.byref(a), None) == EINVAL
    a = _reduce_args()
    a.scratch_bytes -= 1
    assert L.nfl_meshdist_reduce(C.byref(a), None) == ESMALL


def test_the_module_stands_beside_the_geometry_package():
    pkg = os.path.join(ROOT, "nerf_fl_amd")
    source = open(os.path.join(pkg, "meshdist.py")).read()
    assert "_lib.check(" not in source and "C.byref(" not in source and "import ctypes" not in source
    imported = re.search(r"^from \.geometry\._call import \((.*?)\)$", source, flags=re.M | re.S).group(1)
    for helper in ("_launch", "_count", "_mesh_tensors", "_refuse_outside", "_f32", "_positive", "_seed"):
        assert re.search(rf"\b{helper}\b", imported), helper
    # read_ply stands beside write_ply and is public here; its helpers went with it
    assert re.search(r"^from \.geometry\.files import read_ply$", source, flags=re.M) and "_ply_" not in source and "_PLY_" not in source
    files = open(os.path.join(pkg, "geometry", "files.py")).read()
    assert "def read_ply(" in files and "def _ply_header(" in files and "def write_ply(" in files
    # one reduction of a finite box, on the device; each user keeps its one read and its zero fallback
    assert source.count("def _finite_box(") == 1 and source.count("_finite_box(") == 2
    assert "def _mesh_or_grid(" in source and "def _grid_or_mesh" not in source
    assert source.count("method: 'grid' or 'brute', got {method!r}") == 1
    assert sorted(n for n in os.listdir(os.path.join(pkg, "geometry")) if n.endswith(".py")) == [
        "__init__.py", "_call.py", "files.py", "images.py", "lattice.py", "mesh.py", "occupancy.py"]
    from nerf_fl_amd import fusion, geometry, meshdist
    assert meshdist.read_ply is geometry.files.read_ply and not hasattr(geometry, "read_ply")
    assert meshdist.__all__ == ["triangle_grid", "closest_on_mesh", "sample_surface", "mesh_distance", "read_ply"]
    assert len(geometry.__all__) == 24 and not set(meshdist.__all__) & set(geometry.__all__)
    assert fusion.__all__ == ["depth_maps", "fuse_depth", "tsdf_lattice", "surface_support", "drop_unsupported", "fuse_mesh"]
    assert "usual practice" in meshdist.triangle_grid.__doc__ and "MEASURED" in meshdist.triangle_grid.__doc__
    for bad in (dict(points="faces"), dict(thresholds=range(9)), dict(thresholds=(NAN,))):      # refused before any tensor is looked at
        with pytest.raises(ValueError):
            meshdist.mesh_distance(None, None, **bad)


# ---- the restatement: hand cases ---------------------------------------------------------------------------------------------

TRI = (F([0, 0, 0]), F([1, 0, 0]), F([0, 1, 0]))


def test_one_triangle_from_each_of_its_seven_regions_and_from_its_plane():
    p = [[-1, -1, 0], [2, -0.5, 0], [0.5, -1, 0], [-0.5, 2, 0], [-1, 0.5, 0], [1, 1, 0], [0.25, 0.25, 2], [0.25, 0.5, 0]]
    q, uvw, dd, region = dref.point_triangle(F(p), *TRI)
    assert region.tolist() == [1, 2, 3, 4, 5, 6, 7, 7]
    assert q.tolist() == [[0, 0, 0], [1, 0, 0], [0.5, 0, 0], [0, 1, 0], [0, 0.5, 0], [0.5, 0.5, 0], [0.25, 0.25, 0], [0.25, 0.5, 0]]
    assert uvw.tolist() == [[1, 0, 0], [0, 1, 0], [0.5, 0.5, 0], [0, 0, 1], [0.5, 0, 0.5], [0, 0.5, 0.5], [0.5, 0.25, 0.25],
                            [0.25, 0.25, 0.5]]
    assert dd.tolist() == [2, 1.25, 1, 1.25, 1, 0.5, 4, 0]
    assert q.dtype == uvw.dtype == dd.dtype == F
    got = dref.closest(F(p), np.stack(TRI), [[0, 1, 2]], normals=np.tile(F([0, 0, -2]), (8, 1)))
    assert got["distance"].tolist() == [F(np.sqrt(F(2))), F(np.sqrt(F(1.25))), 1, F(np.sqrt(F(1.25))), 1, F(np.sqrt(F(0.5))), 2, 0]
    assert got["triangle"].tolist() == [0] * 8 and got["dot"].tolist() == [-2] * 8
    got = dref.closest(F(p), np.stack(TRI), [[0, 1, 2]], max_distance=1.0)          # dd <= 1: four of the eight
    assert got["triangle"].tolist() == [-1, -1, 0, -1, 0, 0, -1, 0]
    assert np.isinf(got["distance"][[0, 1, 3, 6]]).all() and np.isnan(got["point"][0]).all() and np.isnan(got["bary"][6]).all()


def test_a_tie_between_two_triangles_goes_to_the_lower_index():
    sq = dref.square()
    p = F([[0.5, 0.5, 1.0], [0.25, 0.25, -2.0], [0.9, 0.1, 0.5], [0.1, 0.9, 0.5]])       # on the shared edge twice, then one each
    got = dref.closest(p, sq["vertices"], sq["triangles"])
    assert got["triangle"].tolist() == [0, 0, 0, 1] and got["distance"].tolist() == [1.0, 2.0, 0.5, 0.5]
    got = dref.closest(p, sq["vertices"], sq["triangles"][::-1])                       # the index decides, not the triangle
    assert got["triangle"].tolist() == [0, 0, 1, 0]
    assert got["bary"][0].tolist() == [0.5, 0.5, 0.0]                                # triangle (0, 2, 3): on its edge 0-2


def test_degenerate_and_unusable_triangles():
    ver = F([[1, 1, 1], [0, 0, 0], [1, 0, 0], [2, 0, 0], [NAN, 0, 0], [5, 5, 5]])
    point = dref.closest(F([[0, 0, 0]]), ver, [[0, 0, 0]])                            # a point: region 1, its corner
    assert point["distance"].tolist() == [F(np.sqrt(F(3)))] and point["point"].tolist() == [[1, 1, 1]]
    line = dref.closest(F([[1.5, 1, 0]]), ver, [[1, 2, 3]])                           # collinear: the edge regions still answer
    assert line["distance"].tolist() == [1.0] and line["point"].tolist() == [[1.5, 0, 0]] and line["bary"].tolist() == [[0.25, 0, 0.75]]
    # a NaN corner, an index out of range: never the answer, listed nowhere, no sample
    tri = [[4, 1, 2], [1, 2, 6], [1, 2, -1], [5, 5, 5]]
    got = dref.closest(F([[0.5, 0.1, 0]]), ver, tri)
    assert got["triangle"].tolist() == [3]
    assert dref.usable(ver, tri).tolist() == [False, False, False, True] and dref.outside(ver, tri) == 2
    rows, totals = dref.grid_rows(ver, tri, (0.0, 0.0, 0.0), 1.0, (6, 6, 6))
    assert totals == (1, 2) and rows[(5 * 6 + 5) * 6 + 5] == [3] and sum(len(r) for r in rows) == 1
    m, _, totals = dref.sample_counts(ver, tri, 1000.0, 3)
    assert m.tolist() == [0, 0, 0, 0] and totals == (0, 2, 0)
    none = dref.closest(F([[0, 0, 0], [NAN, 0, 0]]), ver[:0], np.zeros((0, 3), np.int32))        # an empty mesh
    assert none["triangle"].tolist() == [-1, -1] and np.isinf(none["distance"]).all() and np.isnan(none["point"]).all()
    assert dref.closest(F([[INF, 0, 0]]), ver, [[1, 2, 5]])["triangle"].tolist() == [-1]      # a query that is no point


def test_cell_function_and_rows():
    x = F([-5, -1, -0.75, -0.5, 0, 0.49, 0.5, 0.99, 1, 7, NAN, INF, -INF])
    assert dref.cellf(x, -1.0, 0.5, 4).tolist() == [0, 0, 0, 1, 2, 2, 3, 3, 3, 3, 0, 3, 0]
    assert (np.diff(dref.cellf(np.sort(np.random.default_rng(0).uniform(-3, 3, 1000)), -1.0, 1 / 3, 7)) >= 0).all()
    ver = F([[-1, -1, -1], [1, -1, -1], [-1, 1, 1], [0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1]])
    rows, totals = dref.grid_rows(ver, [[0, 1, 2], [3, 4, 5]], (-1.0, -1.0, -1.0), 0.5, (4, 4, 4))
    assert all(0 in r for r in rows) and totals == (64 + 1, 0)                      # the first spans the box: in every cell
    assert [c for c, r in enumerate(rows) if 1 in r] == [(2 * 4 + 2) * 4 + 2]


def test_samples_of_a_hand_mesh():
    ver = F([[0, 0, 0], [2, 0, 0], [0, 1, 0], [0, 0, 0.001], [0.001, 0, 0], [1, 1, 1], [1, 1, 1]])
    tri = [[0, 1, 2], [0, 3, 4], [5, 6, 5], [0, 2, 1]]
    m, ht, totals = dref.sample_counts(ver, tri, 50.5, 11)
    assert m[0] in (50, 51) and m[3] in (50, 51) and m[1] == 0 and m[2] == 0 and totals == (int(m.sum()), 0, 0)
    assert ht[0] != ht[3]
    pts, t, nrm = dref.samples(ver, tri, 50.5, 11)
    assert pts.dtype == nrm.dtype == F and t.dtype == np.int32 and (np.diff(t) >= 0).all()
    assert (pts[:, 2] == 0).all() and (pts[:, 0] >= 0).all() and (pts[:, 1] >= 0).all() and (pts[:, 0] / 2 + pts[:, 1] <= 1 + 1e-6).all()
    assert nrm[t == 0].tolist() == [[0, 0, 1]] * int(m[0]) and nrm[t == 3].tolist() == [[0, 0, -1]] * int(m[3])
    assert not np.array_equal(pts[t == 0], pts[t == 3][:m[0]])
    _, _, totals = dref.sample_counts(ver, tri, 2.0 ** 24, 11)
    assert totals[2] == 2                                                            # area 1 x 2^24 samples: refused
    many = dref.sample_counts(ver, tri, 1e4, 5)[0]                                   # the expected count is area * density
    assert abs(int(many[0]) - 10000) <= 1 and many[1] in (0, 1)
    counts = [dref.sample_counts(ver, tri, 0.25, s)[0][0] for s in range(400)]       # area 1, density 0.25: 0 or 1, a quarter 1
    assert set(counts) == {0, 1} and abs(sum(counts) / 400 - 0.25) < 5 * np.sqrt(0.25 * 0.75 / 400)


def test_reduction_row():
    d = F([0.5, INF, 0.25, NAN, 1.0])
    row = dref.reduce_row(d, F([1.0, NAN, -0.5, 0.0, 0.25]), (0.25, 0.6))
    assert row.tolist() == [3, 1.75, 0.25 + 0.0625 + 1.0, 1.0, 1, 2, 0, 0, 0, 0, 0, 0, 1.75]
    assert dref.reduce_row(d[:0]).tolist() == [0] * 13 and dref.reduce_row(F([INF, INF]), None, (1.0,)).tolist() == [0] * 13
    rng = np.random.default_rng(1)
    big = rng.random(70001).astype(F)
    row = dref.reduce_row(big, None, (0.5,))
    assert row[0] == 70001 and row[3] == big.max() and row[4] == (big <= F(0.5)).sum()
    assert abs(row[1] - big.astype(np.float64).sum()) < 1e-7 and row[1] != np.cumsum(big.astype(np.float64))[-1]    # a fixed order, not the sequential one


# ---- analytic checks of the restatement (tests/test_meshdist_gpu.py repeats them on the device) -------------------------------

def test_square_shifted_along_its_normal():
    r = dref.mesh_distance(dref.square(), dref.square((0, 0, 0.25)), n=2000, thresholds=(0.2, 0.3), seed=3)
    assert 1900 < r["a_to_b"]["n"] < 2100
    assert (np.abs(r["distances_a_to_b"] - 0.25) <= 1e-6).all()
    dref.check_shifted_along_the_normal(r)


def test_square_shifted_in_its_plane():
    r = dref.mesh_distance(dref.square(), dref.square((0.5, 0, 0)), n=4000, seed=5)
    dref.check_shifted_in_the_plane(r["a_to_b"])
    dref.check_shifted_in_the_plane(r["b_to_a"])
    assert abs(r["normal_consistency"] - 1.0) <= 1e-6


# ---- read_ply ----------------------------------------------------------------------------------------------------------------

def _mesh(seed=0, V=37, T=55):
    rng = np.random.default_rng(seed)
    return {"vertices": rng.normal(size=(V, 3)).astype(F), "normals": rng.normal(size=(V, 3)).astype(F),
            "triangles": rng.integers(0, V, (T, 3)).astype(np.int32)}


def test_read_ply_round_trip_is_exact(tmp_path):
    from nerf_fl_amd import geometry, meshdist
    mesh = _mesh()
    mesh["vertices"][3, 1] = NAN                                                    # bits, not values
    col = np.random.default_rng(1).random((37, 3)).astype(F)
    for colors in (None, col):
        path = str(tmp_path / "m.ply")
        geometry.write_ply(path, mesh, colors)
        got = meshdist.read_ply(path)
        for k in ("vertices", "normals", "triangles"):
            assert got[k].dtype == mesh[k].dtype and got[k].tobytes() == mesh[k].tobytes(), k
        assert ("colors" in got) == (colors is not None)
        if colors is not None:
            assert np.array_equal(got["colors"], np.rint(col * 255).astype(np.uint8).astype(F) / F(255))
            again = str(tmp_path / "again.ply")
            geometry.write_ply(again, got, got["colors"])
            assert open(again, "rb").read() == open(path, "rb").read()
    empty = {"vertices": np.zeros((0, 3), F), "normals": np.zeros((0, 3), F), "triangles": np.zeros((0, 3), np.int32)}
    geometry.write_ply(path, empty)
    assert meshdist.read_ply(path)["vertices"].shape == (0, 3)


ASCII = """ply
format ascii 1.0
comment a ground-truth mesh as exporters write it
element vertex 4
property float32 x
property float32 y
property float32 z
property uint8 red
property uint8 green
property uint8 blue
element face 2
property list uint8 uint32 vertex_index
end_header
0 0 0 255 0 0
1 0 0 0 255 0
1 1 0.5 0 0 255
0 1 -1e-3 51 102 204
3 0 1 2
3 0 2 3
"""


def test_read_ply_ascii(tmp_path):
    from nerf_fl_amd import meshdist
    path = tmp_path / "a.ply"
    path.write_text(ASCII)
    got = meshdist.read_ply(str(path))
    assert got["vertices"].tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, F(-1e-3)]]
    assert got["triangles"].tolist() == [[0, 1, 2], [0, 2, 3]] and got["triangles"].dtype == np.int32
    assert got["normals"].tolist() == [[0, 0, 0]] * 4                               # none in the file, and no device to fill them on
    assert got["colors"][3].tolist() == [F(51) / F(255), F(102) / F(255), F(204) / F(255)]


@pytest.mark.parametrize("old,new,found", [
    ("format ascii 1.0", "format binary_big_endian 1.0", "binary_big_endian"),
    ("property float32 z", "property double z", "double"),
    ("property uint8 blue", "property uint8 blue\nproperty uint8 alpha", "alpha"),
    ("property uint8 blue\n", "", "come together"),
    ("property float32 z\n", "", "x, y and z"),
    ("element face 2", "element edge 0\nelement face 2", "edge"),
    ("property list uint8 uint32 vertex_index", "property list uint8 float vertex_index", "float vertex_index"),
    ("property list uint8 uint32 vertex_index", "property list uint8 uint32 indices", "indices"),
    ("3 0 2 3\n", "4 0 2 3 1\n", "numbers"),
    ("3 0 2 3\n", "2 0 2 3\n", "a face of 2"),
    ("3 0 2 3\n", "3 0 2 4\n", "outside"),
    ("3 0 2 3\n", "3 0 2 x\n", "not a number"),
    ("end_header\n", "", "header line '0 0 0 255 0 0'"),
    ("ply\n", "plx\n", "not a PLY"),
    ("comment a ground", "garbage a ground", "garbage"),
])
def test_read_ply_refuses_what_it_does_not_read(tmp_path, old, new, found):
    from nerf_fl_amd import meshdist
    assert old in ASCII
    path = tmp_path / "bad.ply"
    path.write_text(ASCII.replace(old, new))
    with pytest.raises(ValueError, match=re.escape(found)):
        meshdist.read_ply(str(path))


def test_read_ply_refuses_a_truncated_binary_body(tmp_path):
    from nerf_fl_amd import geometry, meshdist
    path = str(tmp_path / "m.ply")
    geometry.write_ply(path, _mesh())
    raw = open(path, "rb").read()
    open(path, "wb").write(raw[:-5])
    with pytest.raises(ValueError, match="bytes"):
        meshdist.read_ply(path)
