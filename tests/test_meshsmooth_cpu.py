"""CPU-side checks of the mesh smoothing (nerf_fl_amd.geometry.mesh_adjacency / smooth_mesh / vertex_normals,
csrc/nfl_meshsmooth.hip): the numpy restatement (tests/meshsmooth_ref.py), which the GPU tests hold the kernels to, on
hand-written cases with the expected rows and flags written out; the condition under which the GPU test may compare
positions on the bits (the order of the triangles and the rotation of their corners change nothing); what smoothing is
for, on a noisy ball; everything refused before a launch (the argument structs and the signatures are held to the header
in tests/test_abi_cpu.py).  No kernel is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import meshsmooth_ref as mr
from abi_probe import L  # noqa: F401  (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ESMALL = -1, -4
CASES = mr.hand_cases()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


def _adj(name):
    mesh = CASES[name]
    return mesh, mr.adjacency(mesh["triangles"], len(mesh["vertices"]))


def _rows(adj, key="neighbors", off="offsets"):
    o = adj[off]
    return [adj[key][o[v]:o[v + 1]].tolist() for v in range(len(o) - 1)]


# ---- the restatement on hand cases

def test_one_triangle_is_all_boundary():
    mesh, adj = _adj("one_triangle")
    assert adj["totals"] == [3, 6, 0, 3]
    assert _rows(adj) == [[1, 2], [0, 2], [0, 1]] and adj["boundary"].tolist() == [True] * 3
    assert _rows(adj, "incident", "tri_offsets") == [[0], [1], [2]]
    for k, dtype in (("offsets", np.int64), ("tri_offsets", np.int64), ("neighbors", np.int32), ("incident", np.int32), ("boundary", bool)):
        assert adj[k].dtype == dtype
    # everything is pinned by its boundary flag; free, a step with f = 1 puts each vertex at the mean of the other two
    assert np.array_equal(_bits(mr.smooth(mesh["vertices"], adj, [0.5, -0.53])), _bits(mesh["vertices"]))
    assert mr.smooth(mesh["vertices"], adj, [1.0], fix_boundary=False).tolist() == [[0.5, 0.5, 0], [0, 0.5, 0], [0.5, 0, 0]]
    assert mr.normals(mesh["vertices"], mesh["triangles"], adj).tolist() == [[0, 0, 1]] * 3


def test_tetrahedron_is_closed():
    mesh, adj = _adj("tetrahedron")
    assert adj["totals"] == [12, 12, 0, 0]
    assert _rows(adj) == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]] and not adj["boundary"].any()
    assert _rows(adj, "incident", "tri_offsets") == [[0, 3, 6], [1, 5, 9], [2, 7, 11], [4, 8, 10]]
    third = np.float32(1.0 / 3.0)
    got = mr.smooth(mesh["vertices"], adj, [1.0])           # the mean of the other three = -p / 3
    assert np.array_equal(_bits(got), _bits((-mesh["vertices"].astype(np.float64) / 3.0).astype(np.float32)))
    assert abs(got[0, 0]) == third
    n = mr.normals(mesh["vertices"], mesh["triangles"], adj)
    assert np.array_equal(_bits(n), _bits((mesh["vertices"] * np.float32(1.0 / np.sqrt(3.0))).astype(np.float32)))   # outwards
    assert np.array_equal(_bits(mr.normals(mesh["vertices"], mesh["triangles"], adj, mr.UNIFORM)), _bits(n))


def test_square_diagonal_is_interior_rim_is_boundary():
    mesh, adj = _adj("square")
    assert adj["totals"] == [6, 10, 0, 4]
    assert _rows(adj) == [[1, 2, 3], [0, 2], [0, 1, 3], [0, 2]] and adj["boundary"].all()
    # vertex 0 meets 2 twice (the diagonal) and 1, 3 once each: the rim makes it boundary
    assert _rows(adj, "incident", "tri_offsets") == [[0, 3], [1], [2, 4], [5]]


def test_three_triangles_on_one_edge():
    mesh, adj = _adj("three_on_an_edge")
    assert adj["totals"] == [9, 14, 0, 5]
    assert _rows(adj) == [[1, 2, 3, 4], [0, 2, 3, 4], [0, 1], [0, 1], [0, 1]]
    assert adj["boundary"].all()                            # through the outer edges; edge 0-1 has multiplicity 3, not 1
    only = mr.adjacency([[0, 1, 2], [0, 1, 3], [0, 1, 4], [0, 2, 3], [0, 3, 4], [0, 4, 2]], 5)
    assert not only["boundary"][0] and only["boundary"][1]  # vertex 0: multiplicities 3, 2, 2, 2; vertex 1: 1, 1, 1, 3


def test_bow_tie():
    mesh, adj = _adj("bow_tie")
    assert adj["totals"] == [6, 12, 0, 5]
    assert _rows(adj) == [[1, 2, 3, 4], [0, 2], [0, 1], [0, 4], [0, 3]] and adj["boundary"].all()


def test_isolated_vertex():
    mesh, adj = _adj("isolated_vertex")
    assert adj["totals"] == [6, 10, 0, 4]
    assert _rows(adj)[4] == [] and _rows(adj, "incident", "tri_offsets")[4] == [] and not adj["boundary"][4]
    got = mr.smooth(mesh["vertices"], adj, [0.5], fix_boundary=False)
    assert np.array_equal(_bits(got[4]), _bits(mesh["vertices"][4]))                 # d == 0: its own bits
    fb = np.full((5, 3), 7.0, dtype=np.float32)
    assert mr.normals(mesh["vertices"], mesh["triangles"], adj)[4].tolist() == [0, 0, 0]
    assert mr.normals(mesh["vertices"], mesh["triangles"], adj, fallback=fb)[4].tolist() == [7, 7, 7]
    assert mr.normals(mesh["vertices"], mesh["triangles"], adj, fallback=fb)[0].tolist() == [0, 0, 1]


def test_triangle_that_names_a_vertex_twice():
    mesh, adj = _adj("repeated_index")
    assert adj["totals"] == [6, 6, 0, 3]
    assert _rows(adj, "incident", "tri_offsets") == [[0, 1, 3], [2, 4], [5]]         # (0, 0, 1) lists vertex 0 twice
    assert _rows(adj) == [[1, 2], [0, 2], [0, 1]]
    # vertex 0 meets 1 three times (twice through (0, 0, 1)) and 2 once; the degenerate triangle adds no normal
    assert adj["boundary"].all()
    assert mr.normals(mesh["vertices"], mesh["triangles"], adj).tolist() == [[0, 0, 1]] * 3


def test_out_of_range_triangles_are_counted_and_take_part_in_nothing():
    mesh, adj = _adj("out_of_range")
    sq = mr.adjacency(CASES["square"]["triangles"], 4)
    assert adj["totals"] == [6, 10, 2, 4]
    for k in ("offsets", "neighbors", "boundary", "tri_offsets"):
        assert np.array_equal(adj[k], sq[k])
    assert adj["incident"].tolist() == [0, 9, 1, 2, 10, 11]                          # the entries keep their triangle's number


def test_nan_vertex_stays_and_is_not_counted():
    mesh, adj = _adj("nan_vertex")
    assert _rows(adj) == [[1, 2, 3], [0, 2, 4], [0, 1, 3, 4], [0, 2], [1, 2]]
    got = mr.smooth(mesh["vertices"], adj, [1.0], fix_boundary=False)
    assert np.array_equal(_bits(got[1]), _bits(mesh["vertices"][1]))                 # NaN and all
    assert got[0].tolist() == [0.5, 1.0, 0.0]                                       # the mean of 2 and 3 only
    assert got[4].tolist() == [1.0, 1.0, 0.0]                                       # vertex 2 alone
    n = mr.normals(mesh["vertices"], mesh["triangles"], adj)
    assert n[0].tolist() == [0, 0, 1] and n[3].tolist() == [0, 0, 1]                # triangle (0, 2, 3) alone
    assert n[1].tolist() == [0, 0, 0] and n[4].tolist() == [0, 0, 0]                # nothing finite to add


def test_pinned_vertex_and_empty_mesh():
    mesh, adj = _adj("tetrahedron")
    pinned = np.array([0, 1, 0, 0], dtype=np.uint8)
    got = mr.smooth(mesh["vertices"], adj, [1.0, 0.5], pinned=pinned)
    assert np.array_equal(_bits(got[1]), _bits(mesh["vertices"][1])) and not np.array_equal(got[0], mesh["vertices"][0])
    assert np.array_equal(_bits(mr.smooth(mesh["vertices"], adj, [])), _bits(mesh["vertices"]))
    empty = mr.adjacency(np.zeros((0, 3), dtype=np.int32), 0)
    assert empty["totals"] == [0, 0, 0, 0] and empty["offsets"].tolist() == [0] and empty["tri_offsets"].tolist() == [0]
    assert mr.adjacency([[0, 1, 2]], 0)["totals"] == [0, 0, 1, 0]
    assert mr.factors(2) == [0.5, -0.53, 0.5, -0.53] and mr.factors(3, 0.25, None) == [0.25] * 3


def test_fixed_against_free_boundary_on_a_grid_patch():
    mesh = mr.grid_patch(5)
    adj = mr.adjacency(mesh["triangles"], 25)
    assert adj["totals"] == [96, 112, 0, 16]
    rim = np.ones((5, 5), dtype=bool)
    rim[1:-1, 1:-1] = False
    assert np.array_equal(adj["boundary"].reshape(5, 5), rim)
    assert _rows(adj)[12] == [6, 7, 11, 13, 17, 18]                                 # an interior vertex of a split grid
    fixed = mr.smooth(mesh["vertices"], adj, mr.factors(3), fix_boundary=True)
    free = mr.smooth(mesh["vertices"], adj, mr.factors(3), fix_boundary=False)
    rim = rim.reshape(-1)
    assert np.array_equal(_bits(fixed[rim]), _bits(mesh["vertices"][rim]))
    assert (fixed[~rim] != mesh["vertices"][~rim]).any(axis=1).all()
    assert (free[rim] != mesh["vertices"][rim]).any(axis=1).all()                   # the rim of a free patch moves inwards
    both = mr.smooth(mesh["vertices"], adj, mr.factors(3), pinned=adj["boundary"], fix_boundary=False)
    assert np.array_equal(_bits(both), _bits(fixed))                                # a pin is a pin


# ---- the condition for exactness

def test_triangle_order_and_corner_rotation_change_nothing():
    """What the exact comparison of the GPU test rests on: the kernels meet the triangles in the order of arrival and sort
    every row, so their adjacency and their positions cannot depend on it -- and neither does the restatement's, under 20
    random permutations of the triangles and rotations of their corners.  The normals are summed in entry order, which a
    permutation changes, and a rotation changes p0: they move by no more than the 1e-6 of the GPU test.
    Measured worst over the noisy ball and a soup: 0.0 for both weightings (the fp64 differences vanish in the fp32 rounding)."""
    rng = np.random.default_rng(7)
    _, ball = mr.noisy_ball()
    worst = {mr.AREA: 0.0, mr.UNIFORM: 0.0}
    for mesh in (ball, mr.soup(257, 700, seed=2)):
        V = len(mesh["vertices"])
        adj = mr.adjacency(mesh["triangles"], V)
        pos = mr.smooth(mesh["vertices"], adj, mr.factors(3), fix_boundary=False)
        nrm = {w: mr.normals(mesh["vertices"], mesh["triangles"], adj, w) for w in worst}
        for _ in range(20):
            tri = mesh["triangles"][rng.permutation(len(mesh["triangles"]))]
            tri = np.take_along_axis(tri, (rng.integers(0, 3, len(tri))[:, None] + np.arange(3)) % 3, axis=1)
            other = mr.adjacency(tri, V)
            for k in ("offsets", "neighbors", "boundary", "tri_offsets"):
                assert np.array_equal(other[k], adj[k]), k
            assert other["totals"] == adj["totals"]
            assert np.array_equal(_bits(mr.smooth(mesh["vertices"], other, mr.factors(3), fix_boundary=False)), _bits(pos))
            for w in worst:
                moved = np.abs(mr.normals(mesh["vertices"], tri, other, w).astype(np.float64) - nrm[w])
                worst[w] = max(worst[w], float(moved.max()))
    print(f"normals under 20 permutations and rotations: worst {worst}")
    assert max(worst.values()) <= 1e-6


# ---- what it is for

def _radius(P):
    r = np.linalg.norm(P.astype(np.float64), axis=1)
    return float(r.mean()), float(np.sqrt(((r - r.mean()) ** 2).mean()))


def test_taubin_smooths_a_noisy_ball_without_shrinking_it():
    """The 33^3 marching-tetrahedra ball of radius 0.6 (5210 vertices) with radial noise of sigma 0.01.  Measured with
    the restatement: RMS deviation from the mean radius 0.00998 before, then 0.00739, 0.00606, 0.00532, 0.00486, 0.00454,
    0.00431, 0.00413, 0.00399, 0.00387, 0.00376 after each of 10 Taubin iterations (lam 0.5, mu -0.53); the mean radius
    goes from 0.599425 to 0.599614 (+1.9e-4) under Taubin and to 0.594092 (-5.3e-3) under 10 plain Laplacian steps of the
    same lam.  The thresholds: strictly falling; below half the start after 10; Taubin's drift under a tenth of the
    Laplacian's."""
    _, noisy = mr.noisy_ball()
    adj = mr.adjacency(noisy["triangles"], len(noisy["vertices"]))
    assert adj["totals"][2:] == [0, 0]                      # closed
    mean0, rms0 = _radius(noisy["vertices"])
    P, last = noisy["vertices"], rms0
    for _ in range(10):
        P = mr.smooth(P, adj, mr.factors(1))
        rms = _radius(P)[1]
        assert rms < last
        last = rms
    assert last < 0.5 * rms0
    assert np.array_equal(_bits(P), _bits(mr.smooth(noisy["vertices"], adj, mr.factors(10))))
    laplace = mr.smooth(noisy["vertices"], adj, mr.factors(10, 0.5, None))
    drift_t, drift_l = abs(_radius(P)[0] - mean0), abs(_radius(laplace)[0] - mean0)
    print(f"rms {rms0} -> {last}; mean radius drift: Taubin {drift_t}, Laplacian {drift_l}")
    assert drift_t < 0.1 * drift_l


def test_recomputed_normals_agree_with_the_extractor():
    """On the un-noised ball the normals from the triangles point the way the density gradient's do, at every vertex
    (measured smallest dot product: 0.9970 area-weighted, 0.9977 uniform)."""
    clean, _ = mr.noisy_ball()
    adj = mr.adjacency(clean["triangles"], len(clean["vertices"]))
    for w in (mr.AREA, mr.UNIFORM):
        n = mr.normals(clean["vertices"], clean["triangles"], adj, w)
        assert ((n.astype(np.float64) * clean["normals"]).sum(axis=1) > 0.0).all()
        assert np.abs(np.linalg.norm(n.astype(np.float64), axis=1) - 1.0).max() < 1e-6


# ---- the C ABI, without a GPU

def test_smoothing_symbols_bound_and_exported():
    """The stages are exported by the geometry package with the constants pinned (the C symbols under them: tests/test_abi_cpu.py)."""
    from nerf_fl_amd import _lib, geometry
    for name in ("mesh_adjacency", "smooth_mesh", "vertex_normals"):
        assert name in geometry.__all__ and callable(getattr(geometry, name))
    assert [_lib.SMOOTH_MAX_STEPS, _lib.ADJ_SHORT_ROW, _lib.NORMAL_WEIGHTINGS["area"],
            _lib.NORMAL_WEIGHTINGS["uniform"]] == [1024, 24, 0, 1]         # held to the header in test_abi_cpu.py


def test_unit_stands_on_the_geometry_headers_alone():
    with open(os.path.join(ROOT, "nerf_fl_amd", "csrc", "nfl_meshsmooth.hip")) as f:
        text = f.read()
    includes = set(re.findall(r'#include\s+"([^"]+)"', text))
    assert "nfl_geom.h" in includes
    assert not includes & {"nfl_mlp.h", "nfl_render_impl.h", "nfl_math.h", "nfl_plan.h"}
    for runtime in ("hipMemset", "hipMemcpy", "hipMalloc", "Synchronize"):
        assert runtime not in text
    with open(os.path.join(ROOT, "nerf_fl_amd", "csrc", "Makefile")) as f:
        make = f.read()
    assert "nfl_meshsmooth.o" in make.split("all:")[0]                      # in OBJS
    assert re.search(r"^nfl_surface\.o .*nfl_meshsmooth\.o.*: nfl_geom\.h nfl_geom_layout\.h$", make, flags=re.M)


def _tiles(n, tile=2048):
    entries, m = 0, -(-n // tile)
    while m > 1:
        entries, m = entries + m, -(-m // tile)
    return -(-entries * 8 // 16) * 16


def test_scratch_sizes(L):
    pad = lambda b: -(-b // 16) * 16
    fn, fs = L.nfl_mesh_adjacency_bytes, L.nfl_mesh_smooth_bytes
    big_t = (2 ** 31 - 1) // 3

    def restated(V, T):
        regions = [4 * V, 4 * V, 4 * V, 8 * V, 8 * V,                       # counts, cursors, degrees, two offsets
                   12 * T, 24 * T, 24 * T, V, _tiles(V)]                    # entries, neighbour rows, sorting area, flags, tile sums
        return sum(pad(b) for b in regions)

    sizes = (1, 2047, 2048, 2049, 2048 ** 2 + 1)
    grid = [(1, 0), (3, 1), (2048, 7), (2049, 5000), (70_000, 150_000), (5_000_000, 9_000_000), (2 ** 31 - 1, big_t)]
    for V, T in grid + [(V, T) for V in sizes for T in (0,) + sizes]:
        assert fn(V, T) == restated(V, T) and fn(V, T) % 16 == 0, (V, T)
    assert fn(0, 0) == 0 and fn(0, 5) == pad(60) + 2 * pad(120)
    for V, T in ((-1, 0), (0, -1), (-1, -1), (2 ** 31, 0), (0, big_t + 1), (2 ** 31, big_t + 1), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)):
        assert fn(V, T) == 0, (V, T)                                       # what the calls refuse
    for V in (1, 3, 4, 257, 70_000, 2 ** 31 - 1):
        assert fs(V) == pad(12 * V)
    assert fs(0) == 0 and fs(-1) == 0 and fs(2 ** 31) == 0 and fs(2 ** 63 - 1) == 0


def _call(L, fn, cls, base, **kw):
    a = cls(**dict(base, **kw))
    return fn(C.byref(a), None)


def test_adjacency_calls_validate_arguments(L):
    from nerf_fl_amd import _lib
    P = 64                                                                 # never dereferenced: every call below is refused
    big_t = (2 ** 31 - 1) // 3 + 1
    base = dict(d_triangles=P, n_vertices=10, n_triangles=4, d_scratch=P, scratch_bytes=L.nfl_mesh_adjacency_bytes(10, 4),
                d_totals=P, n_incident=12, n_neighbors=20, d_tri_offsets=P, d_incident=P, d_offsets=P, d_neighbors=P, d_boundary=P)
    for fn in (L.nfl_mesh_adjacency_count, L.nfl_mesh_adjacency_emit):
        call = lambda **kw: _call(L, fn, _lib.MeshAdjacencyArgs, base, **kw)
        assert fn(None, None) == EINVAL
        for bad in (dict(d_triangles=None), dict(d_scratch=None), dict(d_scratch=68), dict(n_vertices=-1), dict(n_triangles=-1),
                    dict(n_vertices=2 ** 31), dict(n_triangles=big_t), dict(d_scratch=68, scratch_bytes=0)):
            assert call(**bad) == EINVAL, bad
        assert call(scratch_bytes=base["scratch_bytes"] - 1) == ESMALL and call(scratch_bytes=0) == ESMALL
        assert call(n_vertices=0, d_scratch=None, scratch_bytes=0, d_totals=None, d_offsets=None) == 0      # nothing to do
    assert _call(L, L.nfl_mesh_adjacency_count, _lib.MeshAdjacencyArgs, base, d_totals=None) == EINVAL
    emit = lambda **kw: _call(L, L.nfl_mesh_adjacency_emit, _lib.MeshAdjacencyArgs, base, **kw)
    for bad in (dict(n_incident=-1), dict(n_neighbors=-1), dict(n_incident=13), dict(n_neighbors=25), dict(n_incident=0, n_neighbors=1),
                dict(d_tri_offsets=None), dict(d_offsets=None), dict(d_boundary=None), dict(d_incident=None), dict(d_neighbors=None)):
        assert emit(**bad) == EINVAL, bad


def test_smooth_and_normals_calls_validate_arguments(L):
    from nerf_fl_amd import _lib
    P = 64
    two = (C.c_double * 2)(0.5, -0.53)
    base = dict(d_vertices=P, d_offsets=P, d_neighbors=P, n_vertices=10, n_neighbors=30, d_boundary=P, d_pinned=None, fix_boundary=1,
                n_steps=2, factors=two, d_scratch=P, scratch_bytes=L.nfl_mesh_smooth_bytes(10), d_out_vertices=2 * P)
    call = lambda **kw: _call(L, L.nfl_mesh_smooth, _lib.MeshSmoothArgs, base, **kw)
    assert L.nfl_mesh_smooth(None, None) == EINVAL
    many = (C.c_double * 1025)(*([0.5] * 1025))
    for bad in (dict(d_vertices=None), dict(d_offsets=None), dict(d_neighbors=None), dict(d_out_vertices=None), dict(d_out_vertices=P),
                dict(d_boundary=None), dict(d_scratch=None), dict(d_scratch=68), dict(n_vertices=-1), dict(n_vertices=2 ** 31),
                dict(n_neighbors=-1), dict(n_steps=-1), dict(n_steps=1025, factors=many), dict(factors=None),
                dict(factors=(C.c_double * 2)(0.5, float("nan"))), dict(factors=(C.c_double * 2)(float("inf"), 0.5))):
        assert call(**bad) == EINVAL, bad
    assert call(scratch_bytes=base["scratch_bytes"] - 1) == ESMALL and call(scratch_bytes=0) == ESMALL
    assert call(n_vertices=0, d_vertices=None, d_offsets=None, d_scratch=None, scratch_bytes=0, d_out_vertices=None) == 0

    base = dict(d_vertices=P, d_triangles=P, n_vertices=10, n_triangles=4, d_tri_offsets=P, d_incident=P, n_incident=12,
                weighting=0, d_fallback_normals=None, d_out_normals=P)
    call = lambda **kw: _call(L, L.nfl_mesh_normals, _lib.MeshNormalsArgs, base, **kw)
    assert L.nfl_mesh_normals(None, None) == EINVAL
    for bad in (dict(d_vertices=None), dict(d_triangles=None), dict(d_tri_offsets=None), dict(d_incident=None), dict(d_out_normals=None),
                dict(n_vertices=-1), dict(n_triangles=-1), dict(n_vertices=2 ** 31), dict(n_triangles=(2 ** 31 - 1) // 3 + 1),
                dict(n_incident=-1), dict(weighting=2), dict(weighting=-1)):
        assert call(**bad) == EINVAL, bad
    assert call(n_vertices=0, d_vertices=None, d_tri_offsets=None, d_out_normals=None) == 0


def test_python_layer_refuses_before_a_launch():
    import torch
    from nerf_fl_amd import geometry
    mesh = {"vertices": torch.zeros(3, 3), "normals": torch.zeros(3, 3), "triangles": torch.zeros(1, 3, dtype=torch.int32)}
    for call in (lambda: geometry.mesh_adjacency(mesh), lambda: geometry.smooth_mesh(mesh), lambda: geometry.vertex_normals(mesh),
                 lambda: geometry.smooth_mesh(mesh, 3, lam=1.0, mu=None, boundary="free", normals=None)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
    for iterations in (-1, 513, 2.0, None, "ten", True):
        with pytest.raises(ValueError, match="iterations"):
            geometry.smooth_mesh(mesh, iterations)
    for lam in (0.0, -0.5, 1.5, float("nan"), float("inf"), None, "wide"):
        with pytest.raises(ValueError, match="lam"):
            geometry.smooth_mesh(mesh, lam=lam)
    for mu in (0.0, 0.53, float("nan"), float("-inf"), "low"):
        with pytest.raises(ValueError, match="mu"):
            geometry.smooth_mesh(mesh, mu=mu)
    for boundary in ("pinned", None, 1):
        with pytest.raises(ValueError, match="boundary"):
            geometry.smooth_mesh(mesh, boundary=boundary)
    for normals in ("angle", 1):
        with pytest.raises(ValueError, match="normals"):
            geometry.smooth_mesh(mesh, normals=normals)
    for weighting in ("angle", None, 0):
        with pytest.raises(ValueError, match="weighting"):
            geometry.vertex_normals(mesh, weighting=weighting)
    with pytest.raises(ValueError):
        geometry.smooth_mesh({"vertices": torch.zeros(3, 3)})
    # extract_mesh refuses the same before it evaluates anything
    for kw in (dict(smooth=-1), dict(smooth=1.5), dict(smooth=3, smooth_kwargs=dict(lam=2.0)), dict(smooth=3, smooth_kwargs=dict(mu=1.0)),
               dict(smooth=3, smooth_kwargs=dict(boundary="loose")), dict(smooth=3, smooth_kwargs=dict(normals="angle")),
               dict(smooth=3, smooth_kwargs=dict(pinned=None))):
        with pytest.raises(ValueError):
            geometry.extract_mesh({}, {}, (-1, -1, -1), (1, 1, 1), (8, 8, 8), 0.0, **kw)
