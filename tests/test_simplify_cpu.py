"""CPU-side checks of the mesh simplification (nerf_fl_amd.geometry.simplify_mesh, csrc/nfl_simplify.hip): the numpy
restatement (tests/simplify_ref.py), which the GPU tests hold the kernels to, on hand-written cases with the expected values
written out, its invariants on random soups, the quadric placement on a cube, and the condition under which the GPU test
may compare quadric positions to within 2 ulps; everything refused before a launch (the argument struct and the
signatures are held to the header in tests/test_abi_cpu.py).  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest

import simplify_ref as sr
from abi_probe import L, probe  # noqa: F401  (L is a fixture)

EINVAL, ESMALL = -1, -4


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


# ---- the restatement on hand cases

CASES = sr.hand_cases()


def _run(name, placement="mean"):
    mesh, cell, origin = CASES[name]
    return sr.simplify(mesh, cell, origin, placement)


def test_two_vertices_in_one_cell():
    out, cluster, totals = _run("two_in_one_cell")
    assert cluster.tolist() == [0, 0, 1] and totals == [2, 0, 0, 0]
    assert out["triangles"].shape == (0, 3) and out["triangles"].dtype == np.int32
    assert out["vertices"].tolist() == [[0.5, 0.375, 0.25], [1.5, 0.5, 0.5]]
    r = float(np.float32(np.sqrt(0.5)))
    assert out["normals"].tolist() == [[r, r, 0.0], [0.0, 0.0, 1.0]]
    assert out["colors"].tolist() == [[0.5, 0.5, 0.5], [0.25, 0.25, 0.25]]
    for v in out.values():
        assert v.dtype in (np.float32, np.int32)


def test_vertex_on_a_cell_face_and_on_origin():
    mesh, cell, origin = CASES["on_a_face_and_on_origin"]
    valid, ijk, _ = sr.cells(mesh["vertices"], cell, origin)
    assert valid.all() and ijk.tolist() == [[0, 0, 0], [1, 0, -1], [-1, 0, 0]]      # a face belongs to the cell above it
    out, cluster, totals = sr.simplify(mesh, cell, origin)
    assert cluster.tolist() == [0, 1, 2] and totals == [3, 1, 0, 0] and out["triangles"].tolist() == [[0, 1, 2]]
    assert np.array_equal(_bits(out["vertices"]), _bits(mesh["vertices"]))          # clusters of one: their own bits


def test_negative_coordinates():
    mesh, cell, origin = CASES["negative"]
    _, ijk, _ = sr.cells(mesh["vertices"], cell, origin)
    assert ijk.tolist() == [[-1, -1, -2], [-1, -1, -2], [0, 0, 0]]
    out, cluster, totals = sr.simplify(mesh, cell, origin)
    assert cluster.tolist() == [0, 0, 1] and totals == [2, 0, 0, 0]
    assert out["vertices"].tolist() == [[-0.375, -0.875, -1.375], [0.5, 0.5, 0.5]]
    assert int(sr.keys(np.array([[-1, -1, -2]]))[0]) == (2 ** 20 - 1) | (2 ** 20 - 1) << 21 | (2 ** 20 - 2) << 42


def test_cell_limits():
    mesh, cell, origin = CASES["limits"]
    valid, ijk, _ = sr.cells(mesh["vertices"], cell, origin)
    assert valid.tolist() == [True, True, False, False]
    assert ijk[:2, 0].tolist() == [-2 ** 20, 2 ** 20 - 1]
    assert int(sr.keys(ijk[:1])[0]) == 0 | (2 ** 20) << 21 | (2 ** 20) << 42
    assert int(sr.keys(np.full((1, 3), 2 ** 20 - 1))[0]) == 2 ** 63 - 1              # the largest key: never all 64 bits
    out, cluster, totals = sr.simplify(mesh, cell, origin)
    assert cluster.tolist() == [0, 1, -1, -1] and totals == [2, 0, 0, 2] and len(out["vertices"]) == 2


def test_nan_vertex():
    out, cluster, totals = _run("nan_vertex")
    assert cluster.tolist() == [0, -1, 1, 2] and totals == [3, 1, 0, 1]
    assert out["triangles"].tolist() == [[0, 1, 2]]                                 # the triangle on the NaN vertex is gone
    assert out["vertices"].tolist() == [[0.5, 0.5, 0.5], [2.5, 0.5, 0.5], [3.5, 0.5, 0.5]]


def test_square_collapses_to_nothing():
    for placement in ("mean", "quadric"):
        out, cluster, totals = _run("square_to_nothing", placement)
        assert cluster.tolist() == [0, 0, 0, 0] and totals == [1, 0, 0, 0]
        assert out["triangles"].shape == (0, 3)
        assert out["vertices"].tolist() == [[0.5, 0.5, 0.5]] and out["normals"].tolist() == [[0.0, 0.0, 1.0]]


def test_rotations_are_duplicates_and_mirror_images_are_not():
    out, cluster, totals = _run("rotation_and_mirror")
    assert cluster.tolist() == [0, 1, 2, 0, 1, 2] and totals == [3, 2, 0, 0]
    # (4, 5, 3) -> (1, 2, 0) and (5, 1, 3) -> (2, 1, 0): a rotation of the first, a rotation of the third
    assert out["triangles"].tolist() == [[0, 1, 2], [0, 2, 1]]
    assert out["vertices"][:, 0].tolist() == [0.375, 1.375, 2.375]


def test_out_of_range_triangles_are_counted():
    mesh = dict(CASES["nan_vertex"][0])
    mesh["triangles"] = np.array([[0, 2, 3], [0, 2, 4], [-1, 0, 2], [2, 3, 0]], dtype=np.int32)
    out, _, totals = sr.simplify(mesh, 1.0)
    assert totals == [3, 1, 2, 1] and out["triangles"].tolist() == [[0, 1, 2]]     # the last is a rotation of the first


def test_empty_mesh():
    out, cluster, totals = sr.simplify(sr._mesh(np.zeros((0, 3)), np.zeros((0, 3))), 1.0)
    assert cluster.shape == (0,) and totals == [0, 0, 0, 0]
    assert out["vertices"].shape == (0, 3) and out["triangles"].shape == (0, 3)


# ---- invariants on random soups

@pytest.mark.parametrize("V,T,cell", [(300, 900, 0.5), (300, 900, 2.0), (5000, 12000, 0.3), (5000, 12000, 100.0), (65, 200, 1.0)])
def test_invariants_on_random_soups(V, T, cell):
    mesh = sr.soup(V, T, seed=V + T)
    out, cluster, totals = sr.simplify(mesh, cell)
    n_out, tri = totals[0], out["triangles"].astype(np.int64)
    assert totals[1] == len(tri) and totals[2] == 0 and totals[3] == 3
    assert len(out["vertices"]) == len(out["normals"]) == len(out["colors"]) == n_out
    assert ((tri >= 0) & (tri < n_out)).all()
    assert (tri[:, 0] != tri[:, 1]).all() and (tri[:, 1] != tri[:, 2]).all() and (tri[:, 0] != tri[:, 2]).all()
    start = tri.argmin(axis=1)
    canon = np.take_along_axis(tri, (start[:, None] + np.arange(3)) % 3, axis=1)
    assert len(np.unique(canon, axis=0)) == len(tri)                                 # no two are rotations of each other
    used = cluster[cluster >= 0]
    assert np.array_equal(np.unique(used), np.arange(n_out))                         # onto [0, V')
    first = np.full(n_out, V)
    np.minimum.at(first, used, np.flatnonzero(cluster >= 0))
    assert (np.diff(first) > 0).all()                                               # ids ascend with the first member
    # every input triangle that should survive is there, as a rotation
    m = cluster[mesh["triangles"]].astype(np.int64)
    ok = (m >= 0).all(axis=1) & (m[:, 0] != m[:, 1]) & (m[:, 1] != m[:, 2]) & (m[:, 0] != m[:, 2])
    want = {tuple(np.roll(r, -int(r.argmin()))) for r in m[ok]}
    assert want == {tuple(r) for r in canon}
    # a slow, dict-based second opinion on the ids
    seen, ids = {}, []
    valid, ijk, _ = sr.cells(mesh["vertices"], cell)
    for v in range(V):
        ids.append(seen.setdefault(tuple(ijk[v]), len(seen)) if valid[v] else -1)
    assert ids == cluster.tolist()
    # means lie in their cells; a cluster of one keeps its bits
    n = np.bincount(used, minlength=n_out)
    lone = np.flatnonzero(n[cluster.clip(0)] == 1)
    lone = lone[cluster[lone] >= 0]
    for k in ("vertices", "normals", "colors"):
        assert np.array_equal(_bits(out[k][cluster[lone]]), _bits(mesh[k][lone])), k


# ---- the quadric placement

CUBE_CELL, CUBE_ORIGIN = 0.8, (-1.2, -1.2, -1.2)             # cells [-1.2, -0.4), [-0.4, 0.4), [0.4, 1.2) per axis


def _cube_cluster(cluster, mesh, point):
    return int(cluster[np.flatnonzero((mesh["vertices"] == np.float32(point)).all(axis=1))[0]])


def test_quadric_keeps_the_corner_of_a_cube():
    mesh = sr.cube_surface(6)
    assert mesh["vertices"].shape == (218, 3) and mesh["triangles"].shape == (432, 3)
    mean, cluster, totals = sr.simplify(mesh, CUBE_CELL, CUBE_ORIGIN, "mean")
    quad, cluster_q, totals_q = sr.simplify(mesh, CUBE_CELL, CUBE_ORIGIN, "quadric")
    assert totals == totals_q == [26, 48, 0, 0] and np.array_equal(cluster, cluster_q)
    assert np.array_equal(mean["triangles"], quad["triangles"]) and np.array_equal(_bits(mean["normals"]), _bits(quad["normals"]))
    for corner in ((1, 1, 1), (-1, 1, -1), (-1, -1, -1)):
        c = _cube_cluster(cluster, mesh, corner)
        assert (cluster == c).sum() == 7                                             # a cluster of its own, not of one
        d_mean = np.abs(mean["vertices"][c].astype(np.float64) - corner).max()
        d_quad = np.abs(quad["vertices"][c].astype(np.float64) - corner).max()
        assert d_mean > 0.1 and d_quad < 1e-3 and d_quad < d_mean                  # three planes meet in the corner
    c = _cube_cluster(cluster, mesh, (1, 0, 0))                                      # the middle of the face x = 1
    assert (cluster == c).sum() == 9
    for out in (mean, quad):
        assert abs(float(out["vertices"][c, 0]) - 1.0) <= 2.0 ** -23
        assert np.abs(out["vertices"][c, 1:]).max() <= 2.0 ** -23
    # an edge: the quadric vertex stays on the edge's line, the mean falls inside the cube
    c = _cube_cluster(cluster, mesh, (1, 1, 0))
    assert np.abs(quad["vertices"][c, :2] - 1.0).max() < 1e-3 and np.abs(mean["vertices"][c, :2] - 1.0).max() > 0.05
    # nothing leaves its cell
    for out in (mean, quad):
        _, ijk, _ = sr.cells(out["vertices"], CUBE_CELL, CUBE_ORIGIN)
        lead = np.array([np.flatnonzero(cluster == k)[0] for k in range(26)])
        _, ijk_in, _ = sr.cells(mesh["vertices"][lead], CUBE_CELL, CUBE_ORIGIN)
        centre = np.array(CUBE_ORIGIN) + (ijk_in + 0.5) * CUBE_CELL
        assert (np.abs(out["vertices"] - centre) <= CUBE_CELL / 2 * (1 + 1e-6)).all()


def _ulps(a, b):
    """|a - b| in units of the fp32 spacing at max(|a|, |b|)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def ball_mesh():
    import geometry_ref as gr
    lat, lo, hi, sp = sr.ball_lattice(33)
    mesh = gr.extract(lat, 0.0, lo, sp)
    mesh["colors"] = (np.abs(mesh["normals"]) * np.float32(0.5) + np.float32(0.25)).astype(np.float32)
    return mesh, lo, float(sp[0])


def test_quadric_does_not_depend_on_the_order_of_the_sums():
    """What the 2-ulp tolerance of the GPU test rests on: the fp64 sums taken in 20 random orders of the triangles move
    no quadric position by more than one fp32 ulp of the coordinate (the regularisation bounds the condition number by
    about 1 / LAMBDA, so 1e-16 relative in the sums stays far below 6e-8; a final rounding near a tie can still flip)."""
    rng = np.random.default_rng(5)
    ball, lo, sp = ball_mesh()
    worst = 0.0
    for mesh, cell, origin in ((sr.cube_surface(6), CUBE_CELL, CUBE_ORIGIN), (ball, 2 * sp, lo), (ball, 3.5 * sp, lo)):
        base = sr.simplify(mesh, cell, origin, "quadric")[0]["vertices"]
        for _ in range(20):
            got = sr.simplify(mesh, cell, origin, "quadric", order=rng.permutation(len(mesh["triangles"])))[0]["vertices"]
            worst = max(worst, float(_ulps(got, base).max()))
    print(f"quadric positions under 20 permutations of the triangles: worst {worst} ulp")
    assert worst <= 1.0


def test_ball_mesh_shrinks():
    ball, lo, sp = ball_mesh()
    V, T = len(ball["vertices"]), len(ball["triangles"])
    last = (V, T)
    for k in (2.0, 3.5):
        out, cluster, totals = sr.simplify(ball, k * sp, lo)
        assert totals[2:] == [0, 0] and 0 < totals[0] < last[0] and 0 < totals[1] < last[1]
        last = tuple(totals[:2])
        # still a closed surface of the ball: every vertex near the sphere, Euler characteristic 2 when manifold
        r = np.linalg.norm(out["vertices"].astype(np.float64), axis=1)
        assert np.abs(r - 0.6).max() < k * sp


# ---- the C ABI, without a GPU

def test_simplify_symbols_bound_and_exported():
    """The stage is exported by the geometry package (the C symbols under it: tests/test_abi_cpu.py)."""
    from nerf_fl_amd import geometry
    assert "simplify_mesh" in geometry.__all__ and callable(geometry.simplify_mesh)


def test_the_restatement_regularises_as_the_header_says():
    from nerf_fl_amd import _lib
    assert probe()["constants"]["NFL_SIMPLIFY_LAMBDA"] == _lib.SIMPLIFY_LAMBDA == sr.LAMBDA == 1e-3


def _tiles(n, tile=2048):
    entries, m = 0, -(-n // tile)
    while m > 1:
        entries, m = entries + m, -(-m // tile)
    return -(-entries * 8 // 16) * 16


def _cap(n):
    c = 2
    while c < 2 * n:
        c *= 2
    return c if n else 0


def test_simplify_scratch_size(L):
    pad = lambda b: -(-b // 16) * 16
    fn = L.nfl_mesh_simplify_bytes
    assert fn(-1, 0) == 0 and fn(0, -1) == 0 and fn(2 ** 31, 0) == 0 and fn(0, (2 ** 31 - 1) // 3 + 1) == 0
    assert fn(0, 0) == 0 and fn(2 ** 31 - 1, (2 ** 31 - 1) // 3) > 0
    assert [_cap(n) for n in (0, 1, 2, 3, 1024, 1025)] == [0, 2, 4, 8, 2048, 4096]
    for V, T in ((1, 0), (3, 1), (2048, 7), (2049, 5000), (70_000, 150_000), (5_000_000, 9_000_000)):
        exp = (pad(8 * _cap(V)) + pad(4 * _cap(V)) + 2 * pad(4 * V) + pad(8 * V)
               + pad(12 * T) + 2 * pad(4 * _cap(T)) + 2 * pad(4 * T) + pad(8 * T) + max(_tiles(V), _tiles(T))
               + pad(4 * V) + 2 * pad(72 * V))
        assert fn(V, T) == exp, (V, T)


def test_simplify_scratch_layout_over_the_mesh_grid(L):
    """The 15 regions restated here, over the grid of (V, T) test_mesh_cpu.py holds the mesh formulas to and over the
    sizes at which a scan gains a level (2048, 2048^2) or a hash table doubles."""
    pad = lambda b: -(-b // 16) * 16
    fn = L.nfl_mesh_simplify_bytes

    def restated(V, T):
        regions = [8 * _cap(V), 4 * _cap(V), 4 * V, 4 * V, 8 * V,                  # vertex table, slots, flags, ranks
                   12 * T, 4 * _cap(T), 4 * _cap(T), 4 * T, 4 * T, 8 * T,          # triples, triangle table, slots, flags, offsets
                   max(_tiles(V), _tiles(T)), 4 * V, 72 * V, 72 * V]               # tile sums, counts, fixed-point sums, quadrics
        return sum(pad(b) for b in regions)

    sizes = (1, 2047, 2048, 2049, 2048 ** 2 + 1)
    grid = [(1, 0), (3, 1), (2048, 7), (2049, 5000), (5_000_000, 9_000_000)] + [(V, T) for V in sizes for T in (0,) + sizes]
    for V, T in grid:
        assert fn(V, T) == restated(V, T), (V, T)
        assert fn(V, T) % 16 == 0
    big_t = (2 ** 31 - 1) // 3
    assert fn(2 ** 31 - 1, big_t) == restated(2 ** 31 - 1, big_t)
    for V, T in ((-1, 0), (0, -1), (-1, -1), (2 ** 31, 0), (0, big_t + 1), (2 ** 31, big_t + 1), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)):
        assert fn(V, T) == 0, (V, T)                                           # what nm_sizes_ok refuses


def test_simplify_calls_validate_arguments(L):
    from nerf_fl_amd import _lib
    P = 64                                                                 # never dereferenced: every call below is refused
    big_t = (2 ** 31 - 1) // 3 + 1

    def call(fn, **kw):
        a = _lib.MeshSimplifyArgs(d_vertices=P, d_normals=P, d_colors=None, d_triangles=P, n_vertices=10, n_triangles=4,
                                  cell=0.5, placement=0, d_scratch=P, scratch_bytes=L.nfl_mesh_simplify_bytes(10, 4),
                                  d_totals=P, d_cluster=P, n_out_vertices=5, n_out_triangles=2, d_out_vertices=P,
                                  d_out_normals=P, d_out_colors=None, d_out_triangles=P)
        for k, v in kw.items():
            if k == "origin":
                for i in range(3):
                    a.origin[i] = v[i]
            else:
                setattr(a, k, v)
        return fn(C.byref(a), None)

    for fn in (L.nfl_mesh_simplify_count, L.nfl_mesh_simplify_emit):
        assert fn(None, None) == EINVAL
        for bad in (dict(d_vertices=None), dict(d_triangles=None), dict(d_cluster=None), dict(d_scratch=None), dict(d_scratch=68),
                    dict(n_vertices=-1), dict(n_triangles=-1), dict(n_vertices=2 ** 31), dict(n_triangles=big_t),
                    dict(cell=0.0), dict(cell=-1.0), dict(cell=float("nan")), dict(cell=float("inf")),
                    dict(origin=(0.0, float("nan"), 0.0)), dict(origin=(float("inf"), 0.0, 0.0)),
                    dict(placement=2), dict(placement=-1)):
            assert call(fn, **bad) == EINVAL, bad
        assert call(fn, scratch_bytes=L.nfl_mesh_simplify_bytes(10, 4) - 1) == ESMALL and call(fn, scratch_bytes=0) == ESMALL
        assert call(fn, n_vertices=0, d_vertices=None, d_cluster=None, d_scratch=None, scratch_bytes=0) == 0     # nothing to do
    assert call(L.nfl_mesh_simplify_count, d_totals=None) == EINVAL
    emit = L.nfl_mesh_simplify_emit
    for bad in (dict(n_out_vertices=-1), dict(n_out_triangles=-1), dict(n_out_vertices=11), dict(n_out_triangles=5),
                dict(d_normals=None), dict(d_out_vertices=None), dict(d_out_normals=None), dict(d_out_triangles=None),
                dict(d_colors=P, d_out_colors=None)):
        assert call(emit, **bad) == EINVAL, bad
    assert call(emit, n_out_vertices=0, n_out_triangles=0, d_out_vertices=None, d_out_normals=None,
                d_out_triangles=None) == 0                                 # totals of 0: no launch


def test_simplify_mesh_refuses_before_a_launch():
    import torch
    from nerf_fl_amd import geometry
    mesh = {"vertices": torch.zeros(3, 3), "normals": torch.zeros(3, 3), "triangles": torch.zeros(1, 3, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.simplify_mesh(mesh, 0.5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.simplify_mesh(mesh, 0.5, origin=(1, 2, 3), placement="quadric", return_map=True)
    for cell in (0, -1.0, float("nan"), float("inf"), None, "wide"):
        with pytest.raises(ValueError, match="cell"):
            geometry.simplify_mesh(mesh, cell)
    for placement in ("median", None, 1):
        with pytest.raises(ValueError, match="placement"):
            geometry.simplify_mesh(mesh, 0.5, placement=placement)
    for origin in ((0, 0), (0, 0, 0, 0), (0, float("nan"), 0), (0, 0, float("inf")), 1.0, ("a", "b", "c")):
        with pytest.raises(ValueError, match="origin"):
            geometry.simplify_mesh(mesh, 0.5, origin=origin)
    with pytest.raises(ValueError):
        geometry.simplify_mesh({"vertices": torch.zeros(3, 3)}, 0.5)
    # extract_mesh refuses the same before it evaluates anything
    for kw in (dict(simplify=0.0), dict(simplify=0.1, placement="median")):
        with pytest.raises(ValueError):
            geometry.extract_mesh({}, {}, (-1, -1, -1), (1, 1, 1), (8, 8, 8), 0.0, **kw)
