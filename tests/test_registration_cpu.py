"""CPU-side checks of the registration (nerf_fl_amd.registration, csrc/nfl_register.hip): the four C entry points are in the
tables test_abi_cpu.py holds to the header, add no struct, and refuse bad arguments before any launch; the module stands beside
meshdist.py; the numpy restatement (tests/registration_ref.py), which the GPU tests hold the kernels to bit for bit, is
checked against numpy's own SVD and least squares, and on the claims DESIGN.md section 34 makes about the two modes on a
height field.  No kernel is launched.

Tolerances that are MEASURED on the restatement (this machine's numpy, fp64) and not derived, with their measurements:
  plane solve against numpy.linalg.lstsq on the un-reduced rows, 20 seeds of 200 pairs in the unit box: worst difference of an
      unknown 6.2e-17 (the unknowns are 4e-3 .. 2e-2, the normal matrix has condition 8); asserted 100 x that;
  point solve against the SVD solution (Umeyama), 20 seeds of 300 noisy pairs: worst difference of one of the 13 doubles
      1.4e-15; asserted 100 x that;
  plane mode with scale from 20 degrees, translation (0.05, -0.04, 0.03), scale 1.08 on height_field(13), 602 samples: rms per
      iteration 1.1e-1, 1.1e-2, 6.5e-4, 2.4e-6, 8.5e-9 and then the floor the fp32 coordinates set; recovered to 5.8e-7
      degrees, 7.3e-9 in the translation, 2.2e-9 in the scale; asserted 10 x those (registration_ref.RECOVERED);
  the whole height_field(13) displaced by 8 degrees, the same translation and scale 1.04, registered in 8 iterations of plane
      mode with scale: Chamfer distance to itself 5.6e-2 before and 5.9e-9 after; asserted 10 x that
      (registration_ref.REGISTERED_CHAMFER);
  point mode from 8 degrees: rms 4.5e-2, 1.0e-2, 9.8e-3, ... 5.3e-3 after 40 iterations, still 4.39 degrees off."""
import os
import re

import numpy as np
import pytest

import meshdist_ref as dref
import registration_ref as rref
from abi_probe import HEADER, L, declared, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL, ESMALL = -1, -4
INF, NAN = np.inf, np.nan
RECOVERED, PLANE_VS_LSTSQ, POINT_VS_SVD = rref.RECOVERED, rref.PLANE_VS_LSTSQ, rref.POINT_VS_SVD
NAMES = ("nfl_register_bytes", "nfl_register_apply", "nfl_register_moments", "nfl_register_solve")


# ---- sources and validation ------------------------------------------------------------------------------------------------

def test_the_tables_hold_the_four_entry_points_and_no_new_struct(L):
    symbols = {s[0] for s in _lib.SYMBOLS}
    for name in NAMES:
        assert name in symbols and name in declared()["functions"], name
        getattr(L, name)                                                   # exported by the built library
    assert len(declared()["structs"]) == 42 == len(_lib.STRUCTS)           # plain arguments: the header gains no struct
    constants = probe()["constants"]
    for name, value in (("NFL_REGISTER_POINT", rref.POINT), ("NFL_REGISTER_PLANE", rref.PLANE), ("NFL_REGISTER_OK", rref.OK),
                        ("NFL_REGISTER_FEW", rref.FEW), ("NFL_REGISTER_SINGULAR", rref.SINGULAR), ("NFL_REGISTER_TRANSFORM", 13),
                        ("NFL_REGISTER_HISTORY", 4), ("NFL_REGISTER_COUNT", rref.COUNT), ("NFL_REGISTER_SUM_DD", rref.SUM_DD),
                        ("NFL_REGISTER_SUM_P", rref.SUM_P), ("NFL_REGISTER_SUM_Q", rref.SUM_Q), ("NFL_REGISTER_SUM_PP", rref.SUM_PP),
                        ("NFL_REGISTER_SUM_QQ", rref.SUM_QQ), ("NFL_REGISTER_SUM_PQ", rref.SUM_PQ), ("NFL_REGISTER_ATA", rref.ATA),
                        ("NFL_REGISTER_ATB", rref.ATB), ("NFL_REGISTER_SUM_RR", rref.SUM_RR), ("NFL_REGISTER_COLUMNS", rref.COLUMNS)):
        assert _lib.CONSTANTS[name] == constants[name] == value, name
    assert "#define NFL_ABI_VERSION 10\n" in open(HEADER).read()


def test_the_unit_is_built_and_has_its_section():
    assert "---- registration:" in open(HEADER).read()
    make = open(os.path.join(ROOT, "nerf_fl_amd", "csrc", "Makefile")).read()
    assert "nfl_register.o" in make.split("all:")[0]                       # in OBJS
    assert re.search(r"^nfl_register\.o:.*nfl_geom\.h.*nfl_geom_layout\.h", make, flags=re.M)


def test_the_module_stands_beside_meshdist():
    pkg = os.path.join(ROOT, "nerf_fl_amd")
    source = open(os.path.join(pkg, "registration.py")).read()
    assert "_lib.check(" not in source and "C.byref(" not in source and "import ctypes" not in source and "rendering." not in source
    for helper in ("_call", "_positive", "_ptr", "_scratch", "_is", "_on_device"):
        assert re.search(rf"^from \.geometry\._call import .*\b{helper}\b", source, flags=re.M), helper
    assert ".tolist()" not in source and ".item()" not in source and source.count(".cpu()") == 4      # the reads its docstrings name
    # the target goes through meshdist's one front, the box through its one reduction; the fp32 rule of a limit is _positive's
    assert re.search(r"^from \.meshdist import .*\b_finite_box\b.*\b_mesh_or_grid\b", source, flags=re.M)
    assert "isinstance(target" not in source and "torch.where(" not in source and "np.float32(" not in source
    assert sorted(n for n in os.listdir(os.path.join(pkg, "geometry")) if n.endswith(".py")) == [
        "__init__.py", "_call.py", "files.py", "images.py", "lattice.py", "mesh.py", "occupancy.py"]
    from nerf_fl_amd import fusion, geometry, meshdist, registration
    assert registration.__all__ == ["fit_transform", "transform_points", "transform_mesh", "register_mesh", "registered_distance"]
    assert meshdist.__all__ == ["triangle_grid", "closest_on_mesh", "sample_surface", "mesh_distance", "read_ply"]
    assert len(geometry.__all__) == 24 and len(fusion.__all__) == 6
    assert not set(registration.__all__) & (set(geometry.__all__) | set(meshdist.__all__) | set(fusion.__all__))
    for bad in (dict(mode="line"), dict(points="faces"), dict(iterations=0), dict(iterations=2.5), dict(min_pairs=0),
                dict(max_distance=0.0), dict(max_distance=[1.0, 2.0], iterations=3), dict(max_distance=NAN)):
        with pytest.raises(ValueError):                                    # refused before any tensor is looked at
            registration.register_mesh(None, None, **bad)


def test_sizes(L):
    assert L.nfl_register_bytes(0) == 0 and L.nfl_register_bytes(1) == 448 == L.nfl_register_bytes(256)      # 440 padded to 16
    assert L.nfl_register_bytes(257) == 880 and L.nfl_register_bytes(70001) == 274 * 440
    assert L.nfl_register_bytes(2 ** 31 - 1) == 1024 * 440 and L.nfl_register_bytes(2 ** 31) == 0 == L.nfl_register_bytes(-1)


def _apply_args(**over):
    a = dict(d_in=0x1000, d_out=0x2000, n=100, d_transform=0x3000, vectors=0)
    a.update(over)
    return [a[k] for k in ("d_in", "d_out", "n", "d_transform", "vectors")] + [None]


def _moments_args(**over):
    a = dict(d_points=0x1000, d_closest=0x2000, d_triangle=0x3000, d_distance=0x4000, d_vertices=0x5000, d_triangles=0x6000,
             n=1000, n_vertices=30, n_triangles=10, mode=1, max_distance=INF, cx=0.0, cy=0.5, cz=-0.5, d_scratch=0x7000,
             scratch_bytes=4 * 440, d_row=0x8000)
    a.update(over)
    return list(a.values()) + [None]


def _solve_args(**over):
    a = dict(d_row=0x1000, mode=1, with_scale=1, min_pairs=6, cx=0.0, cy=0.5, cz=-0.5, d_transform=0x2000, d_history=0x3000,
             iteration=0)
    a.update(over)
    return list(a.values()) + [None]


def test_apply_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    for over in (dict(d_in=None), dict(d_out=None), dict(d_in=0x1002), dict(d_out=0x2001), dict(n=-1), dict(n=1 << 31),
                 dict(d_transform=None), dict(d_transform=0x3004), dict(vectors=2), dict(vectors=-1)):
        assert L.nfl_register_apply(*_apply_args(**over)) == EINVAL, over
    assert L.nfl_register_apply(*_apply_args(n=0, d_in=None, d_out=None)) == 0                 # no row: NFL_OK without a launch
    assert L.nfl_register_apply(*_apply_args(n=0, d_transform=None)) == EINVAL


def test_moments_refuses_before_any_launch(L):
    for over in (dict(d_points=None), dict(d_closest=None), dict(d_points=0x1002), dict(d_closest=0x2001), dict(d_triangle=None),
                 dict(d_distance=None), dict(d_triangle=0x3002), dict(d_distance=0x4001), dict(d_vertices=None),
                 dict(d_triangles=None), dict(d_vertices=0x5002), dict(d_triangles=0x6001), dict(n=-1), dict(n=1 << 31),
                 dict(n_vertices=-1), dict(n_triangles=-1), dict(n_vertices=1 << 31), dict(n_triangles=(2 ** 31 - 1) // 3 + 1),
                 dict(mode=2), dict(mode=-1), dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=NAN),
                 dict(cx=NAN), dict(cy=INF), dict(cz=-INF), dict(d_scratch=None), dict(d_scratch=0x7004), dict(d_row=None),
                 dict(d_row=0x8004)):
        assert L.nfl_register_moments(*_moments_args(**over)) == EINVAL, over
    assert L.nfl_register_moments(*_moments_args(scratch_bytes=4 * 440 - 1)) == ESMALL
    # point mode does without the distance and the triangle, and then without the mesh; what IS given is still checked
    for over in (dict(mode=0, d_triangle=0x3002), dict(mode=0, d_distance=0x4002), dict(mode=0, d_vertices=None),
                 dict(mode=0, d_triangle=None, d_distance=None, d_vertices=None, d_triangles=None, d_scratch=None),
                 dict(mode=0, d_triangle=None, d_distance=None, d_vertices=None, d_triangles=None, d_row=0x8004)):
        assert L.nfl_register_moments(*_moments_args(**over)) == EINVAL, over
    assert L.nfl_register_moments(*_moments_args(mode=0, d_triangle=None, d_distance=None, d_vertices=None, d_triangles=None,
                                                 scratch_bytes=4 * 440 - 1)) == ESMALL


def test_solve_refuses_before_any_launch(L):
    for over in (dict(d_row=None), dict(d_row=0x1004), dict(d_transform=None), dict(d_transform=0x2004), dict(d_history=None),
                 dict(d_history=0x3004), dict(mode=2), dict(mode=-1), dict(with_scale=2), dict(with_scale=-1), dict(min_pairs=0),
                 dict(min_pairs=-5), dict(iteration=-1), dict(iteration=(2 ** 31 - 1) // 4 + 1), dict(cx=NAN), dict(cy=-INF),
                 dict(cz=INF)):
        assert L.nfl_register_solve(*_solve_args(**over)) == EINVAL, over


# ---- the restatement against numpy's own solvers -----------------------------------------------------------------------------

def test_apply_and_the_row_on_a_hand_case():
    T = rref.pack(2.0, rref.rotation((0, 0, 1), 90), (1, 2, 3))
    x = F([[1, 0, 0], [0, 1, 0], [0.5, 0.5, 4]])
    assert np.allclose(rref.apply(x, T), [[1, 4, 3], [-1, 2, 3], [0, 3, 11]], atol=1e-6)
    assert np.allclose(rref.apply(x, T, vectors=True), [[0, 1, 0], [-1, 0, 0], [-0.5, 0.5, 4]], atol=1e-6)
    assert rref.apply(x, rref.IDENTITY).tobytes() == x.tobytes()
    # two pairs on the unit square (normal +z), one above it by 0.5 and one below by 0.25; a third that is no pair
    sq = dref.square()
    P, Q = F([[0.25, 0.5, 0.5], [0.75, 0.25, -0.25], [NAN, 0, 0]]), F([[0.25, 0.5, 0], [0.75, 0.25, 0], [0, 0, 0]])
    t, d = np.array([1, 0, 0], np.int32), F([0.5, 0.25, 0.0])
    row = rref.moments(P, Q, t, d, sq["vertices"], sq["triangles"], rref.PLANE, INF, (0, 0, 0))
    assert row[rref.COUNT] == 2 and row[rref.SUM_DD] == 0.3125 == row[rref.SUM_RR] and (row[2:rref.ATA] == 0).all()
    a = np.array([[0.5, -0.25, 0, 0, 0, 1, 0.5], [0.25, -0.75, 0, 0, 0, 1, -0.25]])      # (p x n, n, n . p)
    full = a.T @ a
    assert np.array_equal(row[rref.ATA:rref.ATB], full[np.triu_indices(7)])
    assert np.array_equal(row[rref.ATB:rref.SUM_RR], a.T @ np.array([0.5, -0.25]))
    row = rref.moments(P, Q, t, d, sq["vertices"], sq["triangles"], rref.POINT, 0.3, (0, 0, 0))           # the first is too far
    assert row[rref.COUNT] == 1 and row[rref.SUM_P:rref.SUM_P + 3].tolist() == [0.75, 0.25, -0.25] and (row[rref.ATA:] == 0).all()
    assert row[rref.SUM_PQ:rref.SUM_PQ + 9].reshape(3, 3).tolist() == np.outer([0.75, 0.25, -0.25], [0.75, 0.25, 0]).tolist()
    assert rref.moments(P[:0], Q[:0], t[:0], d[:0], sq["vertices"], sq["triangles"], rref.PLANE, INF, (0, 0, 0)).tolist() == [0] * 55


@pytest.mark.parametrize("scale", [False, True])
def test_the_point_solve_is_the_svd_solution(scale):
    """Horn's quaternion through 12 Jacobi sweeps against Umeyama's SVD, on 20 clouds of 300 noisy pairs."""
    worst = 0.0
    for seed in range(20):
        rng = np.random.default_rng(100 + seed)
        P = rng.random((300, 3)).astype(F)
        truth = rref.pack(0.5 + rng.random(), rref.rotation(rng.normal(size=3), 170 * rng.random()), rng.normal(size=3))
        Q = (rref.apply(P, truth) + 0.01 * rng.normal(size=(300, 3))).astype(F)
        T, h = rref.fit(P, Q, scale)
        assert h[0] == 300 and h[2] == rref.OK and h[3] == T[0] and (scale or T[0] == 1.0)
        R = T[1:10].reshape(3, 3)
        # a rotation to rounding: the quaternion is unit to 2 eps, an entry of rot() carries 4 roundings, R R^T sums 3 products
        assert np.abs(R @ R.T - np.eye(3)).max() <= 16 * np.finfo(np.float64).eps and np.linalg.det(R) > 0
        worst = max(worst, np.abs(T - rref.umeyama(P, Q, scale)).max())
    print("point solve against the SVD solution, worst of 13 doubles over 20 seeds:", worst)
    assert worst <= POINT_VS_SVD


def _plane_case(seed, n=200):
    """n well-spread pairs in the unit box: a small triangle with a random normal round every Q, P a little off it."""
    rng = np.random.default_rng(seed)
    Q = rng.random((n, 3))
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    u = np.cross(nrm, rng.normal(size=(n, 3)))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    v = np.cross(nrm, u)
    ver = np.stack([Q - 0.05 * u - 0.05 * v, Q + 0.1 * u, Q + 0.1 * v], axis=1).reshape(-1, 3).astype(F)
    tri = np.arange(3 * n, dtype=np.int32).reshape(n, 3)
    Q = ((ver[0::3].astype(np.float64) + ver[1::3] + ver[2::3]) / 3).astype(F)
    P = (Q + 0.02 * rng.normal(size=(n, 3))).astype(F)
    d = np.sqrt(((P - Q).astype(np.float64) ** 2).sum(axis=1)).astype(F)
    return P, Q, np.arange(n, dtype=np.int32), d, ver, tri


def test_the_plane_solve_is_the_least_squares_solution():
    """The Cholesky solve of the reduced 6 x 6 and 7 x 7 systems against numpy.linalg.lstsq on the 200 un-reduced rows."""
    worst, smallest = 0.0, INF
    for seed in range(20):
        P, Q, t, d, ver, tri = _plane_case(seed)
        c = rref.box_centre(P)
        row = rref.moments(P, Q, t, d, ver, tri, rref.PLANE, INF, c)
        assert row[rref.COUNT] == 200
        N = rref.unit_face_normals(ver, tri)[0][t].astype(np.float64)
        p, e = P.astype(np.float64) - c, P.astype(np.float64) - Q
        A, r = np.concatenate([np.cross(p, N), N, (p * N).sum(axis=1, keepdims=True)], axis=1), (N * e).sum(axis=1)
        for m in (6, 7):
            ref = np.linalg.lstsq(A[:, :m], -r, rcond=None)[0]
            worst = max(worst, np.abs(rref.plane_unknowns(row, m) - ref).max())
            smallest = min(smallest, np.abs(ref).max())
    print("plane solve against lstsq, worst unknown over 20 seeds:", worst, "; the smallest run's largest unknown:", smallest)
    assert PLANE_VS_LSTSQ <= 1e-9 * smallest                               # the bound stays far below what is being solved for
    assert worst <= PLANE_VS_LSTSQ


# ---- the claims about the two modes ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def plane_run():
    target, _, points, truth = rref.problem(20.0, 1.08)
    T, history = rref.register(points, target["vertices"], target["triangles"], mode=rref.PLANE, scale=True, iterations=8)
    return T, history, truth, len(points)


def test_plane_mode_with_scale_converges_within_8_iterations(plane_run):
    T, history, truth, n = plane_run
    print("plane mode, rms per iteration:", ["%.1e" % v for v in history[:, 1]])
    assert 550 < n < 650 and (history[:, 0] == n).all() and (history[:, 2] == rref.OK).all()
    assert history[-1, 1] < 1e-6 and history[0, 1] > 0.05
    assert history[-1, 3] == T[0]


def test_plane_mode_recovers_rotation_translation_and_scale(plane_run):
    T, _, truth, _ = plane_run
    got = rref.errors(T, truth)
    print("plane mode, recovered to (degrees, translation, scale):", got)
    assert all(g <= bound for g, bound in zip(got, RECOVERED)), got


@pytest.fixture(scope="module")
def point_run():
    target, _, points, truth = rref.problem(8.0)
    T, history = rref.register(points, target["vertices"], target["triangles"], mode=rref.POINT, scale=False, iterations=40)
    return T, history, truth, np.abs(target["vertices"]).max()


def test_point_mode_never_gets_worse(point_run):
    """Each step of point-to-point ICP minimises the sum of squares over the current pairs exactly, and taking the closest
    points anew can only shorten them: the rms does not rise.  The slack is what the kernels round: the moved points are
    rounded to fp32 once (half an ulp of a coordinate each, coordinates below 2: 2^-24 x 2 a coordinate, sqrt(3) of it for a
    point) and the distance once more; 4 ulps of 2^-23 x 2 cover both."""
    _, history, _, largest = point_run
    assert largest < 2.0 and (history[:, 2] == rref.OK).all()
    slack = 4 * 2.0 ** -23 * 2.0
    assert (np.diff(history[:, 1]) <= slack).all(), np.diff(history[:, 1]).max()


def test_point_mode_is_still_degrees_off_after_40_iterations(point_run):
    """The recorded reason for the default: the surface is smooth and the points slide along it."""
    T, history, truth, _ = point_run
    angle = rref.errors(T, truth)[0]
    print("point mode after 40 iterations: degrees off", angle, "rms", history[0, 1], "->", history[-1, 1])
    assert angle > 1.0 and history[-1, 1] > 1e-3


def test_the_registered_height_field_lies_on_itself():
    """What registered_distance does, restated: the GPU test holds the device to the same bound."""
    target, source, truth = rref.whole_problem()
    density = 600 / dref.total_area(source["vertices"], source["triangles"])
    points = dref.samples(source["vertices"], source["triangles"], density, 0)[0]
    T, history = rref.register(points, target["vertices"], target["triangles"], mode=rref.PLANE, scale=True, iterations=8)
    before = dref.mesh_distance(source, target, n=600)["chamfer"]
    moved = dict(source, vertices=rref.apply(source["vertices"], T), normals=rref.apply(source["normals"], T, vectors=True))
    after = dref.mesh_distance(moved, target, n=600)["chamfer"]
    print("Chamfer distance of the displaced height field to itself: before", before, "after", after)
    assert (history[:, 2] == rref.OK).all() and before > rref.DISPLACED_CHAMFER and after <= rref.REGISTERED_CHAMFER


# ---- failure statuses ----------------------------------------------------------------------------------------------------------

def test_too_few_pairs_leave_the_transform_alone():
    target, _, points, _ = rref.problem(8.0)
    start = rref.pack(1.01, rref.rotation((1, 0, 0), 2), (0.01, 0, 0))
    T, history = rref.register(points[:5], target["vertices"], target["triangles"], initial=start, iterations=2, min_pairs=6)
    assert T.tobytes() == start.tobytes() and history[:, 0].tolist() == [5, 5] and history[:, 2].tolist() == [rref.FEW] * 2
    assert history[:, 3].tolist() == [1.01] * 2 and np.isfinite(history).all()
    T, history = rref.register(points[:5], target["vertices"], target["triangles"], initial=start, iterations=1, max_distance=1e-9)
    assert T.tobytes() == start.tobytes() and history[0, 0] == 0 and history[0, 2] == rref.FEW and np.isnan(history[0, 1])


@pytest.mark.parametrize("scale", [False, True])
def test_a_planar_target_is_refused_in_plane_mode(scale):
    """Every normal of the unit square is +z: the slide in the plane and the turn about z are columns of zeros, the pivot
    rule meets an exact 0 and refuses; nothing is divided by it and no NaN leaves."""
    sq = dref.square()
    rng = np.random.default_rng(0)
    points = np.concatenate([rng.random((100, 2)), 0.01 * rng.normal(size=(100, 1))], axis=1).astype(F)
    start = rref.pack(1.0, rref.rotation((0, 1, 0), 1), (0, 0, 0.001))
    T, history = rref.register(points, sq["vertices"], sq["triangles"], initial=start, mode=rref.PLANE, scale=scale, iterations=2)
    assert T.tobytes() == start.tobytes() and history[:, 2].tolist() == [rref.SINGULAR] * 2
    assert np.isfinite(history).all() and history[0].tobytes() == history[1].tobytes() and history[0, 0] > 50
    # point mode has no such trouble with the same pairs
    T, history = rref.register(points, sq["vertices"], sq["triangles"], initial=start, mode=rref.POINT, scale=scale, iterations=2)
    assert history[:, 2].tolist() == [rref.OK] * 2 and np.isfinite(T).all()
