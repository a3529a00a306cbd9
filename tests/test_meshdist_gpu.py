"""GPU checks of the mesh distance (csrc/nfl_meshdist.hip through nerf_fl_amd.meshdist and the C ABI) against the numpy
restatement of tests/meshdist_ref.py.

What is compared how.  The library is built with -ffp-contract=off and the restatement makes one numpy operation per header
operation, so closest points (distance, triangle, point, barycentrics, dot), sample counts, points, triangles and normals,
and the reduction row are compared ON THE BITS; grid rows are compared as sorted sets (their order is not defined).  THE
CONTRACT, grid mode returns exactly the bits of brute mode, is checked for every cell size and grid origin below.  Outputs
written through the C ABI are framed with sentinels.

Sizes.  Kernels run 256 threads a workgroup and brute mode stages 256 triangles in LDS: T = 255 / 256 / 257 / 513 cross that
tile; about 430 queries cross a workgroup; the reduction's 70 001 elements make 274 partial rows, more than the 256 threads
that fold them; the sample soup has 70 triangles (more than a wave) with counts of 0, a few, and more than 64."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshcolor_ref as mref
import meshdist_ref as dref
from geom_gpu_util import PAD, ball_mesh, dev as _dev, framed, ptr, same as _same, stream, to_dev as _to_dev, unframe
from gpu_util import DEV
from nerf_fl_amd import _lib, geometry, meshdist

pytestmark = pytest.mark.gpu

F = np.float32
INF, NAN = np.inf, np.nan
KEYS = ("distance", "triangle", "point", "bary")


def _same_fields(got, exp, what, keys=KEYS):
    for k in keys:
        g = got[k].cpu().numpy() if torch.is_tensor(got[k]) else got[k]
        _same(g, exp[k], (what, k))


# ---- the C ABI by hand, outputs framed

def grid_abi(ver, tri, lo, cell, dims):
    """nfl_trigrid_count / _emit for an explicit grid: a meshdist.TriangleGrid, and the totals."""
    L = _lib.lib()
    v, t = _dev(ver, F), _dev(tri, np.int32)
    cells = dims[0] * dims[1] * dims[2]
    nbytes = L.nfl_trigrid_bytes(*dims)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    totals = framed(2, (), -7, torch.int64)
    a = _lib.TriGridArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = ptr(v), ptr(t), v.shape[0], t.shape[0]
    a.lo[:], a.cell, a.dims[:] = lo, cell, dims
    a.d_scratch, a.scratch_bytes, a.d_totals = scratch.data_ptr(), nbytes, totals.data_ptr() + 8 * PAD
    assert L.nfl_trigrid_count(C.byref(a), stream()) == 0
    entries, outside = (int(x) for x in unframe(totals, 2, -7, "grid totals"))
    offsets, rows = framed(cells + 1, (), -7, torch.int64), framed(entries, (), -7, torch.int32)
    a.n_entries, a.d_offsets, a.d_entries = entries, offsets.data_ptr() + 8 * PAD, rows.data_ptr() + 4 * PAD
    assert L.nfl_trigrid_emit(C.byref(a), stream()) == 0
    unframe(offsets, cells + 1, -7, "grid offsets"), unframe(rows, entries, -7, "grid rows")
    g = meshdist.TriangleGrid([float(F(x)) for x in lo], float(F(cell)), list(dims), offsets[PAD:PAD + cells + 1].contiguous(),
                              rows[PAD:PAD + entries].contiguous(), v, t)
    return g, (entries, outside)


def closest_abi(points, ver, tri, grid=None, max_distance=INF, normals=None):
    """nfl_mesh_closest with framed outputs, as host arrays."""
    p = _dev(points, F)
    v, t = (grid.vertices, grid.triangles) if grid is not None else (_dev(ver, F), _dev(tri, np.int32))
    N = p.shape[0]
    out = {"distance": framed(N, (), -3.0, torch.float32), "triangle": framed(N, (), -77, torch.int32),
           "point": framed(N, (3,), -3.0, torch.float32), "bary": framed(N, (3,), -3.0, torch.float32),
           "dot": framed(N, (), -3.0, torch.float32)}
    a = _lib.MeshClosestArgs()
    a.d_points, a.n_points, a.d_vertices, a.d_triangles = ptr(p), N, ptr(v), ptr(t)
    a.n_vertices, a.n_triangles, a.max_distance = v.shape[0], t.shape[0], max_distance
    if grid is not None:
        a.d_offsets, a.d_entries, a.n_entries = grid.offsets.data_ptr(), ptr(grid.entries), grid.entries.shape[0]
        a.lo[:], a.cell, a.dims[:] = grid.lo, grid.cell, grid.dims
    nrm = None if normals is None else _dev(normals, F)
    a.d_normals = ptr(nrm)
    a.d_distance, a.d_triangle = out["distance"].data_ptr() + 4 * PAD, out["triangle"].data_ptr() + 4 * PAD
    a.d_point, a.d_bary = out["point"].data_ptr() + 12 * PAD, out["bary"].data_ptr() + 12 * PAD
    a.d_dot = out["dot"].data_ptr() + 4 * PAD if normals is not None else None
    assert _lib.lib().nfl_mesh_closest(C.byref(a), stream()) == 0
    got = {k: unframe(out[k], N, -77 if k == "triangle" else -3.0, k) for k in out}
    if normals is None:
        assert (got.pop("dot") == -3.0).all()                              # not asked for: not written
    return got


# ---- closest point

ORIGINS = {"round": (-3.0, -2.0, -7.0), "odd": (-3.1, -2.3, -7.7)}           # the second: offsets fp32 does not hold
CELLS = (0.1, 0.25, 1.0 / 3.0, 1.0)
SPAN = (8.4, 4.6, 6.9)                                                      # the boxes reach past x = 5, y = 2, z = -1


def _dims(cell):
    return [int(np.ceil(s / cell)) for s in SPAN]


@pytest.fixture(scope="module")
def soup():
    """40 triangles: 36 of the seeded soup, a unit square of two at z = -4 (a tie across their shared edge), and one
    triangle twice (a tie everywhere); about 430 queries, the awkward ones first."""
    ver, tri = mref.soup(40, 7)
    ver = ver.copy()
    ver[3 * 36:3 * 36 + 3] = [[4, 0, -4], [5, 0, -4], [5, 1, -4]]
    ver[3 * 37:3 * 37 + 3] = [[4, 0, -4], [5, 1, -4], [4, 1, -4]]
    tri = tri.copy()
    tri[39] = tri[38]
    rng = np.random.default_rng(3)
    q = [[4.5, 0.5, -3.75], [4.25, 0.25, -5.0],                             # equidistant from the two of the square
         ver[3 * 38 + 1] + F([0.01, 0.02, 0.03]), ver[3 * 38 + 1] + F([0.5, 0.5, 0.5]),      # nearest the doubled triangle
         ver[0], ver[3 * 20 + 2],                                           # mesh vertices themselves
         [-9, 0, -4], [11, 0, -4], [0, -8, -4], [0, 9, -4], [0, 0, -15], [0, 0, 6], [-9, -9, -15], [12, 8, 5]]      # outside, every side
    for lo in ORIGINS.values():
        for cell in CELLS:
            n = _dims(cell)
            for i in (0, 1, 2, n[0] // 2, n[0] - 1, n[0]):                  # exactly on cell faces, as the kernel places them
                face = [F(lo[k]) + F(min(i, n[k])) * F(cell) for k in range(3)]
                q += [face, [face[0], 0.3, -4.2], [0.7, face[1], -3.1], [0.2, -0.4, face[2]]]
    q += [[k * 0.25, -0.5, -4.0] for k in range(-8, 9)] + [[1.0, j / 3.0, -3.0] for j in range(-3, 4)]     # multiples of a cell
    q = np.concatenate([np.array([np.asarray(x, dtype=F) for x in q], dtype=F), rng.uniform([-3.5, -2.5, -7.5], [5.5, 2.5, -0.5], (200, 3)).astype(F)])
    nrm = rng.normal(size=q.shape).astype(F)
    return dict(ver=ver, tri=tri, q=q, nrm=nrm, exp=dref.closest(q, ver, tri, normals=nrm))


def test_brute_mode_equals_the_restatement_on_the_bits(soup):
    got = closest_abi(soup["q"], soup["ver"], soup["tri"], normals=soup["nrm"])
    _same_fields(got, soup["exp"], "brute", KEYS + ("dot",))
    e = soup["exp"]
    assert e["triangle"][:3].tolist() == [36, 36, 38] and e["distance"][0] == 0.25 and e["distance"][1] == 1.0
    assert e["distance"][4] == 0.0 and e["distance"][5] == 0.0 and (e["triangle"] >= 0).all() and 420 <= len(soup["q"]) <= 440
    mesh = {"vertices": _dev(soup["ver"], F), "normals": _dev(soup["ver"], F), "triangles": _dev(soup["tri"], np.int32)}
    api = meshdist.closest_on_mesh(_dev(soup["q"], F), mesh, method="brute", normals=_dev(soup["nrm"], F))
    _same_fields(api, e, "brute through the module", KEYS + ("dot",))


@pytest.mark.parametrize("origin", sorted(ORIGINS))
@pytest.mark.parametrize("cell", CELLS + (100.0,))
def test_grid_mode_returns_the_bits_of_brute_mode(soup, origin, cell):
    lo, dims = ORIGINS[origin], ([1, 1, 1] if cell == 100.0 else _dims(cell))
    lo = (-50.0, -50.0, -50.0) if cell == 100.0 and origin == "round" else lo     # one cell holding everything (and one that does not)
    grid, (entries, outside) = grid_abi(soup["ver"], soup["tri"], lo, cell, dims)
    assert outside == 0 and entries >= 40
    got = closest_abi(soup["q"], None, None, grid=grid, normals=soup["nrm"])
    _same_fields(got, soup["exp"], ("grid", origin, cell), KEYS + ("dot",))
    api = meshdist.closest_on_mesh(_dev(soup["q"], F), grid)
    _same_fields(api, soup["exp"], ("grid through the module", origin, cell))
    assert "dot" not in api


@pytest.mark.parametrize("limit", [0.3, 1.0])
def test_max_distance_leaves_the_same_infinities_in_both_modes(soup, limit):
    exp = dref.closest(soup["q"], soup["ver"], soup["tri"], limit, soup["nrm"])
    missing = exp["triangle"] < 0
    assert 20 < missing.sum() < len(missing) - 20 and np.isinf(exp["distance"][missing]).all() and np.isnan(exp["dot"][missing]).all()
    _same_fields(closest_abi(soup["q"], soup["ver"], soup["tri"], max_distance=limit, normals=soup["nrm"]), exp, "brute", KEYS + ("dot",))
    for cell in (0.1, 1.0 / 3.0, 1.0):
        grid, _ = grid_abi(soup["ver"], soup["tri"], ORIGINS["odd"], cell, _dims(cell))
        got = closest_abi(soup["q"], None, None, grid=grid, max_distance=limit, normals=soup["nrm"])
        _same_fields(got, exp, ("grid", cell), KEYS + ("dot",))


@pytest.mark.parametrize("T", [255, 256, 257, 513])
def test_the_lds_tile_of_brute_mode(T):
    ver, tri = mref.soup(T, T)
    q = np.random.default_rng(T).uniform([-2.5, -1.5, -6.5], [2.5, 1.5, -1.5], (300, 3)).astype(F)
    exp = dref.closest(q, ver, tri)
    assert exp["triangle"].max() >= T - 8                                    # the last tile answers too
    _same_fields(closest_abi(q, ver, tri), exp, ("brute", T))
    grid = meshdist.triangle_grid({"vertices": _dev(ver, F), "normals": _dev(ver, F), "triangles": _dev(tri, np.int32)})
    _same_fields(meshdist.closest_on_mesh(_dev(q, F), grid), exp, ("grid, the default cell", T))


def test_an_empty_mesh_and_queries_that_are_no_points():
    q = F([[0, 0, 0], [1, 2, 3], [NAN, 0, 0]])
    empty = {"vertices": torch.zeros(0, 3, device=DEV), "normals": torch.zeros(0, 3, device=DEV),
             "triangles": torch.zeros(0, 3, dtype=torch.int32, device=DEV)}
    for method in ("grid", "brute"):
        got = meshdist.closest_on_mesh(_dev(q, F), empty, method=method)
        assert got["triangle"].tolist() == [-1] * 3 and torch.isinf(got["distance"]).all()
        assert torch.isnan(got["point"]).all() and torch.isnan(got["bary"]).all()
    sq = _to_dev(dref.square())
    q = F([[0.5, 0.5, 1], [NAN, 0.5, 1], [0.5, INF, 1], [0.5, 0.5, -INF]])
    for method in ("grid", "brute"):
        got = meshdist.closest_on_mesh(_dev(q, F), sq, method=method, max_distance=2.0)
        assert got["triangle"].tolist() == [0, -1, -1, -1] and got["distance"].tolist() == [1.0, INF, INF, INF]
    assert meshdist.closest_on_mesh(torch.zeros(0, 3, device=DEV), sq)["distance"].shape == (0,)
    none = meshdist.sample_surface(empty, density=10.0)
    assert none["points"].shape == (0, 3) and none["triangles"].shape == (0,)


def test_a_triangle_with_a_nan_corner_is_never_the_answer():
    ver, tri = mref.soup(30, 5)
    ver = ver.copy()
    ver[3 * 4 + 1, 2] = NAN
    ver[3 * 9, 0] = INF
    q = np.concatenate([ver[3 * 4:3 * 4 + 3], ver[3 * 9:3 * 9 + 3], ver[3 * 4:3 * 4 + 3] + F(0.01)])
    q = np.concatenate([q[np.isfinite(q).all(axis=1)], np.random.default_rng(1).uniform(-3, 3, (100, 3)).astype(F) + F([0, 0, -4])])
    exp = dref.closest(q, ver, tri)
    assert not np.isin(exp["triangle"], (4, 9)).any()
    _same_fields(closest_abi(q, ver, tri), exp, "brute")
    mesh = {"vertices": _dev(ver, F), "normals": _dev(ver, F), "triangles": _dev(tri, np.int32)}
    grid = meshdist.triangle_grid(mesh, cell=0.25)
    assert not np.isin(grid.entries.cpu().numpy(), (4, 9)).any()
    _same_fields(meshdist.closest_on_mesh(_dev(q, F), grid), exp, "grid")


# ---- the grid

@pytest.mark.parametrize("origin,cell", [("round", 0.25), ("odd", 1.0 / 3.0), ("odd", 1.0)])
def test_grid_rows_are_the_restatements_as_sets(soup, origin, cell):
    lo, dims = ORIGINS[origin], _dims(cell)
    grid, totals = grid_abi(soup["ver"], soup["tri"], lo, cell, dims)
    rows, exp_totals = dref.grid_rows(soup["ver"], soup["tri"], lo, cell, dims)
    assert totals == exp_totals
    off, ent = grid.offsets.cpu().numpy(), grid.entries.cpu().numpy()
    assert off[0] == 0 and off[-1] == totals[0] and (np.diff(off) == [len(r) for r in rows]).all()
    for c in np.nonzero(np.diff(off))[0]:
        assert sorted(ent[off[c]:off[c + 1]].tolist()) == rows[c], c


def test_a_triangle_spanning_the_box_lies_in_every_cell():
    ver = F([[-1, -1, -1], [1, -1, -1], [-1, 1, 1], [0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1], [9, 9, 9]])
    tri = np.array([[0, 1, 2], [3, 4, 5], [0, 1, 7], [6, 6, 6]], dtype=np.int32)
    grid, totals = grid_abi(ver, tri, (-1.0, -1.0, -1.0), 0.5, (4, 4, 4))
    assert totals == (64 + 1 + 1, 1)                                         # the third names a vertex that is not there
    assert all(0 in grid.row(x, y, z) for x in range(4) for y in range(4) for z in range(4))
    assert grid.row(2, 2, 2) == [0, 1] and grid.row(3, 3, 3) == [0, 3] and grid.row(0, 0, 0) == [0]
    mesh = {"vertices": _dev(ver, F), "normals": _dev(ver, F), "triangles": _dev(tri, np.int32)}
    with pytest.raises(ValueError, match="1 of 4 triangles"):
        meshdist.triangle_grid(mesh)
    mesh["triangles"] = _dev(tri[[0, 1, 3]], np.int32)
    g = meshdist.triangle_grid(mesh, cell=0.5, margin=0.25)
    assert g.lo == [-1.25] * 3 and g.cell == 0.5 and g.dims == [22] * 3 and g.entries.shape[0] > 64
    for bad in (dict(cell=0.0), dict(cell=NAN), dict(cell=-1.0), dict(margin=-0.1), dict(cell=1e-5)):
        with pytest.raises(ValueError):
            meshdist.triangle_grid(mesh, **bad)


# ---- samples

def _sample_soup():
    ver, tri = mref.soup(70, 13)
    ver = ver.copy()
    ver[3 * 5:3 * 5 + 3] = ver[3 * 5]                                       # no area
    c = ver[3 * 8:3 * 8 + 3].mean(axis=0)
    ver[3 * 8:3 * 8 + 3] = c + (ver[3 * 8:3 * 8 + 3] - c) * F(0.01)         # tiny: no sample
    for t in (11, 66):
        c = ver[3 * t:3 * t + 3].mean(axis=0)
        ver[3 * t:3 * t + 3] = c + (ver[3 * t:3 * t + 3] - c) * F(6.0)      # large: its wave emits it
    ver[3 * 20, 1] = NAN
    return ver, tri


def _check_samples(ver, tri, density, seed, what):
    mesh = {"vertices": _dev(ver, F), "normals": _dev(ver, F), "triangles": _dev(tri, np.int32)}
    got = meshdist.sample_surface(mesh, density=density, seed=seed)
    pts, t, nrm = dref.samples(ver, tri, density, seed)
    _same(got["points"], pts, (what, "points"))
    _same(got["triangles"], t, (what, "triangles"))
    _same(got["normals"], nrm, (what, "normals"))
    return mesh, got, dref.sample_counts(ver, tri, density, seed)[0]


def test_samples_of_a_soup_equal_the_restatement_on_the_bits():
    ver, tri = _sample_soup()
    mesh, got, m = _check_samples(ver, tri, 200.0, 7, "soup")
    assert m[5] == 0 and m[8] == 0 and m[20] == 0 and m[11] > 64 and m[66] > 64 and ((m > 0) & (m <= 64)).sum() > 40
    again = meshdist.sample_surface(mesh, density=200.0, seed=7)
    other = meshdist.sample_surface(mesh, density=200.0, seed=8)
    assert all(torch.equal(got[k], again[k]) for k in got)
    assert other["points"].shape != got["points"].shape or not torch.equal(other["points"], got["points"])
    _check_samples(ver, tri, 0.0, 7, "density 0")
    _check_samples(ver, tri, 3000.0, 2 ** 63 + 5, "every triangle by its wave")
    for bad in (dict(density=-1.0), dict(density=NAN), dict(density=INF), dict(density=1.0, n=5), dict(), dict(n=-1), dict(density=1e9)):
        with pytest.raises(ValueError):
            meshdist.sample_surface(mesh, **bad)


def test_samples_of_a_ball_lie_on_their_triangles():
    ball = ball_mesh(n=9)
    ver, tri = ball["vertices"].cpu().numpy(), ball["triangles"].cpu().numpy()
    _, got, m = _check_samples(ver, tri, 400.0, 1, "ball")
    N = got["points"].shape[0]
    assert abs(N - 400.0 * dref.total_area(ver, tri)) < 5 * np.sqrt(len(tri)) and m.max() >= 3
    near = meshdist.closest_on_mesh(got["points"], ball)
    assert near["distance"].max().item() <= 1e-6
    pts, own = got["points"].cpu().numpy(), got["triangles"].cpu().numpy()
    for t in np.unique(own)[::7]:                                           # and their OWN triangle, by the restatement
        assert np.sqrt(dref.point_triangle(pts[own == t], *ver[tri[t]])[2]).max() <= 1e-6
    by_n = meshdist.sample_surface(ball, n=5000, seed=3)
    assert abs(by_n["points"].shape[0] - 5000) < 5 * np.sqrt(len(tri))
    assert torch.allclose(by_n["normals"].norm(dim=1), torch.ones(by_n["normals"].shape[0], device=DEV), atol=1e-6)


# ---- the reduction

@pytest.mark.parametrize("N", [1, 255, 256, 257, 70001, 262145])          # 256 * 1024 + 1: the grid-stride loop's second trip
def test_reduction_equals_the_fixed_order_sum_on_the_bits(N):
    rng = np.random.default_rng(N)
    d = rng.random(N).astype(F) * F(3.0)
    dot_ = rng.uniform(-1, 1, N).astype(F)
    holes = d.copy()
    holes[::5] = INF
    holes[3::11] = NAN
    taus8 = (0.1, 0.5, 1.0, 1.5, 2.0, 2.5, 2.9, 3.5)
    for dist in (d, holes):
        for taus in ((), (1.0,), taus8):
            for dd in (None, dot_):
                row = meshdist._reduce(_dev(dist, F), None if dd is None else _dev(dd, F), list(taus))
                again = meshdist._reduce(_dev(dist, F), None if dd is None else _dev(dd, F), list(taus))
                exp = dref.reduce_row(dist, dd, taus)
                assert row.cpu().numpy().tobytes() == exp.tobytes(), (N, taus, dd is None, row.tolist(), exp.tolist())
                assert torch.equal(row, again)
    assert exp[0] == np.isfinite(holes).sum() and exp[3] == np.max(holes[np.isfinite(holes)], initial=0.0)
    # through the C ABI, the row framed
    L = _lib.lib()
    row = framed(13, (), -5.0, torch.float64)
    scratch = torch.empty(L.nfl_meshdist_reduce_bytes(N) // 8 + 1, dtype=torch.int64, device=DEV)
    dist, a = _dev(holes, F), _lib.MeshDistReduceArgs()
    a.d_distance, a.n, a.n_tau = dist.data_ptr(), N, 8
    a.tau[:] = taus8
    a.d_scratch, a.scratch_bytes, a.d_row = scratch.data_ptr(), L.nfl_meshdist_reduce_bytes(N), row.data_ptr() + 8 * PAD
    assert L.nfl_meshdist_reduce(C.byref(a), stream()) == 0
    assert unframe(row, 13, -5.0, "row").tobytes() == dref.reduce_row(holes, None, taus8).tobytes()


def test_reduction_of_nothing():
    assert meshdist._reduce(torch.zeros(0, device=DEV), None, [1.0]).tolist() == [0.0] * 13
    assert meshdist._reduce(torch.full((300,), INF, device=DEV), None, [1.0]).tolist() == [0.0] * 13


# ---- the whole function

def test_square_shifted_along_its_normal():
    r = meshdist.mesh_distance(_to_dev(dref.square()), _to_dev(dref.square((0, 0, 0.25))), n=2000, thresholds=(0.2, 0.3), seed=3)
    print("square shifted by 0.25 along its normal:", r)
    dref.check_shifted_along_the_normal(r)
    assert all(isinstance(v, float) for v in (r["chamfer"], r["hausdorff"], r["normal_consistency"], r["a_to_b"]["mean"]))


def test_square_shifted_in_its_plane():
    r = meshdist.mesh_distance(_to_dev(dref.square()), _to_dev(dref.square((0.5, 0, 0))), n=4000, seed=5)
    print("square shifted by 0.5 in its plane:", r)
    dref.check_shifted_in_the_plane(r["a_to_b"])
    dref.check_shifted_in_the_plane(r["b_to_a"])
    assert abs(r["normal_consistency"] - 1.0) <= 1e-6
    far = meshdist.mesh_distance(_to_dev(dref.square()), _to_dev(dref.square((0.5, 0, 0))), n=4000, seed=5, max_distance=0.25)
    assert 0 < far["a_to_b"]["missing"] < far["a_to_b"]["n"] and far["a_to_b"]["max"] <= 0.25 and far["hausdorff"] <= 0.25


@pytest.fixture(scope="module")
def balls():
    return ball_mesh(0.8, n=17), ball_mesh(0.8, n=33)


def test_a_mesh_against_itself(balls):
    m = balls[0]
    r = meshdist.mesh_distance(m, m, points="vertices", thresholds=(1e-5,))
    assert r["chamfer"] == 0.0 and r["hausdorff"] == 0.0 and r["fscore"] == [1.0] and r["a_to_b"]["rms"] == 0.0
    assert r["a_to_b"]["n"] == m["vertices"].shape[0] and r["a_to_b"]["missing"] == 0
    r = meshdist.mesh_distance(m, m, n=20000, thresholds=(1e-5,))
    print("a ball against itself, 20 000 samples:", r)
    assert r["hausdorff"] <= 1e-6 and r["fscore"] == [1.0] and abs(r["normal_consistency"] - 1.0) <= 1e-5


def test_two_extractions_of_one_ball(balls):
    """Both surfaces interpolate the same field on tetrahedra of the coarser lattice's cells at most: the true crossing and
    the interpolated one lie on one tetrahedron edge, the longest of which is sqrt(3) spacings."""
    coarse, fine = balls
    bound = np.sqrt(3.0) * (2.0 / 16)
    r = meshdist.mesh_distance(coarse, fine, n=50000, thresholds=(0.01,), seed=1)
    print("ball 17^3 against ball 33^3:", r)
    assert r["hausdorff"] < bound and r["a_to_b"]["missing"] == r["b_to_a"]["missing"] == 0
    for m in balls:
        p = meshdist.sample_surface(m, n=50000, seed=1)["points"]
        off = (p.double().norm(dim=1) - 0.8).abs().max().item()
        print("  samples off the sphere by at most", off)
        assert off < bound
    assert r["normal_consistency"] > 0.99 and r["chamfer"] < r["hausdorff"]
    swapped = meshdist.mesh_distance(fine, coarse, n=50000, thresholds=(0.01,), seed=1)
    assert swapped["a_to_b"] == r["b_to_a"] and swapped["b_to_a"] == r["a_to_b"]
    assert swapped["precision"] == r["recall"] and swapped["recall"] == r["precision"] and swapped["fscore"] == r["fscore"]
    for k in ("chamfer", "hausdorff", "normal_consistency"):
        assert np.float64(swapped[k]).tobytes() == np.float64(r[k]).tobytes(), k


@pytest.mark.parametrize("cell", [0.2, 0.31])
def test_simplification_moves_no_vertex_further_than_a_cell_diagonal(balls, cell):
    mesh = balls[1]
    simple = geometry.simplify_mesh(mesh, cell)
    r = meshdist.mesh_distance(mesh, simple, points="vertices")
    print(f"ball 33^3 simplified with cell {cell}:", r)
    assert simple["vertices"].shape[0] < mesh["vertices"].shape[0] // 4
    assert r["a_to_b"]["max"] <= np.sqrt(3.0) * cell and r["b_to_a"]["max"] <= np.sqrt(3.0) * cell
    assert r["a_to_b"]["n"] == mesh["vertices"].shape[0] and r["b_to_a"]["n"] == simple["vertices"].shape[0]


def test_read_ply_fills_missing_normals_on_the_device(tmp_path, balls):
    m = balls[0]
    path = str(tmp_path / "ball.ply")
    geometry.write_ply(path, m)
    back = meshdist.read_ply(path, device=DEV)
    assert all(torch.equal(back[k], m[k]) for k in ("vertices", "normals", "triangles"))
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    V = m["vertices"].shape[0]
    rec = np.frombuffer(body[:24 * V], dtype=np.float32).reshape(V, 6)[:, :3]
    head = b"".join(l + b"\n" for l in head.split(b"\n") if l and l.split()[-1] not in (b"nx", b"ny", b"nz"))
    open(path, "wb").write(head + b"end_header\n" + rec.tobytes() + body[24 * V:])
    bare = meshdist.read_ply(path, device=DEV)
    assert torch.equal(bare["vertices"], m["vertices"]) and torch.equal(bare["normals"], geometry.vertex_normals(m))
