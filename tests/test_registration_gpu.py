"""GPU checks of the registration (csrc/nfl_register.hip through nerf_fl_amd.registration and the C ABI) against the numpy
restatement of tests/registration_ref.py.

What is compared how.  The library is built with -ffp-contract=off and the restatement makes one numpy operation per header
operation, so the moments row, the applied points, the solved transform with its history row and the WHOLE chain of
register_mesh (sample_surface, nfl_mesh_closest and the three new kernels, eight times over) are compared ON THE BITS.  What
is held to a tolerance -- the recovered transform, fit_transform against the SVD solution, the registered Chamfer distance --
takes its bound from registration_ref, where the CPU tests measure it; the round trip's bound is derived here.  Outputs
written through the C ABI are framed with sentinels, the scratch too.

Sizes.  The moments run 256 threads a workgroup: N = 1, 255, 256, 257 cross it, and 70 001 pairs make 274 partial rows, more
than the 256 threads that fold them, so that a thread adds two.  Every run of pairs holds the ones that must not count."""
import numpy as np
import pytest
import torch

import meshcolor_ref as mref
import meshdist_ref as dref
import registration_ref as rref
from geom_gpu_util import PAD, dev as _dev, framed, ptr, stream, to_dev as _to_dev, unframe
from gpu_util import DEV
from nerf_fl_amd import _lib, meshdist, registration

pytestmark = pytest.mark.gpu

F = np.float32
INF, NAN = np.inf, np.nan
SENTINEL = -7.0
SIZES = (1, 255, 256, 257, 70001, 262145)                                   # 256 * 1024 + 1: the second trip of the reduction's loop
MODES = {"point": rref.POINT, "plane": rref.PLANE}
LIMIT = 0.05                                                                 # max_distance of the moments cases


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype == np.float64 else np.uint32)


def _same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = _bits(got) != _bits(exp)
    assert not bad.any(), (what, int(bad.sum()), "differ", got[bad][:4], exp[bad][:4])


# ---- the cases: a soup with the triangles that must not answer, and pairs round it

@pytest.fixture(scope="module")
def soup():
    """40 seeded triangles, then: 40 a degenerate one (its corners on a line), 41 one with a NaN corner, 42 one that names a
    vertex the mesh does not have."""
    ver, tri = mref.soup(40, 7)
    ver = np.concatenate([ver, F([[0, 0, 0], [1, 1, 1], [2, 2, 2], [NAN, 0, 0]])])
    V = len(ver)
    tri = np.concatenate([tri, np.array([[V - 4, V - 3, V - 2], [0, 1, V - 1], [0, 1, V]], np.int32)])
    return ver, tri


def pairs(N, soup, seed=0):
    """N pairs round the soup, Q some 0.02 from P; among the first 24 (when there are that many) and at the very end the
    pairs that must not count, and one ON the limit that must."""
    ver, tri = soup
    rng = np.random.default_rng(seed + N)
    P = rng.uniform(-1, 1, (N, 3)).astype(F)
    Q = (P + 0.02 * rng.normal(size=(N, 3))).astype(F)
    t = rng.integers(0, 40, N).astype(np.int32)
    d = np.sqrt(((P - Q).astype(np.float64) ** 2).sum(axis=1)).astype(F)
    out = []                                                                # the indices that must not count
    if N >= 24:
        d[3], t[5], Q[7, 1], P[8, 2] = INF, -1, NAN, INF
        d[9] = np.nextafter(F(LIMIT), F(1))                                 # just above the limit
        t[11], t[13], t[15], t[17], t[19] = 40, len(tri), 41, 42, np.iinfo(np.int32).min
        d[21], d[23] = NAN, F(LIMIT)                                        # 23: ON the limit, it counts
        d[N - 1] = INF
        out = [3, 5, 7, 8, 9, 11, 13, 15, 17, 19, 21, N - 1]
    return P, Q, t, d, out


def moments_abi(P, Q, t, d, ver, tri, mode, limit, centre):
    """nfl_register_moments with a framed row and a framed scratch: the (55,) row on the host."""
    L = _lib.lib()
    N = len(P)
    p, q = _dev(P, F), _dev(Q, F)
    ti, di = (None if t is None else _dev(t, np.int32)), (None if d is None else _dev(d, F))
    v, tr = (None, None) if ver is None else (_dev(ver, F), _dev(tri, np.int32))
    nbytes = L.nfl_register_bytes(N)
    assert nbytes % 8 == 0
    scratch = framed(nbytes // 8, (), -7, torch.int64)
    row = framed(rref.COLUMNS, (), SENTINEL, torch.float64)
    rc = L.nfl_register_moments(ptr(p), ptr(q), ptr(ti), ptr(di), ptr(v), ptr(tr), N, 0 if v is None else v.shape[0],
                                0 if tr is None else tr.shape[0], mode, limit, *centre, scratch.data_ptr() + 8 * PAD, nbytes,
                                row.data_ptr() + 8 * PAD, stream())
    assert rc == 0
    unframe(scratch, nbytes // 8, -7, "moments scratch")
    return unframe(row, rref.COLUMNS, SENTINEL, "moments row")


CENTRE = (0.125, -0.25, 0.0625)


@pytest.fixture(scope="module")
def rows(soup):
    """{(N, mode name): (device row on the host, restated row)}, computed once; the solve tests start from them."""
    out = {}
    ver, tri = soup
    for N in SIZES:
        P, Q, t, d, _ = pairs(N, soup)
        for name, mode in MODES.items():
            out[N, name] = (moments_abi(P, Q, t, d, ver, tri, mode, LIMIT, CENTRE),
                            rref.moments(P, Q, t, d, ver, tri, mode, LIMIT, CENTRE))
    return out


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("N", SIZES)
def test_moments_are_the_restatement_on_the_bits(rows, soup, N, mode):
    got, exp = rows[N, mode]
    _same(got, exp, ("moments", N, mode))
    P, Q, t, d, out = pairs(N, soup)
    ok, _ = rref.counting(P, Q, t, d, soup[0], soup[1], LIMIT)
    assert got[rref.COUNT] == ok.sum() and not ok[out].any() and (N < 24 or ok[23])
    assert 0 < got[rref.COUNT] <= N - len(out) and got[rref.SUM_DD] > 0
    other = slice(rref.ATA, rref.COLUMNS) if mode == "point" else slice(rref.SUM_P, rref.ATA)
    assert (_bits(got[other]) == 0).all()                                   # the other mode's columns: +0.0
    mine = got[rref.SUM_P:rref.ATA] if mode == "point" else got[rref.ATA:]
    assert (mine != 0).all()


def test_moments_of_given_partners_and_of_nothing(soup):
    """Point mode without distance, triangle and mesh (fit_transform's call): every finite pair counts and SUM_DD is the
    fp64 |P - Q|^2.  No pair at all: the row of zeros, with no scratch."""
    P, Q, _, _, _ = pairs(257, soup)
    got = moments_abi(P, Q, None, None, None, None, rref.POINT, INF, CENTRE)
    _same(got, rref.moments(P, Q, None, None, None, None, rref.POINT, INF, CENTRE), "given partners")
    assert got[rref.COUNT] == 257 - 2                                        # 7 and 8 hold a NaN and an inf
    for mode in MODES.values():
        assert (_bits(moments_abi(P[:0], Q[:0], None, None, None, None, mode, INF, CENTRE)) == 0).all()
    L = _lib.lib()
    row = framed(rref.COLUMNS, (), SENTINEL, torch.float64)
    assert L.nfl_register_moments(None, None, None, None, None, None, 0, 0, 0, rref.PLANE, INF, 0.0, 0.0, 0.0, None, 0,
                                  row.data_ptr() + 8 * PAD, stream()) == 0
    assert (_bits(unframe(row, rref.COLUMNS, SENTINEL, "empty row")) == 0).all()


# ---- apply

def _similarity(seed=5):
    rng = np.random.default_rng(seed)
    return rref.pack(0.5 + rng.random(), rref.rotation(rng.normal(size=3), 170 * rng.random()), rng.normal(size=3))


@pytest.mark.parametrize("in_place", [False, True])
@pytest.mark.parametrize("vectors", [False, True])
@pytest.mark.parametrize("N", [1, 257])
def test_apply_is_the_restatement_on_the_bits(N, vectors, in_place):
    rng = np.random.default_rng(N)
    x = rng.normal(size=(N, 3)).astype(F)
    if N > 1:
        x[3], x[5, 1] = (0, 0, 0), NAN
    T = _similarity()
    buf = framed(N, (3,), SENTINEL, torch.float32)
    src = _dev(x, F)
    if in_place:
        buf[PAD:PAD + N] = src
    d_in = buf.data_ptr() + 12 * PAD if in_place else ptr(src)
    t13 = _dev(T, np.float64)
    assert _lib.lib().nfl_register_apply(d_in, buf.data_ptr() + 12 * PAD, N, ptr(t13), int(vectors), stream()) == 0
    got = unframe(buf, N, SENTINEL, "applied")
    exp = rref.apply(x, T, vectors)
    ok = ~np.isnan(exp)
    assert np.array_equal(np.isnan(got), ~ok)
    _same(got[ok], exp[ok], ("apply", N, vectors, in_place))
    assert _bits(src.cpu().numpy()[~np.isnan(x)]).tolist() == _bits(x[~np.isnan(x)]).tolist()        # the input is left alone
    assert t13.cpu().numpy().tobytes() == T.tobytes()


# ---- solve

def solve_abi(row, mode, scale, min_pairs, centre, T, iteration=1, slots=3):
    """nfl_register_solve on a host row: (the 13 doubles, the (slots, 4) history) with everything framed."""
    r, t13 = _dev(row, np.float64), framed(13, (), SENTINEL, torch.float64)
    t13[PAD:PAD + 13] = _dev(T, np.float64)
    history = framed(4 * slots, (), SENTINEL, torch.float64)
    rc = _lib.lib().nfl_register_solve(ptr(r), mode, int(scale), min_pairs, *centre, t13.data_ptr() + 8 * PAD,
                                       history.data_ptr() + 8 * PAD, iteration, stream())
    assert rc == 0
    assert r.cpu().numpy().tobytes() == np.asarray(row, np.float64).tobytes()
    return unframe(t13, 13, SENTINEL, "transform"), unframe(history, 4 * slots, SENTINEL, "history").reshape(slots, 4)


@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("N", [257, 70001])
def test_solve_is_the_restatement_on_the_bits(rows, N, mode, scale):
    row = rows[N, mode][0]
    start = _similarity(11)
    T, history = solve_abi(row, MODES[mode], scale, 6, CENTRE, start)
    expT, exph = rref.solve(row, MODES[mode], scale, 6, CENTRE, start)
    assert exph[2] == rref.OK and exph[0] == row[rref.COUNT]
    _same(T, expT, ("transform", N, mode, scale))
    _same(history[1], exph, ("history", N, mode, scale))
    assert (history[[0, 2]] == SENTINEL).all()                              # written at the given iteration and nowhere else
    assert T.tobytes() != start.tobytes() and history[1, 3] == T[0] and (scale or T[0] == start[0])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_solve_failures_leave_the_transform_alone(rows, mode):
    start = _similarity(11)
    row = rows[257, mode][0]
    count = int(row[rref.COUNT])
    T, history = solve_abi(row, MODES[mode], True, count + 1, CENTRE, start, iteration=0)      # one pair short
    assert T.tobytes() == start.tobytes()
    _same(history[0], np.array([count, np.sqrt(row[rref.SUM_DD] / count), rref.FEW, start[0]]), "few")
    assert (history[1:] == SENTINEL).all()
    T, history = solve_abi(row, MODES[mode], True, count, CENTRE, start, iteration=2)          # just enough
    assert history[2, 2] == rref.OK and T.tobytes() != start.tobytes() and (history[:2] == SENTINEL).all()
    empty = np.zeros(rref.COLUMNS)
    T, history = solve_abi(empty, MODES[mode], False, 1, CENTRE, start)
    assert T.tobytes() == start.tobytes() and history[1, 2] == rref.FEW and np.isnan(history[1, 1]) and history[1, 0] == 0


@pytest.mark.parametrize("scale", [False, True])
def test_a_planar_target_is_singular_in_plane_mode(scale):
    """The pairs of points above the unit square: the pivot rule meets an exact 0, the transform stays, no NaN leaves."""
    sq = dref.square()
    rng = np.random.default_rng(0)
    P = np.concatenate([rng.random((100, 2)), 0.01 * rng.normal(size=(100, 1))], axis=1).astype(F)
    got = dref.closest(P, sq["vertices"], sq["triangles"])
    centre = rref.box_centre(P)
    row = moments_abi(P, got["point"], got["triangle"], got["distance"], sq["vertices"], sq["triangles"], rref.PLANE, INF, centre)
    _same(row, rref.moments(P, got["point"], got["triangle"], got["distance"], sq["vertices"], sq["triangles"], rref.PLANE, INF,
                            centre), "planar row")
    start = _similarity(3)
    T, history = solve_abi(row, rref.PLANE, scale, 6, centre, start)
    assert T.tobytes() == start.tobytes() and history[1, 2] == rref.SINGULAR and history[1, 0] == 100
    assert np.isfinite(history[1]).all() and history[1, 3] == start[0]
    _same(history[1], rref.solve(row, rref.PLANE, scale, 6, centre, start)[1], "planar history")
    # a row of NaNs: not solvable either, and nothing is written to the transform
    T, history = solve_abi(np.where(np.arange(rref.COLUMNS) == 0, 100.0, NAN), rref.PLANE, scale, 6, centre, start)
    assert T.tobytes() == start.tobytes() and history[1, 2] == rref.SINGULAR


# ---- the chain

@pytest.fixture(scope="module")
def chain():
    """register_mesh on the inner part of height_field(13), displaced by 20 degrees, a translation and the scale 1.08: the
    result, a second run, the restated loop and the truth."""
    target, source, points, truth = rref.problem(20.0, 1.08)
    tgt, src = _to_dev(target), _to_dev(source)
    run = lambda: registration.register_mesh(src, tgt, mode="plane", scale=True, iterations=8, n=600, seed=0)
    return run(), run(), rref.register(points, target["vertices"], target["triangles"], mode=rref.PLANE, scale=True, iterations=8), truth


def _device13(result):
    return result["device"].cpu().numpy()


def test_the_chain_is_the_restated_loop_on_the_bits(chain):
    got, _, (expT, exph), _ = chain
    h = got["history"]
    print("register_mesh, rms per iteration:", ["%.1e" % v for v in h["rms"]])
    assert h["count"] == [int(c) for c in exph[:, 0]] and h["status"] == ["ok"] * 8
    _same(np.array(h["rms"]), exph[:, 1], "rms per iteration")
    _same(np.array(h["scale"]), exph[:, 3], "scale per iteration")
    _same(_device13(got), expT, "the transform")
    assert got["scale"] == expT[0] and got["rotation"].tobytes() == expT[1:10].tobytes()
    assert got["translation"].tobytes() == expT[10:13].tobytes()
    assert np.array_equal(got["matrix"][:3, :3], expT[0] * expT[1:10].reshape(3, 3)) and got["matrix"][3].tolist() == [0, 0, 0, 1]


def test_two_runs_give_the_same_bits(chain):
    a, b, _, _ = chain
    assert _device13(a).tobytes() == _device13(b).tobytes() and a["history"] == b["history"]


def test_the_chain_recovers_the_transform(chain):
    got, _, _, truth = chain
    errs = rref.errors(_device13(got), truth)
    print("register_mesh recovered to (degrees, translation, scale):", errs)
    assert got["history"]["rms"][-1] < 1e-6 and got["history"]["rms"][0] > 0.05
    assert all(e <= bound for e, bound in zip(errs, rref.RECOVERED)), errs


def test_register_mesh_takes_a_grid_vertices_and_a_schedule_and_refuses_a_plane():
    target, source, _, truth = rref.problem(8.0, 1.0)
    tgt, src = _to_dev(target), _to_dev(source)
    grid = meshdist.triangle_grid(tgt)
    limits = [0.5, 0.25, 0.1, 0.05, 0.05, 0.05]
    got = registration.register_mesh(src, grid, iterations=6, points="vertices", max_distance=limits)
    expT, exph = rref.register(source["vertices"], target["vertices"], target["triangles"], iterations=6, max_distance=limits)
    _same(_device13(got), expT, "vertices, a grid, a schedule")
    _same(np.array(got["history"]["rms"]), exph[:, 1], "rms")
    assert got["scale"] == 1.0 and got["history"]["count"] == [len(source["vertices"])] * 6
    assert rref.errors(_device13(got), truth)[0] < 1e-4
    start = {"scale": 1.0, "rotation": rref.rotation((0.3, -0.5, 0.8), 6.0), "translation": truth[10:13]}
    again = registration.register_mesh(src, grid, initial=start, iterations=4, points="vertices")
    assert again["history"]["rms"][0] < got["history"]["rms"][0] and rref.errors(_device13(again), truth)[0] < 1e-4
    with pytest.raises(RuntimeError, match="could not be solved"):
        registration.register_mesh(src, _to_dev(dref.square()), iterations=2, points="vertices")
    with pytest.raises(RuntimeError, match="fewer than min_pairs"):
        registration.register_mesh(src, grid, iterations=2, points="vertices", max_distance=1e-9)


# ---- the closed form

@pytest.mark.parametrize("scale", [False, True])
def test_fit_transform_is_the_svd_solution(scale):
    rng = np.random.default_rng(42)
    P = rng.random((300, 3)).astype(F)
    truth = _similarity(8)
    if not scale:
        truth[0] = 1.0                                                      # what a rigid fit can reach
    Q = (rref.apply(P, truth) + 0.01 * rng.normal(size=(300, 3))).astype(F)
    P[17, 0] = NAN                                                          # a row that is no point takes no part
    got = registration.fit_transform(_dev(P, F), _dev(Q, F), scale=scale)
    keep = np.isfinite(P).all(axis=1)
    expT, exph = rref.fit(P, Q, scale)
    _same(_device13(got), expT, "fit_transform")
    assert got["history"]["count"] == [299] and got["history"]["status"] == ["ok"] and got["history"]["rms"] == [exph[1]]
    worst = np.abs(_device13(got) - rref.umeyama(P[keep], Q[keep], scale)).max()
    print("fit_transform against the SVD solution:", worst)
    assert worst <= rref.POINT_VS_SVD and (scale or got["scale"] == 1.0)
    moved = registration.transform_points(_dev(P[keep], F), got).cpu().numpy()
    assert np.sqrt(((moved - Q[keep]) ** 2).sum(axis=1).mean()) < 0.02 * 1.01             # the noise that was added, 0.01 an axis
    with pytest.raises(RuntimeError, match="fewer than min_pairs"):
        registration.fit_transform(_dev(P[:2], F), _dev(Q[:2], F))


# ---- on a mesh

@pytest.fixture(scope="module")
def whole():
    target, source, truth = rref.whole_problem()
    return _to_dev(target), _to_dev(source), source, truth


def test_registered_distance_of_the_displaced_height_field_to_itself(whole):
    tgt, src, _, truth = whole
    before = meshdist.mesh_distance(src, tgt, n=600)["chamfer"]
    got = registration.registered_distance(src, tgt, register=dict(scale=True, iterations=8, n=600), n=600)
    print("Chamfer distance before", before, "after", got["chamfer"], "rms per iteration", ["%.1e" % v for v in got["history"]["rms"]])
    assert before > rref.DISPLACED_CHAMFER and got["chamfer"] <= rref.REGISTERED_CHAMFER
    assert got["history"]["status"] == ["ok"] * 8 and set(got["transform"]) == {"scale", "rotation", "translation", "matrix", "device"}
    assert all(e <= bound for e, bound in zip(rref.errors(_device13(got["transform"]), truth), rref.RECOVERED))
    assert got["a_to_b"]["missing"] == 0 and got["b_to_a"]["missing"] == 0


def test_transform_mesh_and_back(whole):
    """There and back the vertices return within fp32 rounding: every coordinate is below 2, so each of the two roundings is
    at most 2^-24 a coordinate; the inverse turns and scales the first into at most sqrt(3) 2^-24 / s of one coordinate."""
    _, src, source, truth = whole
    mesh = dict(src, colors=torch.rand_like(src["vertices"]), label="kept")
    T = {"scale": truth[0], "rotation": truth[1:10].reshape(3, 3), "translation": truth[10:13]}
    moved = registration.transform_mesh(mesh, T)
    assert moved["triangles"] is mesh["triangles"] and moved["colors"] is mesh["colors"] and moved["label"] == "kept"
    assert set(moved) == set(mesh) and moved["vertices"] is not mesh["vertices"]
    _same(moved["vertices"].cpu().numpy(), rref.apply(source["vertices"], truth), "vertices")
    _same(moved["normals"].cpu().numpy(), rref.apply(source["normals"], truth, vectors=True), "normals")
    inv = rref.inverse(truth)
    back = registration.transform_mesh(moved, {"scale": inv[0], "rotation": inv[1:10].reshape(3, 3), "translation": inv[10:13]})
    assert float(moved["vertices"].abs().max()) < 2.0 and np.abs(source["vertices"]).max() < 2.0
    bound = 2.0 ** -24 * (np.sqrt(3.0) / truth[0] + 1.0) * (1 + 1e-6)
    err = np.abs(back["vertices"].cpu().numpy().astype(np.float64) - source["vertices"]).max()
    print("there and back:", err, "bound", bound)
    assert err <= bound
    lengths = np.linalg.norm(back["normals"].cpu().numpy(), axis=1)
    assert np.abs(lengths - 1.0).max() < 1e-6
    for bad in ("T", {"scale": 1.0}, {"scale": NAN, "rotation": np.eye(3), "translation": np.zeros(3)},
                dict(T, device=torch.zeros(12, dtype=torch.float64, device=DEV))):
        with pytest.raises(ValueError, match="transform"):
            registration.transform_points(src["vertices"], bad)
