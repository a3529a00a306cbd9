"""GPU checks of the mesh solid queries (csrc/nfl_meshcast.hip through nerf_fl_amd.solid and the C ABI) against the numpy
restatement of tests/meshsolid_ref.py.

What is compared how.  Crossings, votes and flags are integers and are compared as such; the expected ones come from the
restatement's BRUTE count inside the grid's box, and the device is asked through the grid and through brute mode, so THE CONTRACT
-- the count-mode walk returns brute mode's integers -- is checked on the device for every cell size and origin of
tests/test_meshcast_cpu.py.  The signed distance and the lattice are compositions: their magnitude has closest_on_mesh's bits,
their value the bits of the restated composition.  The round trip through remesh and the volumes are held to bounds that are
derived where they stand.

Sizes.  About 400 rays cross a workgroup of 256; 40 triangles and the ball's few thousand cross the 256-triangle tile of brute
mode, and 255, 256, 257 and 513 stand at its seams; the lattices have 17^3, 16^3 and (the round trip) 33^3 points."""
import math

import numpy as np
import pytest
import torch

import meshcast_ref as cref
import meshsolid_ref as sref
from geom_gpu_util import PAD, ball_mesh, dev as _dev, framed, ptr, same as _same, stream, unframe
from gpu_util import DEV
from nerf_fl_amd import _lib, geometry, meshdist, solid
from test_meshcast_gpu import explicit_grid, tile_case

pytestmark = pytest.mark.gpu

F = np.float32
INF, NAN = np.inf, np.nan
CUBE = ((-1.0,) * 3, (1.0,) * 3)


def _box(grid):
    return cref.box_of(grid.lo, grid.cell, grid.dims)


def _mesh(ver, tri):
    return {"vertices": _dev(ver, F), "normals": _dev(ver, F), "triangles": _dev(tri, np.int32)}


def _abi_args(grid, rows=True):
    return (ptr(grid.vertices), ptr(grid.triangles), grid.vertices.shape[0], grid.triangles.shape[0],
            grid.offsets.data_ptr() if rows else None, ptr(grid.entries) if rows else None, grid.entries.shape[0] if rows else 0,
            *grid.lo, grid.cell, *grid.dims)


# ---- crossings: the soup, every cell size, both origins, both methods

@pytest.fixture(scope="module")
def soup():
    ver, tri, rays, _ = sref.soup()                                           # with the rays whose near or far cuts a crossing off
    return dict(ver=ver, tri=tri, rays=rays, dev=_dev(rays, F))


@pytest.mark.parametrize("name,lo,cell,dims", cref.configs(), ids=[f"{n[0]}-{n[1]:.3g}" for n, _, _, _ in cref.configs()])
def test_crossings_equal_the_restatement_as_integers(soup, name, lo, cell, dims):
    grid = explicit_grid(soup["ver"], soup["tri"], lo, cell, dims)
    exp = sref.crossings(soup["rays"], soup["ver"], soup["tri"], _box(grid))
    if name[0] != "part":
        assert (exp >= 2).sum() >= 15 and (exp == 1).sum() >= 40
    for method in ("grid", "brute"):
        got = solid.count_crossings(soup["dev"], grid, method=method)
        assert got.dtype == torch.int32 and got.shape == (len(exp),)
        _same(got, exp, (name, method))


def test_crossings_without_a_box_the_default_grid_a_view_and_no_ray(soup):
    mesh = _mesh(soup["ver"], soup["tri"])
    exp = sref.crossings(soup["rays"], soup["ver"], soup["tri"])
    _same(solid.count_crossings(soup["dev"], mesh, method="brute"), exp, "brute, no box")
    grid = meshdist.triangle_grid(mesh, margin=0.5)
    _same(solid.count_crossings(soup["dev"], grid), sref.crossings(soup["rays"], soup["ver"], soup["tri"], _box(grid)), "default grid")
    view = torch.zeros(len(soup["rays"]), 9, device=DEV)[:, :8]            # rows that are not contiguous
    view.copy_(soup["dev"])
    _same(solid.count_crossings(view, mesh, method="brute"), exp, "a view")
    assert solid.count_crossings(torch.zeros(0, 8, device=DEV), grid).shape == (0,)
    for bad in (torch.zeros(4, 7, device=DEV), torch.zeros(4, 8, device=DEV, dtype=torch.float64), torch.zeros(4, 8)):
        with pytest.raises((ValueError, RuntimeError)):
            solid.count_crossings(bad, grid)


@pytest.mark.parametrize("T", [255, 256, 257, 513])
def test_the_lds_tile_of_brute_mode(T):
    """Brute mode at the seams of its 256-triangle tile, with a grid's box and without; the grid count beside it."""
    ver, tri, bad, rays = tile_case(T)
    mesh = _mesh(ver, tri)
    grid = meshdist.triangle_grid(mesh, margin=0.5)
    dev = _dev(rays, F)
    for target, box in ((mesh, None), (grid, _box(grid))):
        exp = sref.crossings(rays, ver, tri, box)
        assert (exp >= 2).sum() >= 40 and exp.max() >= 4
        _same(solid.count_crossings(dev, target, method="brute"), exp, ("brute", T, box is not None))
    _same(solid.count_crossings(dev, grid), exp, ("grid", T))


def test_through_the_c_abi_nothing_is_written_past_the_end(soup):
    grid = explicit_grid(soup["ver"], soup["tri"], cref.ORIGINS["odd"], 0.25, cref.dims_of(0.25))
    box = _box(grid)
    exp = sref.crossings(soup["rays"], soup["ver"], soup["tri"], box)
    N = len(soup["rays"])
    L = _lib.lib()
    for rows in (True, False):
        out = framed(N, (), -77, torch.int32)
        assert L.nfl_mesh_crossings(ptr(soup["dev"]), N, *_abi_args(grid, rows), out.data_ptr() + 4 * PAD, stream()) == 0
        _same(unframe(out, N, -77, ("count", rows)), exp, ("count", rows))
    pts = np.concatenate([soup["rays"][:300, :3], F([[NAN, 0, 0], [0, -INF, 0], [0, 0, -3]])])     # 303: more than a workgroup
    want, want_votes = sref.inside(pts, soup["ver"], soup["tri"], 5, box)
    P, d = len(pts), _dev(pts, F)
    for rows in (True, False):
        votes, flags = framed(P, (), 0xAB, torch.uint8), framed(P, (), 0xAB, torch.uint8)
        assert L.nfl_mesh_inside(ptr(d), P, *_abi_args(grid, rows), 5, votes.data_ptr() + PAD, flags.data_ptr() + PAD, stream()) == 0
        _same(unframe(votes, P, 0xAB, "votes"), want_votes, ("votes", rows))
        _same(unframe(flags, P, 0xAB, "inside"), want.astype(np.uint8), ("inside", rows))
        alone = framed(P, (), 0xAB, torch.uint8)                              # d_inside may be absent
        assert L.nfl_mesh_inside(ptr(d), P, *_abi_args(grid, rows), 5, alone.data_ptr() + PAD, None, stream()) == 0
        _same(unframe(alone, P, 0xAB, "votes alone"), want_votes, ("votes alone", rows))
    assert want_votes[-3:-1].tolist() == [255, 255] and len(set(want_votes.tolist())) >= 4           # an open soup: the votes differ


# ---- inside: the sealed box, the open square, the ball

@pytest.mark.parametrize("scene", ["box", "square"])
def test_inside_on_the_analytic_scenes(scene):
    s = getattr(cref, "scene_" + scene)()
    grid = explicit_grid(s["ver"], s["tri"], s["lo"], s["cell"], s["dims"])
    if scene == "box":
        inner, outer = sref.box_points(s)
        pts = np.concatenate([inner, outer, F([[5, 5, 5], [-40, 0.1, 0.2], [NAN, 0, 0], [0, INF, 0]])])      # beyond the grid's box too
    else:                                                                     # an open mesh: equality with the restatement, no more
        rng = np.random.default_rng(4)
        pts = np.concatenate([rng.uniform(-1.4, 1.4, (60, 3)) * [1, 1, 0.3], s["point"], [[0, 0, -0.2], [0.3, 0.1, 0.4]]]).astype(F)
    d = _dev(pts, F)
    odd = sref.parities(pts, s["ver"], s["tri"], 7, _box(grid))
    for K in (1, 3, 5, 7):
        want, want_votes = sref.majority(pts, odd, K)
        for method in ("grid", "brute"):
            got = solid.inside_mesh(d, grid, directions=K, method=method)
            assert set(got) == {"inside", "votes"} and got["inside"].dtype == torch.bool and got["votes"].dtype == torch.uint8
            _same(got["votes"], want_votes, (scene, K, method, "votes"))
            _same(got["inside"], want, (scene, K, method, "inside"))
        if scene == "box":
            assert want_votes.tolist() == [K] * 10 + [0] * 12 + [255] * 2 and want.tolist() == [True] * 10 + [False] * 14
    if scene == "square":
        assert 0 < odd.sum() < odd.size                                       # some rays cross the square, some do not


@pytest.fixture(scope="module")
def ball():
    mesh = ball_mesh(0.8, 17)
    ver, tri = sref.ball()
    _same(mesh["vertices"], ver, "the fixture is the ball extract_surface emits")
    _same(mesh["triangles"], tri, "the fixture is the ball extract_surface emits")
    grid = meshdist.triangle_grid(mesh)
    pts = sref.ball_points()
    return dict(mesh=mesh, grid=grid, ver=ver, tri=tri, box=_box(grid), pts=pts, dev=_dev(pts, F))


def test_inside_the_ball(ball):
    pts = np.concatenate([ball["pts"], F([[NAN, 0, 0], [0.1, 0.2, INF]])])
    d = _dev(pts, F)
    for K in (3, 7):                                                          # unanimous: checked on the restatement in the CPU tests
        want = np.array([True] * 200 + [False] * 202)
        want_votes = np.array([K] * 200 + [0] * 200 + [255] * 2, dtype=np.uint8)
        for target, method in ((ball["grid"], "grid"), (ball["grid"], "brute"), (ball["mesh"], "grid"), (ball["mesh"], "brute")):
            got = solid.inside_mesh(d, target, directions=K, method=method)
            _same(got["votes"], want_votes, (K, method, "votes"))
            _same(got["inside"], want, (K, method, "inside"))
    again = solid.inside_mesh(d, ball["grid"], directions=7)                 # two runs, the same
    assert torch.equal(again["votes"], got["votes"]) and torch.equal(again["inside"], got["inside"])
    none = solid.inside_mesh(torch.zeros(0, 3, device=DEV), ball["grid"])
    assert none["inside"].shape == (0,) and none["votes"].shape == (0,) and none["inside"].dtype == torch.bool
    for bad in (torch.zeros(4, 2, device=DEV), torch.zeros(4, 3, device=DEV, dtype=torch.float64), torch.zeros(4, 3),
                torch.zeros(3, 4, device=DEV).t()):
        with pytest.raises((ValueError, RuntimeError)):
            solid.inside_mesh(bad, ball["grid"])


def test_signed_distance(ball):
    d = ball["dev"]
    for limit in (None, 0.05):
        plain = meshdist.closest_on_mesh(d, ball["grid"], max_distance=limit)
        got = solid.signed_distance(d, ball["grid"], max_distance=limit)
        assert set(got) == {"distance", "triangle", "point", "bary", "inside", "votes"}
        assert torch.equal(got["distance"].abs().view(torch.int32), plain["distance"].view(torch.int32))     # the magnitude: the bits
        for k in ("triangle", "point", "bary"):
            assert torch.equal(got[k].view(torch.int32), plain[k].view(torch.int32)), k
        inside = got["inside"].cpu().numpy()
        assert inside.tolist() == [True] * 200 + [False] * 200 and got["votes"].cpu().numpy().tolist() == [3] * 200 + [0] * 200
        dist = got["distance"].cpu().numpy()
        assert (dist[inside] < 0).all() and (dist[~inside] > 0).all()         # the sign: from inside
        if limit is None:
            norm = np.linalg.norm(ball["pts"].astype(np.float64), axis=1)
            assert np.isfinite(dist).all() and np.abs(-dist - (0.8 - norm)).max() < 0.03     # the facets cut at most that off
        else:                                                                 # nothing within 0.05 of these points: the sign stays
            assert np.isinf(dist).all() and (plain["triangle"] == -1).all()
    brute = solid.signed_distance(d, ball["mesh"], directions=5, method="brute")
    near = solid.signed_distance(d, ball["mesh"], directions=5)
    assert torch.equal(brute["distance"].view(torch.int32), near["distance"].view(torch.int32)) and torch.equal(brute["votes"], near["votes"])


# ---- the lattice: the restated composition, the round trip, the volumes

RES = (17, 17, 17)


@pytest.fixture(scope="module")
def lattice_ref():
    """The restated composition at the 17^3 lattice points: computed once and kept (meshsolid_ref.ball_lattice)."""
    ref = sref.ball_lattice()
    assert (ref["lo"], ref["hi"]) == CUBE and ref["res"] == RES
    return dict(ref, lattice=sref.lattice_value(ref["sd"], ref["trunc"]))


def test_solid_lattice_equals_the_restated_composition(ball, lattice_ref):
    assert lattice_ref["trunc"] == 0.375
    _same(geometry.lattice_points(*CUBE, RES, DEV).reshape(-1, 3), lattice_ref["pts"], "the points")
    lattice, inside = solid.solid_lattice(ball["mesh"], *CUBE, RES)
    assert lattice.shape == (17, 17, 17) == inside.shape and lattice.dtype == torch.float32 and inside.dtype == torch.bool
    assert lattice.is_contiguous()
    _same(lattice.reshape(-1), lattice_ref["lattice"], "the lattice")
    _same(inside.reshape(-1), lattice_ref["inside"], "inside")
    count = int(lattice_ref["inside"].sum())
    assert int(inside.sum()) == count and abs(count * 0.125 ** 3 - 4 / 3 * math.pi * 0.8 ** 3) < 0.15
    host = lattice_ref["lattice"]
    assert ((host > 0) == lattice_ref["inside"]).all()                        # positive inside: tsdf_lattice's convention
    assert (host == 1).sum() > 50 and (host == -1).sum() > 1000 and (np.abs(host) < 1).sum() > 1000      # +1 deep inside, -1 far outside
    assert np.isinf(lattice_ref["sd"]).sum() > 1000                           # nothing within trunc: +-1 by the side
    wide, _ = solid.solid_lattice(ball["mesh"], *CUBE, RES, trunc=0.2, directions=1)
    assert torch.equal(wide > 0, inside) and not torch.equal(wide, lattice)


# one lattice spacing: linear interpolation of a truncated distance between two lattice points of which one is inside and one
# outside puts the crossing between them, and the surface crosses that edge too
SPACING_33 = 2.0 / 32


def test_remesh_round_trip_and_offset(ball):
    res = (33, 33, 33)
    again = solid.remesh(ball["mesh"], *CUBE, res)
    assert again["triangles"].shape[0] > 4 * ball["tri"].shape[0] * 0.8       # twice the resolution: about four times the triangles
    moved = meshdist.closest_on_mesh(again["vertices"], ball["grid"])["distance"]
    worst = float(moved.max())
    radius = lambda m: float(m["vertices"].double().norm(dim=1).mean())
    s = 0.1
    grown, shrunk = solid.remesh(ball["mesh"], *CUBE, res, offset=s), solid.remesh(ball["mesh"], *CUBE, res, offset=-s)
    print(f"remesh at 33^3: {again['vertices'].shape[0]} vertices, the furthest {worst:.4e} from the original (spacing {SPACING_33}); "
          f"mean radius {radius(again):.5f}, grown by {s}: {radius(grown):.5f}, shrunk: {radius(shrunk):.5f}")
    assert worst <= SPACING_33
    assert abs((radius(grown) - radius(again)) - s) <= SPACING_33 and abs((radius(again) - radius(shrunk)) - s) <= SPACING_33
    assert float(solid.mesh_volume(grown)) > float(solid.mesh_volume(again)) > float(solid.mesh_volume(shrunk)) > 0
    with pytest.raises(ValueError):
        solid.remesh(ball["mesh"], *CUBE, res, offset=3 * SPACING_33)


def test_volume_overlap(ball):
    got = solid.volume_overlap(ball["mesh"], ball["mesh"], *CUBE, RES)
    assert got["iou"] == 1.0 and got["cells_a"] == got["cells_b"] == got["intersection"] == got["union"] > 1000
    assert got["volume_a"] == got["cells_a"] * 0.125 ** 3 == got["volume_intersection"]
    # [-0.5, 0.5]^3 on the 16^3 lattice over [-1, 1]^3: x_i = -1 + 2 i / 15, and +-0.5 would be i = 3.75 and 11.25 -- no point on a
    # face; inside are i = 4 .. 11, 8 per axis
    res = (16, 16, 16)
    pts = sref.lattice_points(*CUBE, res).reshape(-1, 3)
    assert (np.abs(np.abs(pts) - 0.5) > 0.03).all()
    a_ver, a_tri = sref.box_mesh((-0.5,) * 3, (0.5,) * 3)
    b_ver, b_tri = sref.box_mesh((-0.25, -0.4, -0.8), (0.75, 0.6, 0.2))       # the same box shifted by (0.25, 0.1, -0.3)
    in_a, in_b = sref.inside(pts, a_ver, a_tri, 3)[0], sref.inside(pts, b_ver, b_tri, 3)[0]
    assert in_a.sum() == 8 ** 3 == ((np.abs(pts) < 0.5).all(axis=1)).sum()
    a, b = _mesh(a_ver, a_tri), _mesh(b_ver, b_tri)
    alone = solid.volume_overlap(a, a, *CUBE, res)
    assert alone["cells_a"] == 512 == alone["union"] and alone["iou"] == 1.0 and abs(alone["volume_a"] - 512 * (2 / 15) ** 3) < 1e-12
    got = solid.volume_overlap(a, b, *CUBE, res)
    want = (int(in_a.sum()), int(in_b.sum()), int((in_a & in_b).sum()), int((in_a | in_b).sum()))
    assert (got["cells_a"], got["cells_b"], got["intersection"], got["union"]) == want
    # by hand: b holds x: i = 6 .. 13 (8), y: 5 .. 11 (7), z: 2 .. 8 (7); both hold x: 6 .. 11, y: 5 .. 11, z: 4 .. 8
    assert want == (512, 8 * 7 * 7, 6 * 7 * 5, 512 + 392 - 210) and got["iou"] == 210 / 694
    assert all(isinstance(got[k], int) for k in ("cells_a", "cells_b", "intersection", "union"))
    assert solid.volume_overlap(a, b, *CUBE, res) == got                      # every number the same on every run
    far = _mesh(*sref.box_mesh((5, 5, 5), (6, 6, 6)))
    none = solid.volume_overlap(far, far, *CUBE, res)
    assert none["union"] == 0 and math.isnan(none["iou"])


def test_mesh_volume(ball):
    """The box: 8, to fp64 rounding, when it is wound outward -- and 0 for cref.scene_box, the same solid, whose opposite
    faces are wound alike: mesh_volume is the cheap check of a winding that its docstring says it is.  The ball: every point
    of its surface lies between the spheres through its innermost and outermost points, so its volume lies between theirs;
    the outermost point of a triangle mesh is a vertex, and no point of a face is nearer than the face's plane."""
    ver, tri = sref.box_mesh(*CUBE)
    got = solid.mesh_volume(_mesh(ver, tri))
    assert got.dtype == torch.float64 and got.shape == () and got.device.type == "cuda" and abs(float(got) - 8.0) < 1e-12
    assert abs(float(solid.mesh_volume(_mesh(ver, tri[:, ::-1]))) + 8.0) < 1e-12      # wound inward
    s = cref.scene_box()
    assert float(solid.mesh_volume(_mesh(s["ver"], s["tri"]))) == 0.0
    assert float(solid.mesh_volume(_mesh(ver[:0], tri[:0]))) == 0.0
    r_out = float(np.linalg.norm(ball["ver"].astype(np.float64), axis=1).max())
    c = ball["ver"].astype(np.float64)[ball["tri"]]
    normal = np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    r_in = float((np.abs((normal * c[:, 0]).sum(axis=1)) / np.linalg.norm(normal, axis=1)).min())     # no point of a face is nearer than its plane
    assert 0.75 < r_in < r_out <= 0.8 * (1 + 1e-6)                            # a concave field, interpolated: no vertex outside the sphere
    volume = float(solid.mesh_volume(ball["mesh"]))
    print(f"the ball's volume {volume:.6f} between {4 / 3 * math.pi * r_in ** 3:.6f} (r = {r_in:.5f}) and {4 / 3 * math.pi * r_out ** 3:.6f}")
    assert 4 / 3 * math.pi * (r_in * (1 - 1e-6)) ** 3 < volume < 4 / 3 * math.pi * 0.8 ** 3
