"""GPU checks of depth fusion: the three kernels of csrc/nfl_tsdf.hip against the numpy restatement of tests/tsdf_ref.py,
through the C ABI and through nerf_fl_amd.fusion.

Both sides evaluate the same fp32 formulae with every operation rounded on its own (the library is built with
-ffp-contract=off; division and square root are correctly rounded on both), so EVERY word is held to equality: accumulators,
counts, lattices, flags and meshes.  Every call through the C ABI writes into buffers framed by sentinels and is made twice.

The lattices are the smallest that cross the boundaries of the code: (2, 2, 2) is the least the entry points take, (5, 4, 3)
is less than a wave, (65, 3, 2) and (257, 3, 3) put the end of an x-row one point past a wave and past a 256-thread
workgroup, (33, 9, 8) is more than one workgroup with rows that straddle waves.  The restatements are computed once per
module and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_ref as gref
import mesh_ref
import meshcolor_ref as mref
import tsdf_ref as tref
from geom_gpu_util import (ball_mesh as _ball_mesh, dev as _dev, F, framed as _framed, PAD, ptr as _ptr, same as _same,
                           stream as _stream, unframe as _unframe)
from gpu_util import DEV
from nerf_fl_amd import _lib, fusion, geometry
from nerf_fl_amd.data import ImageBank

pytestmark = pytest.mark.gpu

SENTINEL = -7.0
RES = [(2, 2, 2), (5, 4, 3), (65, 3, 2), (257, 3, 3), (33, 9, 8)]
LO, HI = (-1.2, -1.0, -0.8), (1.2, 1.0, 0.9)
TRUNC = 0.4
INF, NAN = np.inf, np.nan


def _spacing(res):
    return np.array([(h - l) / (n - 1) for l, h, n in zip(LO, HI, res)], dtype=F)


def _cameras(which):
    """"one": a 65 x 33 frame that cuts the box off above and below.  "four": four frames of different sizes, one of them a
    single pixel, one camera INSIDE the box (lattice points behind it and beside it)."""
    if which == "one":
        return [mref.camera(65, 33, 40, 40, 32.25, 16.5, mref.look_at((3.0, 0.4, 0.2)))]
    return [mref.camera(33, 17, 20, 20, 16, 8, mref.look_at((0.5, 0.2, 3.0))),
            # one pixel, straight above the lattice's first column of points (x, y) = (lo.x, lo.y): they lie ON its axis
            mref.camera(1, 1, 2, 2, 0, 0, np.array([[1, 0, 0, F(LO[0])], [0, 1, 0, F(LO[1])], [0, 0, 1, 3.0]])),
            mref.camera(20, 31, 15, 18, 9.5, 15, mref.look_at((0.3, 0.2, 0.1), (-1.0, 0.0, 0.0))),
            mref.camera(9, 9, 8, 8, 4, 4, mref.look_at((-2.0, 2.0, -2.0)))]


def _salted_maps(cams, seed):
    """Depth maps around the distances of the box (every regime of phi occurs) and pixel weights in (0, 1), a tenth of the
    words of each salted: NaN, +inf, 0 and negative depths; 0, negative and NaN weights."""
    rng = np.random.default_rng(seed)
    depths, weights = [], []
    for c in cams:
        shape = (c["height"], c["width"])
        d = rng.uniform(0.3, 4.5, size=shape).astype(F)
        w = rng.uniform(0.05, 1.0, size=shape).astype(F)
        salt = rng.integers(0, 40, size=shape)
        for k, v in enumerate((NAN, INF, 0.0, -1.5)):
            d[salt == k] = v
        for k, v in enumerate((0.0, -0.5, NAN)):
            w[salt == 10 + k] = v
        depths.append(d)
        weights.append(w)
    return depths, weights


def _fuse_abi(cams, depths, res, sp, trunc, *, lo=LO, first=0, count=None, weights=None, image_weights=None, start=True,
              acc=None, views=None):
    """nfl_tsdf_fuse of cams[first : first + count] into accumulators framed by sentinels; run twice.  Returns host arrays
    (acc (nz, ny, nx, 2), views (nz, ny, nx))."""
    count = len(cams) - first if count is None else count
    nx, ny, nz = res
    P = nx * ny * nz
    run = slice(first, first + count)
    cat = lambda maps: np.concatenate([np.asarray(m, dtype=F).reshape(-1) for m in maps[run]] or [np.zeros(0, F)])
    d_table = torch.from_numpy(mref.table_of(cams).view(np.uint8).reshape(-1).copy()).to(DEV)
    d_depth = _dev(cat(depths), F)
    d_pw = None if weights is None else _dev(cat(weights), F)
    d_iw = None if image_weights is None else _dev(image_weights, F)
    outs = []
    for _ in range(2):
        b_acc, b_views = _framed(P, (2,), SENTINEL, torch.float32), _framed(P, (), -7, torch.int32)
        if not start:
            b_acc[PAD:PAD + P] = _dev(acc, F).view(P, 2)
            b_views[PAD:PAD + P] = _dev(views, np.int32).view(P)
        a = _lib.TsdfFuseArgs()
        a.d_table, a.n_images, a.first, a.count, a.start = d_table.data_ptr(), len(cams), first, count, int(start)
        a.d_depth, a.n_depth, a.d_pixel_weights, a.d_image_weights = _ptr(d_depth), d_depth.numel(), _ptr(d_pw), _ptr(d_iw)
        a.nx, a.ny, a.nz, a.trunc = nx, ny, nz, trunc
        a.lo[:], a.spacing[:] = [float(v) for v in lo], [float(v) for v in sp]
        a.d_acc, a.d_views = b_acc[PAD:].data_ptr(), b_views[PAD:].data_ptr()
        _lib.check(_lib.lib().nfl_tsdf_fuse(C.byref(a), _stream()), "nfl_tsdf_fuse")
        outs.append((_unframe(b_acc, P, SENTINEL, "acc").reshape(nz, ny, nx, 2), _unframe(b_views, P, -7, "views").reshape(nz, ny, nx)))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def _equal(got, exp, what):
    (ga, gv), (ea, ev) = got, exp
    bad = (ga.view(np.uint32) != ea.view(np.uint32)).any(axis=-1) | (gv != ev)
    assert not bad.any(), (what, int(bad.sum()), "points differ", ga[bad][:4], ea[bad][:4], gv[bad][:4], ev[bad][:4])


_CASES = {}


def _case(which, res):
    """(cams, depths, weights, spacing, the restatement with pixel weights) of a camera set and a lattice, computed once."""
    if (which, res) not in _CASES:
        cams = _cameras(which)
        depths, weights = _salted_maps(cams, 11 if which == "one" else 12)
        sp = _spacing(res)
        _CASES[which, res] = cams, depths, weights, sp, tref.fuse(cams, depths, np.array(LO, F), sp, res, F(TRUNC), weights)
    return _CASES[which, res]


# ---- fuse ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["one", "four"])
@pytest.mark.parametrize("res", RES)
def test_fuse_equals_the_restatement(res, which):
    cams, depths, weights, sp, exp = _case(which, res)
    _equal(_fuse_abi(cams, depths, res, sp, TRUNC, weights=weights), exp, "pixel weights")
    assert res == (2, 2, 2) or (exp[1].max() >= 1 and (exp[0][..., 0] > 0).any() and (exp[0][..., 0] < 0).any())
    if which == "four":                                                    # the single pixel is read: by the points on its axis
        assert tref.fuse(cams[1:2], depths[1:2], np.array(LO, F), sp, res, F(TRUNC), weights[1:2])[1].sum() >= 1
    # without pixel weights: NULL is 1 for every pixel
    _equal(_fuse_abi(cams, depths, res, sp, TRUNC), tref.fuse(cams, depths, np.array(LO, F), sp, res, F(TRUNC)), "NULL weights")


@pytest.mark.parametrize("res", [(5, 4, 3), (257, 3, 3)])
def test_fuse_runs_and_image_weights(res):
    cams, depths, weights, sp, exp = _case("four", res)
    lo = np.array(LO, F)
    # a run inside the table: the depth words are numbered from the run's first image
    mid = tref.fuse(cams[1:3], depths[1:3], lo, sp, res, F(TRUNC), weights[1:3])
    _equal(_fuse_abi(cams, depths, res, sp, TRUNC, first=1, count=2, weights=weights), mid, "first=1, count=2")
    # the same bank as one run, and as three runs that continue: equal bits
    got = _fuse_abi(cams, depths, res, sp, TRUNC, first=0, count=1, weights=weights)
    got = _fuse_abi(cams, depths, res, sp, TRUNC, first=1, count=2, weights=weights, start=False, acc=got[0], views=got[1])
    got = _fuse_abi(cams, depths, res, sp, TRUNC, first=3, count=1, weights=weights, start=False, acc=got[0], views=got[1])
    _equal(got, exp, "three runs")
    # an empty run that starts zeroes the accumulators; one that continues leaves them alone (no launch)
    zero = _fuse_abi(cams, depths, res, sp, TRUNC, first=2, count=0)
    assert not zero[0].any() and not zero[1].any()
    kept = _fuse_abi(cams, depths, res, sp, TRUNC, first=2, count=0, start=False, acc=exp[0], views=exp[1])
    _equal(kept, exp, "count == 0 continues")
    # image weights, indexed by the table's n: 0 and NaN drop their images
    iw = np.array([0.5, 0.0, NAN, 2.0], dtype=F)
    want = tref.fuse(cams, depths, lo, sp, res, F(TRUNC), weights, iw)
    _equal(_fuse_abi(cams, depths, res, sp, TRUNC, weights=weights, image_weights=iw), want, "image weights")
    only = tref.fuse([cams[0], cams[3]], [depths[0], depths[3]], lo, sp, res, F(TRUNC), [weights[0], weights[3]], [iw[0], iw[3]])
    assert np.array_equal(want[1], only[1]) and np.array_equal(want[0].view(np.uint32), only[0].view(np.uint32))
    _equal(_fuse_abi(cams, depths, res, sp, TRUNC, first=1, count=2, weights=weights, image_weights=iw, start=False,
                     acc=exp[0], views=exp[1]), exp, "both images of the run dropped")


def test_fuse_exact_places():
    """A 9 x 9 camera at the origin looking down -z (fx = fy = 8, cx = cy = 4) and a lattice whose points project exactly:
    x = +-1.5 at z = -3 onto the frame's first and last column, y = +-1.5 onto its first and last row; the plane z = 0 is
    the camera's own, z = 3 lies behind it.  Then the point (0, 0, -3) alone, at distance 3: a depth of 2 at the centre
    pixel makes phi exactly 1, a depth of 4 exactly -1."""
    cam = mref.camera(9, 9, 8, 8, 4, 4)
    res, lo, sp = (5, 4, 3), np.array([-1.5, -1.5, -3.0], F), np.array([0.75, 1.0, 3.0], F)
    near, far = np.full((9, 9), 3.5, F), np.full((9, 9), 4.0, F)           # |p| is 3 .. 3.68 on the plane z = -3: both in the band
    near[0, 0] = NAN                                                       # the pixel of the corner point (-1.5, 1.5, -3)
    exp = tref.fuse([cam, cam], [near, far], lo, sp, res, F(1.0))
    got = _fuse_abi([cam, cam], [near, far], res, sp, 1.0, lo=lo)
    _equal(got, exp, "exact places")
    acc, views = got
    assert views[1:].max() == 0                                            # on the camera's plane and behind it: nothing
    assert views[0, :, 4].tolist() == [2, 2, 2, 2]                         # x = 1.5: u = 8, the last column
    assert views[0, :, 0].tolist() == [2, 2, 2, 1]                         # x = -1.5: u = 0; its last point reads pixel (0, 0)
    assert views[0, 0].tolist() == [2] * 5 and views[0, 3].tolist() == [1, 2, 2, 2, 2]         # the last and the first row
    near, far = np.full((9, 9), 2.0, F), np.full((9, 9), 4.0, F)
    centre = tref.fuse([cam, cam], [near, far], np.array([0.0, 0.0, -3.0], F), sp, (2, 2, 2), F(1.0))
    both = _fuse_abi([cam, cam], [near, far], (2, 2, 2), sp, 1.0, lo=(0.0, 0.0, -3.0))
    _equal(both, centre, "the centre point")
    assert both[0][0, 0, 0].tolist() == [0.0, 2.0] and both[1][0, 0, 0] == 2          # phi = 1 and phi = -1, both counted
    one = _fuse_abi([cam], [near], (2, 2, 2), sp, 1.0, lo=(0.0, 0.0, -3.0))
    assert one[0][0, 0, 0].tolist() == [1.0, 1.0]


# ---- resolve and support ---------------------------------------------------------------------------------------------------

def _resolve_abi(acc, views, res, min_weight, min_views, fill):
    nx, ny, nz = res
    P = nx * ny * nz
    d_acc, d_views = _dev(acc, F), _dev(views, np.int32)
    outs = []
    for _ in range(2):
        b_lat, b_known = _framed(P, (), SENTINEL, torch.float32), _framed(P, (), 9, torch.uint8)
        a = _lib.TsdfResolveArgs()
        a.d_acc, a.d_views, a.nx, a.ny, a.nz, a.min_views = d_acc.data_ptr(), d_views.data_ptr(), nx, ny, nz, min_views
        a.min_weight, a.fill, a.d_lattice, a.d_known = min_weight, fill, b_lat[PAD:].data_ptr(), b_known[PAD:].data_ptr()
        _lib.check(_lib.lib().nfl_tsdf_resolve(C.byref(a), _stream()), "nfl_tsdf_resolve")
        outs.append((_unframe(b_lat, P, SENTINEL, "lattice").reshape(nz, ny, nx), _unframe(b_known, P, 9, "known").reshape(nz, ny, nx)))
    assert np.array_equal(outs[0][0].view(np.uint32), outs[1][0].view(np.uint32)) and np.array_equal(outs[0][1], outs[1][1])
    return outs[0]


def _support_abi(ver, known, res, lo, sp):
    nx, ny, nz = res
    V = len(ver)
    d_ver, d_known = _dev(np.reshape(ver, (-1, 3)), F), _dev(known, np.uint8)
    outs = []
    for _ in range(2):
        buf = _framed(V, (), 9, torch.uint8)
        a = _lib.TsdfSupportArgs()
        a.d_vertices, a.n_vertices, a.d_known, a.nx, a.ny, a.nz = _ptr(d_ver), V, d_known.data_ptr(), nx, ny, nz
        a.lo[:], a.spacing[:] = [float(v) for v in lo], [float(v) for v in sp]
        a.d_support = buf[PAD:].data_ptr()
        _lib.check(_lib.lib().nfl_tsdf_support(C.byref(a), _stream()), "nfl_tsdf_support")
        outs.append(_unframe(buf, V, 9, "support"))
    assert np.array_equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("res", RES)
def test_resolve_equals_the_restatement(res):
    _, _, _, _, (acc, views) = _case("four", res)
    flat = acc[..., 1].reshape(-1)
    at = int(np.argmax(views.reshape(-1)))                                 # a point some images saw: thresholds at its totals
    total, seen = flat[at], int(views.reshape(-1)[at])
    cases = [(0.5, 1, -1.0), (1e-6, 2, 3.5), (float(total), 1, -1.0), (float(np.nextafter(total, F(INF))), 1, -1.0),
             (1e-6, seen, 0.0), (1e-6, seen + 1, INF)]
    for k, (min_weight, min_views, fill) in enumerate(cases):
        if k in (2, 3) and not total > 0:
            continue                                                        # (2, 2, 2) may see nothing at all
        exp = tref.resolve(acc, views, F(min_weight), min_views, F(fill))
        got = _resolve_abi(acc, views, res, min_weight, min_views, fill)
        assert np.array_equal(got[0].view(np.uint32), exp[0].view(np.uint32)) and np.array_equal(got[1], exp[1]), (res, k)
        if seen and k in (2, 4):
            assert got[1].reshape(-1)[at] == 1
        if seen and k in (3, 5):
            assert got[1].reshape(-1)[at] == 0 and got[0].reshape(-1)[at] == F(fill)


@pytest.mark.parametrize("res", RES)
def test_support_equals_the_restatement(res):
    nx, ny, nz = res
    rng = np.random.default_rng(nx)
    known = (rng.uniform(size=(nz, ny, nx)) < 0.8).astype(np.uint8)
    lo, sp = np.array(LO, F), _spacing(res)
    at = lambda i, j, k: lo + np.array([i, j, k], F) * sp                  # a lattice point, as the kernels place it
    top = (nx - 1, ny - 1, nz - 1)
    hand = [at(0, 0, 0), at(*top), at(1, 0, 1),                            # ON lattice points
            (at(0, 0, 0) + at(1, 0, 0)) / F(2), (at(1, 1, 0) + at(1, 1, 1)) / F(2),            # axis edges
            (at(0, 0, 0) + at(1, 1, 0)) / F(2),                            # a face diagonal
            (at(0, 0, 0) + at(1, 1, 1)) / F(2), at(0, 0, 0) + (at(1, 1, 1) - at(0, 0, 0)) * F(0.25),     # body diagonals
            at(-1, 0, 0), at(0, ny, 0), at(*top) + sp * F(0.01), lo - sp * F(1e-3),            # outside the box
            [NAN, 0, 0], [0, INF, 0], [0, 0, -INF]]
    cloud = rng.uniform(np.array(LO) - 0.1, np.array(HI) + 0.1, size=(300, 3))
    ver = np.concatenate([np.array(hand, dtype=F), cloud.astype(F)])
    exp = tref.support(ver, known, lo, sp)
    got = _support_abi(ver, known, res, lo, sp)
    assert np.array_equal(got, exp), (res, np.nonzero(got != exp)[0][:8])
    assert exp[8:15].max() == 0 and exp[0] == known[0, 0, 0]
    assert nx < 33 or 0 < exp[15:].sum() < 300                             # a cell of the small ones is rarely all known
    # all observed: everything inside the box is supported; nothing observed: nothing is
    assert np.array_equal(_support_abi(ver, np.ones_like(known), res, lo, sp), tref.support(ver, np.ones_like(known), lo, sp))
    assert _support_abi(ver, np.zeros_like(known), res, lo, sp).max() == 0
    assert _support_abi(np.zeros((0, 3), F), known, res, lo, sp).shape == (0,)


# ---- through Python --------------------------------------------------------------------------------------------------------

def _bank_of(cams, seed=5):
    """An ImageBank with the cameras `cams` (its pixels are noise: fusion reads the cameras only)."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, size=(c["height"], c["width"], 3), dtype=np.uint8) for c in cams]
    K = np.stack([np.array([[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1]], dtype=np.float64) for c in cams])
    c2w = np.stack([c["c2w"].reshape(3, 4).astype(np.float64) for c in cams])
    bank = ImageBank(images, c2w, K, 2.0, 6.0, device=DEV)
    assert all(np.array_equal(a["c2w"], b["c2w"]) and a["fx"] == b["fx"] and a["cx"] == b["cx"]
               for a, b in zip(mref.cameras_of(bank.host_table), cams))
    return bank


def _host_mesh(mesh):
    return {k: mesh[k].cpu().numpy() for k in ("vertices", "normals", "triangles")}


@pytest.fixture(scope="module")
def sphere():
    fx = tref.sphere_fixture(17, 3, 33)
    acc, views = tref.fuse(fx["cams"], fx["depths"], fx["lo"], fx["spacing"], fx["res"], fx["trunc"])
    return fx, _bank_of(fx["cams"]), acc, views, tref.resolve(acc, views, 0.5)


def _conditions(c):
    assert c["wall_unfiltered"] >= 1 and c["wall_kept"] == 0
    assert c["V"] > 0 and c["euler"] == 2 and c["every_edge_twice"] and c["orphans"] == 0
    assert c["worst_spacings"] <= 1.0


def test_the_sphere_fixture_on_the_device(sphere):
    fx, bank, acc, views, (lattice, known) = sphere
    box = (tref.BOX[0],) * 3, (tref.BOX[1],) * 3
    depth = _dev(np.stack(fx["depths"]), F)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                                # no host synchronisation up to the support flags
    try:
        out = fusion.fuse_depth(bank, depth, *box, fx["res"], float(fx["trunc"]))
        lat, kn = fusion.tsdf_lattice(out, min_weight=0.5)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    _same(out["acc"], acc, "acc")
    _same(out["views"], views, "views")
    _same(lat, lattice, "lattice")
    _same(kn, known, "known")
    mesh = geometry.extract_surface(lat, 0.0, *box)
    exp_mesh = gref.extract(lattice, 0.0, fx["lo"], fx["spacing"])
    for k in ("vertices", "normals", "triangles"):
        _same(mesh[k], exp_mesh[k], k)
    torch.cuda.set_sync_debug_mode("error")
    try:
        sup = fusion.surface_support(mesh, kn, *box)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    exp_sup = tref.support(exp_mesh["vertices"], known, fx["lo"], fx["spacing"])
    assert sup.dtype == torch.bool
    _same(sup.view(torch.uint8), exp_sup, "support")
    kept = fusion.drop_unsupported(mesh, kn, *box)
    exp_kept = mesh_ref.compact(np.arange(len(exp_sup)), exp_sup.astype(bool), exp_mesh)
    for k in ("vertices", "normals", "triangles"):
        _same(kept[k], exp_kept[k], "kept " + k)
    c = tref.surface_conditions(_host_mesh(mesh), sup.cpu().numpy(), tref.RADIUS, fx["spacing"][0], fx["trunc"])
    print("the sphere on the device:", c)
    _conditions(c)
    assert kept["vertices"].shape[0] == c["V"] and kept["triangles"].shape[0] == c["T"]
    # run by run into the same accumulators: equal bits; and the cleaning that fuse_mesh ends with keeps the one surface
    part = fusion.fuse_depth(bank, depth[:2], *box, fx["res"], float(fx["trunc"]), count=2)
    again = fusion.fuse_depth(bank, depth[2:], *box, fx["res"], float(fx["trunc"]), first=2, into=part)
    assert again is part
    _same(part["acc"], acc, "acc in two runs")
    _same(part["views"], views, "views in two runs")
    cleaned = geometry.clean_mesh(kept, min_triangles=1)
    assert cleaned["triangles"].shape == kept["triangles"].shape and cleaned["vertices"].shape == kept["vertices"].shape


def test_depth_maps_of_a_mesh_fuse_to_its_surface(sphere):
    """The same lattice and cameras, the depth maps now geometry.mesh_depth's of the ball mesh (a sphere of radius 0.8
    extracted on a 17^3 lattice over [-1, 1]^3): the conditions hold again."""
    fx, bank = sphere[:2]
    box = (tref.BOX[0],) * 3, (tref.BOX[1],) * 3
    ball = _ball_mesh()
    depth = torch.stack([geometry.mesh_depth(ball, bank=bank, image=i) for i in range(bank.n_images)])
    assert torch.isfinite(depth).any() and torch.isinf(depth).any()
    out = fusion.fuse_depth(bank, depth, *box, fx["res"], float(fx["trunc"]))
    lat, kn = fusion.tsdf_lattice(out)
    mesh = geometry.extract_surface(lat, 0.0, *box)
    sup = fusion.surface_support(mesh, kn, *box)
    c = tref.surface_conditions(_host_mesh(mesh), sup.cpu().numpy(), tref.RADIUS, fx["spacing"][0], fx["trunc"])
    print("the ball mesh's depth maps:", c)
    _conditions(c)
    kept = fusion.drop_unsupported(mesh, kn, *box)
    assert kept["vertices"].shape[0] == c["V"] and kept["triangles"].shape[0] == c["T"]


def test_python_refuses_before_a_launch(sphere):
    fx, bank = sphere[:2]
    box = (tref.BOX[0],) * 3, (tref.BOX[1],) * 3
    depth = _dev(np.stack(fx["depths"]), F)
    good = fusion.fuse_depth(bank, depth, *box, fx["res"], 0.4)
    for call in (lambda: fusion.fuse_depth(bank, depth, *box, fx["res"], 0.0),
                 lambda: fusion.fuse_depth(bank, depth, *box, fx["res"], float("nan")),
                 lambda: fusion.fuse_depth(bank, depth, *box, (17, 1, 17), 0.4),
                 lambda: fusion.fuse_depth(bank, depth, box[1], box[0], fx["res"], 0.4),
                 lambda: fusion.fuse_depth(bank, depth[:2], *box, fx["res"], 0.4),
                 lambda: fusion.fuse_depth(bank, depth, *box, fx["res"], 0.4, first=5, count=2),
                 lambda: fusion.fuse_depth(bank, depth.cpu(), *box, fx["res"], 0.4),
                 lambda: fusion.fuse_depth(bank, depth.double(), *box, fx["res"], 0.4),
                 lambda: fusion.fuse_depth(bank, depth, *box, fx["res"], 0.4, pixel_weights=depth[:3]),
                 lambda: fusion.fuse_depth(bank, depth, *box, fx["res"], 0.4, image_weights=[1.0, 2.0]),
                 lambda: fusion.fuse_depth(bank, depth, *box, fx["res"], 0.5, into=good),
                 lambda: fusion.fuse_depth(bank, depth, *box, (17, 17, 9), 0.4, into=good),
                 lambda: fusion.tsdf_lattice(good, min_weight=0.0),
                 lambda: fusion.tsdf_lattice(good, min_views=0),
                 lambda: fusion.tsdf_lattice(good, fill=float("nan")),
                 lambda: fusion.tsdf_lattice({"acc": good["acc"]}),
                 lambda: fusion.surface_support(_ball_mesh(), good["views"], *box),
                 lambda: fusion.fuse_mesh({}, {}, bank, *box, fx["res"], run_pixels=0),
                 lambda: fusion.depth_maps({}, {}, bank, 0, 7, 8, 8),
                 lambda: fusion.depth_maps({}, {}, bank, 0, 1, 8, 8, opaque=0.1, empty=0.5)):
        with pytest.raises((ValueError, RuntimeError)):
            call()
    with pytest.raises(ValueError, match="^lo, hi and res are 3 numbers each"):
        fusion.fuse_depth(bank, depth, (0, 0), box[1], fx["res"], 0.4)


def _fields():
    from nerf_fl_amd import NeRF, PosEmbedding, synth

    def module(typ, seed):
        m = NeRF(typ, in_channels_xyz=63, in_channels_dir=27)
        m.load_state_dict(synth.make_field_params(seed, "sharp", typ=typ), strict=True)
        return m.to(DEV)

    return {"coarse": module("coarse", 21), "fine": module("fine", 22)}, {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}


@pytest.fixture(scope="module")
def field_bank():
    eyes = [(0.0, 0.0, 4.0), (0.5, 0.3, 4.0)]
    cams = [mref.camera(9, 7, 12, 12, 4, 3, mref.look_at(e)) for e in eyes]
    return _fields(), _bank_of(cams)


def test_depth_maps_compose_the_inference_outputs(field_bank):
    from nerf_fl_amd import eval as ev
    (models, emb), bank = field_bank
    depth, weights = fusion.depth_maps(models, emb, bank, 0, 2, 8, 8, opaque=0.6, empty=0.2)
    again = fusion.depth_maps(models, emb, bank, 0, 2, 8, 8, opaque=0.6, empty=0.2)
    assert depth.shape == weights.shape == (2 * 63,) and depth.dtype == weights.dtype == torch.float32
    _same(depth, again[0].cpu().numpy(), "depth twice")
    _same(weights, again[1].cpu().numpy(), "weights twice")
    exp_d, exp_w = [], []
    for i in range(2):
        rec = bank.host_table[i]
        K = torch.tensor([[float(rec["fx"]), 0.0, float(rec["cx"])], [0.0, float(rec["fy"]), float(rec["cy"])], [0.0, 0.0, 1.0]])
        _, res = ev.render_frame(models, emb, torch.from_numpy(rec["c2w"].reshape(3, 4).copy()), K, 7, 9, 2.0, 6.0, 8, 8,
                                 ts=int(rec["id"]), white_back=False, device=DEV, output_transient=False)
        d, o = res["depth_fine"], res["opacity_fine"]
        out = torch.full_like(d, float("nan"))
        out[o >= 0.6] = d[o >= 0.6]
        out[o <= 0.2] = float("inf")
        exp_d.append(out)
        exp_w.append(o)
    _same(depth, torch.cat(exp_d).cpu().numpy(), "depth")
    _same(weights, torch.cat(exp_w).cpu().numpy(), "weights")
    one = fusion.depth_maps(models, emb, bank, 1, 1, 8, 8, opaque=0.6, empty=0.2)     # a run inside the bank
    _same(one[0], exp_d[1].cpu().numpy(), "depth of image 1")


def test_fuse_mesh_does_not_depend_on_the_runs(field_bank):
    (models, emb), bank = field_bank
    lo, hi, res = (-1.5, -1.2, -1.0), (1.5, 1.2, 1.5), (11, 9, 10)
    kw = dict(N_samples=8, N_importance=8, opaque=0.6, empty=0.2, min_triangles=None)
    whole = fusion.fuse_mesh(models, emb, bank, lo, hi, res, **kw)
    split = fusion.fuse_mesh(models, emb, bank, lo, hi, res, run_pixels=63, **kw)
    assert set(whole) == {"vertices", "normals", "triangles", "lattice", "known"}
    assert whole["lattice"].shape == (10, 9, 11) and whole["known"].dtype == torch.uint8
    for k in whole:
        _same(split[k], whole[k].cpu().numpy(), k)
    # the pieces, by hand: the default trunc is 3 x the largest spacing
    depth, weights = fusion.depth_maps(models, emb, bank, 0, 2, 8, 8, opaque=0.6, empty=0.2)
    acc = fusion.fuse_depth(bank, depth, lo, hi, res, 3.0 * 0.3, pixel_weights=weights)
    lat, kn = fusion.tsdf_lattice(acc)
    _same(whole["lattice"], lat.cpu().numpy(), "lattice")
    _same(whole["known"], kn.cpu().numpy(), "known")
    cams = mref.cameras_of(bank.host_table)
    d, w = depth.cpu().numpy().reshape(2, 7, 9), weights.cpu().numpy().reshape(2, 7, 9)
    sp = np.array([0.3, 0.3, 2.5 / 9], dtype=F)
    exp = tref.fuse(cams, list(d), np.array(lo, F), sp, res, F(3.0 * 0.3), list(w))
    _same(acc["acc"], exp[0], "acc of rendered maps")
    _same(acc["views"], exp[1], "views of rendered maps")
    assert kn.any()
