"""GPU checks of the mesh cast (csrc/nfl_meshcast.hip through nerf_fl_amd.raycast and the C ABI) against the numpy restatement
of tests/meshcast_ref.py.

What is compared how.  The library is built with -ffp-contract=off and the restatement makes one numpy operation per header
operation, so t, triangle, corner weights and point of a cast, and the hits and openness of an occlusion call, are compared ON
THE BITS.  The expected values come from the restatement's BRUTE cast inside the grid's box; the device is asked through the
grid and through brute mode, first hit and any hit, so THE CONTRACT -- grid mode returns the bits of brute mode -- is checked on
the device for every cell size and origin of tests/test_meshcast_cpu.py.  render_mesh, the existing raster, is the yardstick
of a cross-check that shares no code with the cast.

Sizes.  About 400 rays cross a workgroup of 256; 40 triangles and the ball's few thousand cross the 256-triangle tile of brute
mode, and 255, 256, 257 and 513 stand at its seams; the occlusion mesh has at most 200 vertices at 64 rays each, the analytic scenes one point at up to 4096."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshcast_ref as cref
import meshcolor_ref as mref
from geom_gpu_util import EYES, PAD, ball_mesh, dev as _dev, framed, intrinsics, pose, ptr, same as _same, stream, unframe
from gpu_util import DEV
from nerf_fl_amd import NeRF, PosEmbedding, _lib, eval as nfl_eval, geometry, meshdist, raycast, rendering, synth
from nerf_fl_amd.geometry._call import _count, _launch, _ptr

pytestmark = pytest.mark.gpu

F = np.float32
INF, NAN = np.inf, np.nan
KEYS = ("t", "triangle", "bary", "point")


def explicit_grid(ver, tri, lo, cell, dims):
    """nfl_trigrid_count / _emit for a grid given by hand (triangle_grid chooses its own): a meshdist.TriangleGrid."""
    v, t = _dev(ver, F), _dev(tri, np.int32)
    a = _lib.TriGridArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(v), _ptr(t), v.shape[0], t.shape[0]
    a.lo[:], a.cell, a.dims[:] = lo, cell, dims
    entries, outside = _count(a, "nfl_trigrid_count", _lib.lib().nfl_trigrid_bytes(*dims), 2, torch.device(DEV))
    assert outside == 0
    offsets = torch.empty(dims[0] * dims[1] * dims[2] + 1, dtype=torch.int64, device=DEV)
    rows = torch.empty(entries, dtype=torch.int32, device=DEV)
    a.n_entries, a.d_offsets, a.d_entries = entries, _ptr(offsets), _ptr(rows)
    _launch("nfl_trigrid_emit", a)
    return meshdist.TriangleGrid([float(F(x)) for x in lo], float(F(cell)), list(dims), offsets, rows, v, t)


def _box(grid):
    return cref.box_of(grid.lo, grid.cell, grid.dims)


def _same_fields(got, exp, what, keys=KEYS):
    for k in keys:
        _same(got[k], exp[k], (what, k))


def _mesh(ver, tri):
    return {"vertices": _dev(ver, F), "normals": _dev(ver, F), "triangles": _dev(tri, np.int32)}


# ---- the soup: every cell size, both origins, both methods, both modes

@pytest.fixture(scope="module")
def soup():
    ver, tri = cref.soup40()
    rays = cref.soup_rays(ver, tri)
    return dict(ver=ver, tri=tri, rays=rays, dev=_dev(rays, F))


@pytest.mark.parametrize("name,lo,cell,dims", cref.configs(), ids=[f"{n[0]}-{n[1]:.3g}" for n, _, _, _ in cref.configs()])
def test_cast_equals_the_restatement_on_the_bits(soup, name, lo, cell, dims):
    grid = explicit_grid(soup["ver"], soup["tri"], lo, cell, dims)
    exp = cref.cast(soup["rays"], soup["ver"], soup["tri"], _box(grid))
    assert (exp["triangle"] >= 0).sum() >= 50
    for method in ("grid", "brute"):
        got = raycast.cast_rays(soup["dev"], grid, method=method)
        _same_fields(got, exp, (name, method))
        got = raycast.cast_rays(soup["dev"], grid, mode="any", method=method)
        assert set(got) == {"t", "hit"}
        _same(got["t"], np.where(exp["triangle"] >= 0, F(0), F(INF)).astype(F), (name, method, "any"))
        assert got["hit"].dtype == torch.bool and np.array_equal(got["hit"].cpu().numpy(), exp["triangle"] >= 0)


def test_brute_mode_without_a_box_and_the_default_grid(soup):
    mesh = _mesh(soup["ver"], soup["tri"])
    exp = cref.cast(soup["rays"], soup["ver"], soup["tri"])
    _same_fields(raycast.cast_rays(soup["dev"], mesh, method="brute"), exp, "brute, no box")
    grid = meshdist.triangle_grid(mesh, margin=0.5)
    _same_fields(raycast.cast_rays(soup["dev"], grid), cref.cast(soup["rays"], soup["ver"], soup["tri"], _box(grid)), "default grid")
    view = torch.zeros(len(soup["rays"]), 9, device=DEV)[:, :8]            # rows that are not contiguous
    view.copy_(soup["dev"])
    _same_fields(raycast.cast_rays(view, mesh, method="brute"), exp, "a view")
    none = raycast.cast_rays(torch.zeros(0, 8, device=DEV), grid)
    assert none["t"].shape == (0,) and none["point"].shape == (0, 3)
    for bad in (torch.zeros(4, 7, device=DEV), torch.zeros(4, 8, device=DEV, dtype=torch.float64), torch.zeros(4, 8)):
        with pytest.raises((ValueError, RuntimeError)):
            raycast.cast_rays(bad, grid)


def tile_case(T):
    """The soup of test_meshdist_gpu.py's test_the_lds_tile_of_brute_mode with one triangle made unusable (a NaN corner) at a
    seam of the 256-triangle tile -- index 255 or 256, the last of a full tile or the first of the next; with T = 255, which
    has neither, the last slot of the ragged tile -- and 300 rays: the first eight aimed along the face normals at the
    centroids of the last eight triangles from 0.05 away, 100 aimed at triangles drawn at random from 3 away, the rest
    random through the soup's box.  300 rays are a workgroup and 44 threads of a second one, whose other 212 stage without
    asking.  An aimed ray hits its target or something before it, so a third of the rays hit by construction; the one aimed
    at the unusable triangle, where that is among the last eight, has a NaN origin: no ray, it asks nothing and hits nothing.
    On the restatement 158 to 172 of the 300 hit, and seven of the last eight triangles answer, in all four sizes."""
    ver, tri = mref.soup(T, T)
    ver = ver.copy()
    bad = 255 if T == 256 else min(256, T - 1)
    ver[3 * bad + 1, 0] = NAN
    rng = np.random.default_rng(T)
    c = ver.reshape(T, 3, 3).astype(np.float64)
    centre, normal = c.mean(1), np.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0])
    last = np.arange(T - 8, T)
    some = rng.choice(np.setdiff1d(np.arange(T), [bad]), 100, replace=False)
    d = np.concatenate([-normal[last] / np.linalg.norm(normal[last], axis=1, keepdims=True), rng.normal(size=(100, 3))])
    back = np.concatenate([np.full(8, 0.05), np.full(100, 3.0)])[:, None]
    o = centre[np.concatenate([last, some])] - back * d / np.linalg.norm(d, axis=1, keepdims=True)
    o = np.concatenate([o, rng.uniform([-2.5, -1.5, -6.5], [2.5, 1.5, -1.5], (192, 3))])
    d = np.concatenate([d, rng.normal(size=(192, 3))])
    rays = np.concatenate([o, d, np.zeros((300, 1)), np.full((300, 1), INF)], axis=1).astype(F)
    return ver, tri, bad, rays


@pytest.mark.parametrize("T", [255, 256, 257, 513])
def test_the_lds_tile_of_brute_mode(T):
    """Brute mode at the seams of its 256-triangle tile, first hit and any hit, with a grid's box and without."""
    ver, tri, bad, rays = tile_case(T)
    mesh = _mesh(ver, tri)
    grid = meshdist.triangle_grid(mesh, margin=0.5)
    dev = _dev(rays, F)
    for target, box in ((mesh, None), (grid, _box(grid))):
        exp = cref.cast(rays, ver, tri, box)
        assert exp["triangle"].max() >= T - 8                                 # the last, ragged tile answers too
        assert (exp["triangle"] >= 0).sum() >= 75 and bad not in exp["triangle"]
        got = raycast.cast_rays(dev, target, method="brute")
        _same_fields(got, exp, ("brute", T, box is not None))
        assert bad not in got["triangle"].tolist()
        got = raycast.cast_rays(dev, target, mode="any", method="brute")
        _same(got["t"], np.where(exp["triangle"] >= 0, F(0), F(INF)).astype(F), ("brute, any", T, box is not None))


def test_through_the_c_abi_outputs_framed_and_optional(soup):
    grid = explicit_grid(soup["ver"], soup["tri"], cref.ORIGINS["odd"], 0.25, cref.dims_of(0.25))
    exp = cref.cast(soup["rays"], soup["ver"], soup["tri"], _box(grid))
    N = len(soup["rays"])
    out = {"t": framed(N, (), -3.0, torch.float32), "triangle": framed(N, (), -77, torch.int32),
           "bary": framed(N, (3,), -3.0, torch.float32), "point": framed(N, (3,), -3.0, torch.float32)}
    at = lambda k: out[k].data_ptr() + (12 if k in ("bary", "point") else 4) * PAD
    args = (ptr(soup["dev"]), N, ptr(grid.vertices), ptr(grid.triangles), grid.vertices.shape[0], grid.triangles.shape[0],
            grid.offsets.data_ptr(), ptr(grid.entries), grid.entries.shape[0], *grid.lo, grid.cell, *grid.dims)
    L = _lib.lib()
    assert L.nfl_mesh_cast(*args, 0, at("t"), at("triangle"), at("bary"), at("point"), stream()) == 0
    got = {k: unframe(out[k], N, -77 if k == "triangle" else -3.0, k) for k in out}
    _same_fields(got, exp, "abi")
    only_t = framed(N, (), -3.0, torch.float32)
    assert L.nfl_mesh_cast(*args, 0, only_t.data_ptr() + 4 * PAD, None, None, None, stream()) == 0
    _same(unframe(only_t, N, -3.0, "t alone"), exp["t"], "t alone")
    assert L.nfl_mesh_cast(*args, 1, at("t"), at("triangle"), at("bary"), at("point"), stream()) == 0     # any hit: d_t alone
    _same(unframe(out["t"], N, -3.0, "any"), np.where(exp["triangle"] >= 0, F(0), F(INF)).astype(F), "any")
    _same(unframe(out["triangle"], N, -77, "any leaves the rest"), exp["triangle"], "any leaves the rest")


# ---- the ball: a frame of rays from outside, and rays from inside outward

H = W = 48


@pytest.fixture(scope="module")
def ball():
    mesh = ball_mesh(0.8, 17)
    grid = meshdist.triangle_grid(mesh)
    ver, tri = mesh["vertices"].cpu().numpy(), mesh["triangles"].cpu().numpy()
    c2w, K = pose(EYES[2]), intrinsics(W, H)
    frame = nfl_eval.frame_rays(torch.from_numpy(c2w).float(), torch.from_numpy(K).float(), H, W, 0.0, 10.0, DEV)
    rng = np.random.default_rng(11)
    inside = np.concatenate([rng.uniform(-0.3, 0.3, (500, 3)), rng.normal(size=(500, 3)), np.zeros((500, 1)), np.full((500, 1), INF)],
                            axis=1).astype(F)
    box = _box(grid)
    return dict(mesh=mesh, grid=grid, ver=ver, tri=tri, c2w=c2w, K=K, frame=frame, inside=inside,
                exp_frame=cref.cast(frame.cpu().numpy(), ver, tri, box), exp_inside=cref.cast(inside, ver, tri, box))


def test_a_frame_of_rays_and_rays_from_inside_the_ball(ball):
    assert len(ball["tri"]) > 1000
    covered = ball["exp_frame"]["triangle"] >= 0
    assert 0.1 < covered.mean() < 0.9
    assert (ball["exp_inside"]["triangle"] >= 0).all()                        # a closed surface: every inside ray hits
    r = np.linalg.norm(ball["exp_inside"]["point"].astype(np.float64), axis=1)
    assert np.abs(r - 0.8).max() < 0.02
    for method in ("grid", "brute"):
        _same_fields(raycast.cast_rays(ball["frame"], ball["grid"], method=method), ball["exp_frame"], ("frame", method))
        _same_fields(raycast.cast_rays(_dev(ball["inside"], F), ball["grid"], method=method), ball["exp_inside"], ("inside", method))
    got = raycast.cast_rays(ball["frame"], ball["grid"], mode="any")
    assert np.array_equal(got["hit"].cpu().numpy(), covered)
    _same_fields(raycast.cast_rays(ball["frame"], ball["mesh"]), ball["exp_frame"], "a mesh dict: the same default grid")


# The relative difference between the cast's depth and render_mesh's, over the pixels of the test below: MEASURED, then asserted
# at 10 x the measurement (render_mesh computes in fp32 in camera space, the cast in fp64 in world space).
DEPTH_MEASURED = 4.949e-06
DEPTH_ASSERTED = 4.949e-05


def test_cross_check_against_the_raster_of_render_mesh(ball):
    """The same 48 x 48 camera through two implementations that share no code: the cast, and the raster of nfl_meshray.h
    behind render_mesh.  Wherever the restatement puts the hit further than 1e-3 (barycentric) from every edge of its triangle,
    the two triangle indices agree, with no allowance, and the depths t * |d| and `depth` differ by no more than a relative
    DEPTH_ASSERTED = 4.949e-05 = 10 x DEPTH_MEASURED = 4.949e-06, the worst difference measured on the MI355X (596 of the 599
    covered pixels lie clear of the edges; the triangles agree on all 599).  The edge margin is a condition, not a
    measurement: at least 90 % of the covered pixels must lie outside it, so that the test cannot pass by excluding the frame."""
    exp = ball["exp_frame"]
    covered = exp["triangle"] >= 0
    with np.errstate(invalid="ignore"):
        clear = covered & (exp["bary"].min(axis=1) > 1e-3)
    assert clear.sum() >= 0.9 * covered.sum(), (clear.sum(), covered.sum())
    img = geometry.render_mesh(ball["mesh"], ball["c2w"], ball["K"], H, W, shade="facing")
    got = raycast.cast_rays(ball["frame"], ball["grid"])
    tri_r, depth_r = img["triangle"].reshape(-1).cpu().numpy(), img["depth"].reshape(-1).cpu().numpy().astype(np.float64)
    tri_c = got["triangle"].cpu().numpy()
    depth_c = got["t"].cpu().numpy().astype(np.float64) * np.linalg.norm(ball["frame"][:, 3:6].cpu().numpy().astype(np.float64), axis=1)
    assert np.array_equal(tri_r[clear], tri_c[clear])
    worst = float((np.abs(depth_c[clear] - depth_r[clear]) / depth_r[clear]).max())
    print(f"cast against render_mesh: {clear.sum()} of {covered.sum()} covered pixels clear of the edges; worst relative depth "
          f"difference {worst:.3e}; off the margin the triangles differ in {int((tri_r[covered] != tri_c[covered]).sum())} pixels")
    assert worst <= DEPTH_ASSERTED


# ---- occlusion

def _occ(grid, pts, nrm, K, radius=INF, bias=1e-3, seed=0):
    hits, opn = raycast._occlusion(_dev(pts, F), _dev(nrm, F), grid, K, radius, bias, seed)
    return hits.cpu().numpy(), opn.cpu().numpy()


def _occ_ref(grid, ver, tri, pts, nrm, K, radius=INF, bias=1e-3, seed=0):
    return cref.occlusion(pts, nrm, ver, tri, grid.lo, grid.cell, grid.dims, K, radius, bias, seed)


def test_vertex_occlusion_of_a_small_mesh_equals_the_restatement():
    mesh = ball_mesh(0.8, 5)
    ver, nrm, tri = (mesh[k].cpu().numpy() for k in ("vertices", "normals", "triangles"))
    V = len(ver)
    assert 30 <= V <= 200
    inward = {"vertices": mesh["vertices"], "normals": (-mesh["normals"]).contiguous(), "triangles": mesh["triangles"]}
    grid = meshdist.triangle_grid(mesh)
    bias = 1e-3 * grid.cell
    for m, n, what in ((mesh, nrm, "outward"), (inward, -nrm, "inward")):
        opn = raycast.vertex_occlusion(m, rays=64, seed=3, grid=grid)
        hits, again = raycast._occlusion(m["vertices"], m["normals"], grid, 64, INF, bias, 3)
        exp_hits, exp_open = _occ_ref(grid, ver, tri, ver, n, 64, bias=bias, seed=3)
        _same(hits, exp_hits, (what, "hits"))
        _same(opn, exp_open, (what, "open"))
        assert torch.equal(opn, again)                                        # two runs, the same bits
        assert opn.shape == (V,) and opn.dtype == torch.float32
    assert exp_hits.min() >= 32                                               # inside a closed ball next to nothing is open
    # from outside, looking at the ball: it takes sin^2 = (0.8 / 1.2)^2 = 0.44 of the cosine-weighted hemisphere, so the counts vary
    far_pts, toward = (ver * F(1.5)).astype(F), (-nrm).astype(F)
    hits3, open3 = _occ(grid, far_pts, toward, 64, seed=3)
    exp3 = _occ_ref(grid, ver, tri, far_pts, toward, 64, seed=3)
    _same(hits3, exp3[0], "from outside, hits")
    _same(open3, exp3[1], "from outside, open")
    hits4 = _occ(grid, far_pts, toward, 64, seed=4)[0]
    assert not np.array_equal(hits4, hits3) and abs(hits3[hits3 >= 0].mean() / 64 - 0.444) < 0.1     # another seed, other counts
    short = _occ(grid, far_pts, toward, 64, radius=0.6, seed=3)[0]        # the ball is 0.4 away along the normal, 0.89 at its rim
    _same(short, _occ_ref(grid, ver, tri, far_pts, toward, 64, radius=0.6, seed=3)[0], "a radius")
    assert 0 < short[short >= 0].sum() < hits3[hits3 >= 0].sum()
    pts = _dev(ver[:5] * F(0.5), F)                                           # given points instead of the vertices
    got = raycast.vertex_occlusion(mesh, rays=33, points=pts, normals=_dev(nrm[:5], F), bias=0.0, seed=9)
    _same(got, _occ_ref(grid, ver, tri, ver[:5] * F(0.5), nrm[:5], 33, bias=0.0, seed=9)[1], "points, 33 rays")
    assert (got.cpu().numpy() == 0).all()


@pytest.mark.parametrize("scene,K", [("square", 256), ("box", 256), ("wall", 4096)])
def test_occlusion_of_the_analytic_scenes(scene, K):
    s = getattr(cref, "scene_" + scene)()
    grid = explicit_grid(s["ver"], s["tri"], s["lo"], s["cell"], s["dims"])
    hits, opn = _occ(grid, s["point"], s["normal"], K)
    exp_hits, exp_open = _occ_ref(grid, s["ver"], s["tri"], s["point"], s["normal"], K)
    _same(hits, exp_hits, (scene, "hits"))
    _same(opn, exp_open, (scene, "open"))
    print(f"{scene}: {hits[0]} of {K} rays hit, open {opn[0]}")
    if scene == "square":
        assert opn[0] == 1.0
    elif scene == "box":
        assert opn[0] == 0.0
    else:
        assert abs(float(opn[0]) - 0.5) <= 5 * np.sqrt(0.25 / K)
        assert _occ(grid, s["point"], s["normal"], K, seed=1)[0][0] != hits[0]


def test_points_that_are_no_points_and_a_block_of_several_waves():
    s = cref.scene_wall()
    grid = explicit_grid(s["ver"], s["tri"], s["lo"], s["cell"], s["dims"])
    rng = np.random.default_rng(2)
    pts = np.concatenate([rng.uniform(-3, 3, (9, 2)), np.zeros((9, 1))], axis=1).astype(F)     # 9 points: more than a workgroup's 4
    nrm = np.tile(F([0, 0, 1]), (9, 1))
    pts[2, 0], nrm[5], nrm[7, 1] = NAN, 0.0, INF
    hits, opn = _occ(grid, pts, nrm, 100)
    exp_hits, exp_open = _occ_ref(grid, s["ver"], s["tri"], pts, nrm, 100)
    _same(hits, exp_hits, "hits")
    _same(opn, exp_open, "open")
    assert hits[[2, 5, 7]].tolist() == [-1, -1, -1] and np.isnan(opn[[2, 5, 7]]).all() and (hits[[0, 1, 3, 4, 6, 8]] >= 0).all()


# ---- clipping render rays to a band

def test_clip_rays_to_mesh(ball):
    rays = ball["frame"].clone()
    rays[:, 3:6] *= 2.0                                                       # t is the ray's own parameter: |d| = 2
    rays[::3, 6] = 1.3                                                        # a near that the band reaches below
    t = raycast.cast_rays(rays, ball["grid"])["t"]
    band = 0.25
    out, hit = raycast.clip_rays_to_mesh(ball["grid"], rays, band)
    assert out.shape == rays.shape and hit.dtype == torch.bool and torch.equal(hit, torch.isfinite(t))
    assert 0.1 < hit.float().mean().item() < 0.9 and torch.equal(out[:, :6], rays[:, :6])
    w = band / rays[:, 3:6].norm(dim=1)
    assert torch.equal(out[hit, 6], torch.maximum(rays[hit, 6], t[hit] - w[hit]))
    assert torch.equal(out[hit, 7], torch.minimum(rays[hit, 7], t[hit] + w[hit]))
    assert torch.equal(out[~hit], rays[~hit])                                 # a miss keeps its bounds
    assert bool((out[hit, 6] <= t[hit]).all() and (t[hit] <= out[hit, 7]).all())
    wide, hit2 = raycast.clip_rays_to_mesh(ball["grid"], rays, 100.0)        # a band beyond near and far: clamped to them
    assert torch.equal(hit2, hit) and torch.equal(wide, rays)
    zero, _ = raycast.clip_rays_to_mesh(ball["mesh"], rays, 0.0)
    assert torch.equal(zero[hit, 6], t[hit]) and torch.equal(zero[hit, 7], t[hit])
    mb = raycast.MeshBand(ball["grid"], band)
    a, b = mb.clip(rays)
    assert torch.equal(a, out) and torch.equal(b, hit) and raycast.MeshBand(ball["mesh"], 0.1).grid.dims == ball["grid"].dims


def _models():
    coarse, fine = NeRF("coarse"), NeRF("fine")
    coarse.load_state_dict(synth.make_field_params(21, "sharp", typ="coarse"))
    fine.load_state_dict(synth.make_field_params(22, "sharp", typ="fine"))
    return {"coarse": coarse.to(DEV), "fine": fine.to(DEV)}, {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}


@pytest.mark.parametrize("white_back", [False, True])
def test_clipped_inference_takes_a_mesh_band(ball, white_back):
    h = w = 32
    rays = nfl_eval.frame_rays(torch.from_numpy(ball["c2w"]).float(), torch.from_numpy(intrinsics(w, h)).float(), h, w, 0.5, 6.0, DEV)
    models, emb = _models()
    mb = raycast.MeshBand(ball["grid"], 0.2)
    clipped, hit = mb.clip(rays)
    assert 0.1 < hit.float().mean().item() < 0.9
    with torch.no_grad():
        out = nfl_eval.clipped_inference(models, emb, rays, None, mb, 8, 8, chunk=512, white_back=white_back)
        direct = nfl_eval.batched_inference(models, emb, clipped[hit], None, 8, 8, False, 512, white_back)
    assert set(out) == {k for k in direct if not k.startswith("_")} and "rgb_fine" in out
    for k, v in out.items():
        assert v.shape[0] == h * w and torch.equal(v[hit], direct[k]), k     # the hit rows: bit for bit
        fill = (1.0 if white_back else 0.0) if "rgb" in k else models["fine"].beta_min if k == "beta" else 0.0
        assert bool((v[~hit] == fill).all()), k                               # the missed rows: the documented fill values
    rendering.check_status(torch.device(DEV))
    # an OccupancyGrid passed the same way gives what it gave before
    c = torch.linspace(-1.0, 1.0, 17, device=DEV)
    lat = (0.8 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).contiguous()
    occ = geometry.occupancy_grid(lat, 0.0, (-1.0,) * 3, (1.0,) * 3)
    oc, ohit = geometry.clip_rays(occ, rays)
    with torch.no_grad():
        out = nfl_eval.clipped_inference(models, emb, rays, None, occ, 8, 8, chunk=512, white_back=white_back)
        direct = nfl_eval.batched_inference(models, emb, oc[ohit], None, 8, 8, False, 512, white_back)
    assert all(torch.equal(out[k][ohit], direct[k]) for k in out) and 0 < int(ohit.sum()) < h * w
    with pytest.raises(ValueError):
        nfl_eval.clipped_inference(models, emb, rays, None, ball["grid"], 8, 8)      # a bare grid is neither


def test_render_frame_takes_a_mesh_band(ball):
    models, emb = _models()
    c2w, K = torch.from_numpy(ball["c2w"]).float(), torch.from_numpy(intrinsics(32, 32)).float()
    mb = raycast.MeshBand(ball["grid"], 0.2)
    with torch.no_grad():
        img, res = nfl_eval.render_frame(models, emb, c2w, K, 32, 32, 0.5, 6.0, 8, 8, device=DEV, occupancy=mb)
        ref = nfl_eval.clipped_inference(models, emb, nfl_eval.frame_rays(c2w, K, 32, 32, 0.5, 6.0, DEV), None, mb, 8, 8)
    assert img.shape == (32, 32, 3) and img.dtype == torch.uint8 and torch.equal(res["rgb_fine"], ref["rgb_fine"])
