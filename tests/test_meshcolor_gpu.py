"""GPU checks of mesh colour: the depth and blend kernels (csrc/nfl_meshcolor.hip) against the numpy restatement of
tests/meshcolor_ref.py, through the C ABI and through geometry.mesh_depth / color_mesh_from_images / extract_mesh.

Both sides evaluate the same fp32 formulae with every operation rounded on its own (the library is built with
-ffp-contract=off; division and square root are correctly rounded on both), so EVERY word is held to equality: depth maps,
accumulators, colours, counts and masks.  The restatement brute-forces every triangle against every pixel, so the equality
also shows that the raster kernel's boxes (and its wave path for boxes above 64 pixels) lose no hit.

The shapes are the smallest that cross the boundaries of the code: 1 / 63 / 64 / 65 / 257 triangles and vertices for the
waves and the 256-thread workgroups, frames of 1 x 1 up to 65 x 33, boxes below and above 64 pixels.  The restatement of a
case is computed once per module and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshcolor_ref as mref
from geom_gpu_util import (ball_mesh as _ball_mesh, dev as _dev, EYES, F, frame as _frame, framed as _framed,
                           intrinsics as _intrinsics, PAD, pose as _pose, stream as _stream, unframe as _unframe)
from gpu_util import DEV
from nerf_fl_amd import NeRF, PosEmbedding, _lib, geometry, synth
from nerf_fl_amd.data import ImageBank

pytestmark = pytest.mark.gpu

SENTINEL = -7.0


def _depth_abi(ver, tri, cams, first=0, count=None):
    """nfl_mesh_depth of cams[first : first + count] into a buffer framed by sentinels; run twice."""
    count = len(cams) - first if count is None else count
    table = mref.table_of(cams)
    n = int(sum(c["width"] * c["height"] for c in cams[first:first + count]))
    d_ver, d_tri = _dev(np.reshape(ver, (-1, 3)), F), _dev(np.reshape(tri, (-1, 3)), np.int32)
    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    outs = []
    for _ in range(2):
        buf = _framed(n, (), SENTINEL, torch.float32)
        a = _lib.MeshDepthArgs()
        a.d_vertices = d_ver.data_ptr() if d_ver.numel() else None
        a.d_triangles = d_tri.data_ptr() if d_tri.numel() else None
        a.n_vertices, a.n_triangles = d_ver.shape[0], d_tri.shape[0]
        a.d_table, a.n_images, a.first, a.count = d_table.data_ptr(), len(cams), first, count
        a.d_depth, a.n_depth = buf[PAD:].data_ptr(), n
        _lib.check(_lib.lib().nfl_mesh_depth(C.byref(a), _stream()), "nfl_mesh_depth")
        outs.append(_unframe(buf, n, SENTINEL, "depth"))
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    return outs[0]


def _check_depth(ver, tri, cams, what):
    got = _depth_abi(ver, tri, cams)
    exp = mref.run_depth(ver, tri, cams)
    bad = got.view(np.uint32) != exp.view(np.uint32)
    assert not bad.any(), (what, int(bad.sum()), "words differ", got[bad][:4], exp[bad][:4])
    return got


# ---- depth -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_depth_soup_triangle_counts(T):
    ver, tri = mref.soup(400, 7)
    got = _check_depth(ver, tri[:T], [_frame(65, 33)], f"T={T}")
    assert np.isfinite(got).any() or T == 1


@pytest.mark.parametrize("size", [(1, 1), (63, 5), (64, 64), (65, 33)])
def test_depth_soup_frame_sizes(size):
    ver, tri = mref.soup(400, 7)
    got = _check_depth(ver, tri[:257], [_frame(*size)], f"frame {size}")
    assert got.shape == (size[0] * size[1],)


def test_depth_run_of_three_cameras_of_different_sizes():
    ver, tri = mref.soup(400, 7)
    cams = [mref.camera(33, 17, 20, 20, 16, 8, mref.look_at((0.5, 0.2, 1.0), (0, 0, -4))),
            mref.camera(65, 33, 40, 40, 32.25, 16.5),
            mref.camera(20, 31, 15, 18, 9.5, 15, mref.look_at((4.0, 0.0, -4.0), (0, 0, -4))),
            mref.camera(9, 9, 8, 8, 4, 4)]
    exp = mref.run_depth(ver, tri[:257], cams)
    got = _depth_abi(ver, tri[:257], cams)
    assert np.array_equal(got.view(np.uint32), exp.view(np.uint32))
    # a run inside the table: the words are numbered from the run's first image
    n0, n3 = 33 * 17, 81
    mid = _depth_abi(ver, tri[:257], cams, first=1, count=2)
    assert np.array_equal(mid.view(np.uint32), exp[n0:-n3].view(np.uint32))
    assert all(np.isfinite(exp[s]).any() for s in (slice(0, n0), slice(n0, n0 + 65 * 33), slice(n0 + 65 * 33, -n3)))


def test_depth_salted_soup():
    ver, tri = mref.soup(400, 7)
    ver, tri = ver[:3 * 130].copy(), tri[:130].copy()
    ver[3 * 5 + 1, 0] = np.nan                                       # a NaN vertex
    ver[3 * 6] = [np.inf, 0, -3]
    ver[3 * 9 + 2] = ver[3 * 9 + 1]                                  # a degenerate triangle: two corners coincide
    ver[3 * 12:3 * 12 + 3, 2] *= -1                                  # a triangle behind the camera
    ver[3 * 70:3 * 70 + 3] = [[-1, -1, -3], [1, -1, -3], [0.3, 1, 1.5]]       # one straddling the camera plane
    ver[3 * 71:3 * 71 + 3] = [[0, -1, -3], [0, 1, -3], [0, 0, -5]]   # edge-on: det == 0 on a column when cx is an integer
    tri[100] = [3, 4, 3 * 130]                                       # an index past the vertices
    tri[101] = [-1, 4, 5]
    for cam in (_frame(65, 33), mref.camera(65, 33, 40, 40, 32, 16)):
        _check_depth(ver, tri, [cam], "salted")


def test_depth_large_and_small_boxes():
    """One triangle over the whole 65 x 33 frame (a box of 2145 pixels: the wave path), a sliver thinner than a pixel (a
    box of a few pixels that most of its rays miss), and both in front of a soup of ordinary ones."""
    cam = _frame(65, 33)
    big = np.array([[-9, -5, -5], [9, -5, -5], [0, 9, -5]], dtype=F)
    # 0.03 pixels thick where it crosses row 16 (y = 0.025 at z = -2), between columns 31.9 and 32.2: one pixel centre
    sliver = np.array([[-0.16, 0.020, -2], [0.19, 0.031, -2], [0.04, 0.027, -2]], dtype=F)
    got = _check_depth(big, [[0, 1, 2]], [cam], "big")
    assert np.isfinite(got).all()
    got = _check_depth(sliver, [[0, 1, 2]], [cam], "sliver")
    assert np.isfinite(got).sum() == 1 and np.isfinite(got.reshape(33, 65)[16, 32])
    ver, tri = mref.soup(400, 7)
    ver = np.concatenate([ver[:3 * 65], big, sliver])
    tri = np.concatenate([tri[:65], [[195, 196, 197], [198, 199, 200]]]).astype(np.int32)
    _check_depth(ver, tri, [cam, _frame(64, 64)], "big + sliver + soup")


def test_depth_of_nothing():
    cam = _frame(63, 5)
    ver, tri = mref.soup(4, 7)
    for v, t in ((np.zeros((0, 3), F), np.zeros((0, 3), np.int32)), (ver, np.zeros((0, 3), np.int32)),
                 (np.zeros((0, 3), F), tri)):
        assert (_depth_abi(v, t, [cam]) == np.inf).all()


def _np_mesh(mesh):
    return tuple(mesh[k].cpu().numpy() for k in ("vertices", "normals", "triangles"))


def _bank(channels, sizes=None, eyes=EYES, images=None, seed=5):
    """Six cameras on the axes at distance 3 looking at the origin; frames of 48 x 40 and 40 x 48 (W x H) in turn."""
    rng = np.random.default_rng(seed)
    sizes = sizes or [(48, 40) if k % 2 == 0 else (40, 48) for k in range(len(eyes))]
    if images is None:
        images = [rng.integers(0, 256, size=(h, w, channels), dtype=np.uint8) for w, h in sizes]
    K = np.stack([_intrinsics(w, h) for w, h in sizes])
    return ImageBank(images, np.stack([_pose(e) for e in eyes]), K, 2.0, 6.0, device=DEV), images


@pytest.fixture(scope="module")
def ball():
    mesh = _ball_mesh()
    assert mesh["vertices"].shape[0] > 300 and mesh["triangles"].shape[0] > 600
    return mesh


def test_depth_of_the_ball_from_three_sides(ball):
    ver, _, tri = _np_mesh(ball)
    cams = [mref.camera(48, 40, 50, 50, 23.75, 19.5, _pose(e)) for e in EYES[:3]]
    got = _check_depth(ver, tri, cams, "ball").reshape(3, 40, 48)
    assert (np.abs(got[:, 20, 24] - 2.2) < 0.1).all() and (got[:, 0, 0] == np.inf).all()    # 3 - 0.8 at the centre
    # the Python forms: a free camera, and an image of a bank
    K = np.array([[50.0, 0, 23.75], [0, 50.0, 19.5], [0, 0, 1]])
    d = geometry.mesh_depth(ball, _pose(EYES[1]), K, 40, 48)
    assert d.shape == (40, 48) and d.dtype == torch.float32
    assert np.array_equal(d.cpu().numpy().view(np.uint32), got[1].view(np.uint32))
    d = geometry.mesh_depth(ball, torch.from_numpy(_pose(EYES[2])).to(DEV), torch.from_numpy(K).to(DEV), 40, 48)
    assert np.array_equal(d.cpu().numpy().view(np.uint32), got[2].view(np.uint32))
    bank, _ = _bank(3)
    d = geometry.mesh_depth(ball, bank=bank, image=3)
    exp = mref.depth_map(ver, tri, mref.cameras_of(bank.host_table)[3])
    assert d.shape == (48, 40) and np.array_equal(d.cpu().numpy().view(np.uint32), exp.view(np.uint32))
    with pytest.raises(ValueError):
        geometry.mesh_depth(ball, bank=bank, image=6)
    with pytest.raises(ValueError):
        geometry.mesh_depth(ball, _pose(EYES[1]), K, 40, 48, bank=bank, image=0)


def test_no_host_synchronisation_with_device_arguments(ball):
    """Both forms of mesh_depth, and color_mesh_from_images with its defaults and with device tensors, under torch's
    synchronisation check: a blocking copy or a read of a device value raises."""
    bank, _ = _bank(3)
    K = torch.tensor([[50.0, 0, 23.75], [0, 50.0, 19.5], [0, 0, 1]], device=DEV)
    c2w = torch.from_numpy(_pose(EYES[1])).float().to(DEV)
    weights = torch.ones(6, device=DEV)
    grey = torch.full((3,), 0.25, device=DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        free = geometry.mesh_depth(ball, c2w, K, 40, 48)
        banked = geometry.mesh_depth(ball, bank=bank, image=1)
        got = geometry.color_mesh_from_images(ball, bank, 0.1)
        again = geometry.color_mesh_from_images(ball, bank, 0.1, image_weights=weights, fallback=grey, reject=0.2,
                                                images=[0, 2, 3], batch_pixels=48 * 40)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert free.shape == (40, 48) and banked.shape == (48, 40) and torch.isfinite(free).any() and torch.isfinite(banked).any()
    assert got["seen"].any() and again["seen"].any()


# ---- blend -----------------------------------------------------------------------------------------------------------------

TOL = 0.1                      # of the ball's blend cases: below the lattice spacing 0.125, far below the ball's 1.6


@pytest.fixture(scope="module", params=[3, 4], ids=["rgb", "rgba"])
def blended(request, ball):
    """The ball, a six-camera bank and the restatement of its blend: computed once, shared, never written to."""
    bank, images = _bank(request.param)
    ver, nrm, tri = _np_mesh(ball)
    cams = mref.cameras_of(bank.host_table)
    depths = [mref.depth_map(ver, tri, c) for c in cams]
    sums, views = mref.blend(ver, nrm, cams, images, depths, TOL)
    for a in depths + [sums, views]:
        a.setflags(write=False)
    return dict(bank=bank, images=images, cams=cams, depths=depths, sums=sums, views=views, ver=ver, nrm=nrm, tri=tri)


def _blend_abi(b, V, runs, ball):
    """nfl_mesh_depth + nfl_mesh_blend over `runs` ([(first, count)]) for the first V vertices, accumulators framed by
    sentinel rows."""
    bank, lib = b["bank"], _lib.lib()
    d_ver, d_nrm = _dev(b["ver"][:V], F), _dev(b["nrm"][:V], F)
    sums = torch.full((V + 2, 4), SENTINEL, dtype=torch.float32, device=DEV)
    views = torch.full((V + 2,), -7, dtype=torch.int32, device=DEV)
    for k, (first, count) in enumerate(runs):
        n = int(sum(c["width"] * c["height"] for c in b["cams"][first:first + count]))
        depth = torch.empty(n, dtype=torch.float32, device=DEV)
        geometry.images._run_depth(ball["vertices"], ball["triangles"], bank.table, bank.n_images, first, count, depth)
        a = _lib.MeshBlendArgs()
        a.d_vertices, a.d_normals, a.n_vertices, a.d_pixels = d_ver.data_ptr(), d_nrm.data_ptr(), V, bank.pixels.data_ptr()
        a.d_table, a.n_images, a.first, a.count, a.weighting = bank.table.data_ptr(), bank.n_images, first, count, 0
        a.d_depth, a.n_depth, a.min_cos, a.depth_tol, a.start = depth.data_ptr(), n, 0.0, TOL, int(k == 0)
        a.d_sum, a.d_views = sums[1:].data_ptr(), views[1:].data_ptr()
        _lib.check(lib.nfl_mesh_blend(C.byref(a), _stream()), "nfl_mesh_blend")
    s, v = sums.cpu().numpy(), views.cpu().numpy()
    assert (s[0] == SENTINEL).all() and (s[-1] == SENTINEL).all() and v[0] == -7 and v[-1] == -7
    return s[1:-1], v[1:-1]


@pytest.mark.parametrize("V", [1, 63, 64, 65, None])
def test_blend_accumulators_equal_the_restatement(blended, ball, V):
    V = blended["ver"].shape[0] if V is None else V
    exp_s, exp_v = blended["sums"][:V], blended["views"][:V]
    for runs in ([(k, 1) for k in range(6)], [(0, 4), (4, 2)], [(0, 6)]):
        s, v = _blend_abi(blended, V, runs, ball)
        assert np.array_equal(v, exp_v), runs
        assert np.array_equal(s.view(np.uint32), exp_s.view(np.uint32)), (runs, np.abs(s - exp_s).max())
    if V > 65:
        assert 0 < (exp_v > 0).sum() and exp_v.max() >= 2


def test_color_mesh_from_images_equals_the_restatement(blended, ball):
    b = blended
    exp_c = mref.colors_of(b["sums"], b["views"], (0.25, 0.5, 0.75))
    for batch in (1 << 26, 48 * 40 + 40 * 48, 1):                    # one run, runs of two, runs of one
        got = geometry.color_mesh_from_images(ball, b["bank"], TOL, fallback=(0.25, 0.5, 0.75), batch_pixels=batch)
        assert got["colors"].dtype == torch.float32 and got["views"].dtype == torch.int32 and got["seen"].dtype == torch.bool
        assert np.array_equal(got["views"].cpu().numpy(), b["views"])
        assert np.array_equal(got["seen"].cpu().numpy(), b["views"] > 0)
        assert np.array_equal(got["weight"].cpu().numpy().view(np.uint32), b["sums"][:, 3].view(np.uint32))
        assert np.array_equal(got["colors"].cpu().numpy().view(np.uint32), exp_c.view(np.uint32))
    c = got["colors"].cpu().numpy()
    assert c.min() >= 0.0 and c.max() <= 1.0
    # a selection, weights, uniform weighting and a stricter angle: the restatement over the same images
    sel, w = [1, 2, 4], np.array([9.0, 0.5, 2.0, 9.0, 0.0, 9.0], dtype=F)
    pick = lambda xs: [xs[i] for i in sel]
    s, v = mref.blend(b["ver"], b["nrm"], pick(b["cams"]), pick(b["images"]), pick(b["depths"]), TOL, image_weights=w[sel],
                      min_cos=0.3, weighting="uniform")
    got = geometry.color_mesh_from_images(ball, b["bank"], TOL, images=sel, image_weights=w, min_cos=0.3, weighting="uniform")
    assert np.array_equal(got["views"].cpu().numpy(), v)
    assert np.array_equal(got["weight"].cpu().numpy().view(np.uint32), s[:, 3].view(np.uint32))
    assert np.array_equal(got["colors"].cpu().numpy().view(np.uint32), mref.colors_of(s, v).view(np.uint32))
    # reject: the second pass centred on the first one's colours
    c1 = mref.colors_of(b["sums"], b["views"])
    s2, v2 = mref.blend(b["ver"], b["nrm"], b["cams"], b["images"], b["depths"], TOL, center=c1, reject=0.2)
    for batch in (1 << 26, 48 * 40):                                 # depth maps kept, and rasterised again
        got = geometry.color_mesh_from_images(ball, b["bank"], TOL, reject=0.2, batch_pixels=batch)
        assert np.array_equal(got["views"].cpu().numpy(), v2)
        # a vertex all of whose samples were rejected keeps the first pass's colour
        assert np.array_equal(got["colors"].cpu().numpy().view(np.uint32), mref.colors_of(s2, v2, c1).view(np.uint32))
        assert np.array_equal(got["seen"].cpu().numpy(), v2 > 0)
    assert (v2 <= b["views"]).all() and (v2 < b["views"]).any()
    # two views that disagree by more than 2 r: both rejected against their mean, the mean stays
    far = ((b["views"] == 2) & (v2 == 0))
    print(f"reject: {int(far.sum())} vertices lost all their samples in the second pass")
    for bad in (dict(weighting="sin"), dict(min_cos=-0.1), dict(reject=-1.0), dict(images=[6]), dict(batch_pixels=0),
                dict(image_weights=[1.0]), dict(fallback=(1.0, 2.0))):
        with pytest.raises(ValueError):
            geometry.color_mesh_from_images(ball, b["bank"], TOL, **bad)
    with pytest.raises(ValueError):
        geometry.color_mesh_from_images(ball, b["bank"], -0.5)


# ---- properties that need no restatement -----------------------------------------------------------------------------------

def _flat(color, w=48, h=40):
    return np.broadcast_to(np.array(color, dtype=np.uint8), (h, w, 3)).copy()


def test_flat_colour_bank_gives_that_colour(ball):
    """Every seen vertex holds c to 1e-6: a ratio of sums of the same weights, three fp32 roundings."""
    col = (51, 153, 204)
    bank, _ = _bank(3, images=[_flat(col, *s) for s in [(48, 40), (40, 48)] * 3])
    got = geometry.color_mesh_from_images(ball, bank, TOL)
    seen = got["seen"].cpu().numpy()
    assert seen.mean() > 0.9
    assert np.abs(got["colors"].cpu().numpy()[seen] - np.array(col) / 255.0).max() <= 1e-6
    assert (got["colors"][~got["seen"]] == 0.5).all()


def test_inner_shell_is_hidden_by_the_outer_one():
    outer, inner = _ball_mesh(0.8), _ball_mesh(0.4)
    Vo = outer["vertices"].shape[0]
    both = {"vertices": torch.cat([outer["vertices"], inner["vertices"]]), "normals": torch.cat([outer["normals"], inner["normals"]]),
            "triangles": torch.cat([outer["triangles"], inner["triangles"] + Vo])}
    bank, _ = _bank(3)
    seen = geometry.color_mesh_from_images(both, bank, 0.05)["seen"]
    assert not seen[Vo:].any() and seen[:Vo].float().mean() > 0.5
    assert geometry.color_mesh_from_images(both, bank, 1e9)["seen"].all()


def test_reject_removes_the_odd_image():
    """Three cameras share a pose on each of two sides (so that whatever the odd image sees, two others see too, with the
    same weights); one of the six shows another colour.  The first pass puts a vertex it sees a third of the way towards
    that colour, 0.25 / 3 on the largest channel: inside reject = 0.1 for the two good samples, outside it for the odd one."""
    mesh = _ball_mesh()
    c, odd = (204, 102, 51), (140, 102, 51)                          # 64 / 255 = 0.251 apart
    images = [_flat(c) for _ in range(6)]
    images[2] = _flat(odd)
    bank, _ = _bank(3, sizes=[(48, 40)] * 6, eyes=[EYES[0]] * 3 + [EYES[3]] * 3, images=images)
    sees = geometry.color_mesh_from_images(mesh, bank, TOL, images=[2])["seen"].cpu().numpy()
    assert sees.sum() > 50
    target = np.array(c) / 255.0
    first = geometry.color_mesh_from_images(mesh, bank, TOL)
    plain = first["colors"].cpu().numpy()
    assert (np.abs(plain[sees] - target).max(axis=1) > 0.03).all()
    got = geometry.color_mesh_from_images(mesh, bank, TOL, reject=0.1)
    assert np.array_equal(got["views"].cpu().numpy()[sees], first["views"].cpu().numpy()[sees] - 1)
    assert np.abs(got["colors"].cpu().numpy()[sees] - target).max() <= 1e-6


# ---- extract_mesh ----------------------------------------------------------------------------------------------------------

def test_extract_mesh_with_and_without_images():
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(DEV)
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (17, 17, 17)
    bank, _ = _bank(3)
    with torch.no_grad():
        iso = geometry.density_lattice(model, emb, lo, hi, res).median().item()
        plain = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso)
        field = geometry.surface_colors(model, emb, plain["vertices"], plain["normals"])
        assert "seen" not in plain and torch.equal(plain["colors"], field)          # the default path is untouched
        mesh = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, color_from=bank)
        assert torch.equal(mesh["vertices"], plain["vertices"]) and torch.equal(mesh["triangles"], plain["triangles"])
        exp = geometry.color_mesh_from_images(mesh, bank, 2.0 * 2.0 / 16, fallback=field)
        seen = exp["seen"]
        assert seen.any() and torch.equal(mesh["seen"], seen)
        assert torch.equal(mesh["colors"], exp["colors"])
        assert torch.equal(mesh["colors"][~seen], field[~seen])
        grey = geometry.color_mesh_from_images(mesh, bank, 0.25)["colors"]
        assert torch.equal(mesh["colors"][seen], grey[seen])
        tight = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, color_from=bank, depth_tol=0.01,
                                      color_kwargs=dict(weighting="uniform", images=[0, 1]))
        exp = geometry.color_mesh_from_images(tight, bank, 0.01, weighting="uniform", images=[0, 1], fallback=field)
        assert torch.equal(tight["colors"], exp["colors"])
