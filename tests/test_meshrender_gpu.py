"""GPU checks of mesh render: the visibility and shade kernels (csrc/nfl_meshrender.hip) against the numpy restatement of
tests/meshrender_ref.py, through the C ABI and through geometry.mesh_visibility / render_mesh, eval.render_mesh_video and
eval.evaluate_mesh.

Both sides evaluate the same fp32 formulae with every operation rounded on its own (the library is built with
-ffp-contract=off; division and square root are correctly rounded on both), so EVERYTHING is held to equality: every word,
float colour, byte, depth and triangle index, in all three modes.  The restatement brute-forces every triangle against
every pixel, so the equality also shows that the raster's boxes (and its wave path for boxes above 64 pixels) lose no hit
and that ties fall to the lower index whatever the order of the atomics.

The shapes are the smallest that cross the boundaries of the code: 1 / 63 / 64 / 65 / 257 triangles for the waves and the
256-thread workgroups, frames of 1 x 1 up to 65 x 33, boxes below and above 64 pixels, a run whose first image is one
pixel.  The restatement of a case is computed once and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshcolor_ref as mref
import meshrender_ref as rref
from geom_gpu_util import (ball_mesh as _ball_mesh, dev as _dev, EYES, F, field_bits as _bits, frame as _frame,
                           framed as _framed, intrinsics as _intrinsics, PAD, pose as _pose, ptr as _ptr,
                           same_fields as _same, stream as _stream, unframe as _unframe)
from gpu_util import DEV
from nerf_fl_amd import _lib, eval as nfl_eval, geometry, metrics
from nerf_fl_amd.data import ImageBank

pytestmark = pytest.mark.gpu

S_WORD, S_F, S_I, S_B = 0x0123456789ABCDEF, -7.0, -7, 0xAB
BG = (0.25, 0.5, 0.75)
KEYS = ("rgb", "rgb_u8", "depth", "triangle")


def _abi(ver, tri, cams, mode="color", attr=None, first=0, count=None, outputs=KEYS, background=BG, words=None):
    """nfl_mesh_visibility (unless `words` are given) and nfl_mesh_shade of cams[first : first + count], every buffer framed
    by sentinels; the visibility runs twice and must give the same bits."""
    lib = _lib.lib()
    count = len(cams) - first if count is None else count
    table = mref.table_of(cams)
    n = int(sum(c["width"] * c["height"] for c in cams[first:first + count]))
    d_ver, d_tri = _dev(np.reshape(ver, (-1, 3)), F), _dev(np.reshape(tri, (-1, 3)), np.int32)
    d_attr = None if attr is None else _dev(np.reshape(attr, (-1, 3)), F)
    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    got = {}
    if words is None:
        runs = []
        for _ in range(2):
            vis = _framed(n, (), S_WORD, torch.int64)
            a = _lib.MeshVisibilityArgs()
            a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(d_ver), _ptr(d_tri), d_ver.shape[0], d_tri.shape[0]
            a.d_table, a.n_images, a.first, a.count = d_table.data_ptr(), len(cams), first, count
            a.d_vis, a.n_vis = vis[PAD:].data_ptr(), n
            _lib.check(lib.nfl_mesh_visibility(C.byref(a), _stream()), "nfl_mesh_visibility")
            runs.append(_unframe(vis, n, S_WORD, "words").view(np.uint64))
        assert np.array_equal(runs[0], runs[1])
        got["words"] = runs[0]
    else:
        vis = _framed(n, (), S_WORD, torch.int64)
        vis[PAD:PAD + n] = torch.from_numpy(np.asarray(words, dtype=np.uint64).view(np.int64).copy()).to(DEV)
    bufs = {"rgb": _framed(n, (3,), S_F, torch.float32), "rgb_u8": _framed(n, (3,), S_B, torch.uint8),
            "depth": _framed(n, (), S_F, torch.float32), "triangle": _framed(n, (), S_I, torch.int32)}
    s = _lib.MeshShadeArgs()
    s.d_vertices, s.d_triangles, s.n_vertices, s.n_triangles = _ptr(d_ver), _ptr(d_tri), d_ver.shape[0], d_tri.shape[0]
    s.d_table, s.n_images, s.first, s.count, s.mode = d_table.data_ptr(), len(cams), first, count, _lib.SHADE_MODES[mode]
    s.d_vis, s.n_vis, s.d_attr = vis[PAD:].data_ptr(), n, _ptr(d_attr)
    s.background[:] = background
    s.d_rgb, s.d_rgb_u8, s.d_depth, s.d_triangle = (bufs[k][PAD:].data_ptr() if k in outputs else None for k in KEYS)
    _lib.check(lib.nfl_mesh_shade(C.byref(s), _stream()), "nfl_mesh_shade")
    for k, sentinel in zip(KEYS, (S_F, S_B, S_F, S_I)):
        h = _unframe(bufs[k], n, sentinel, k)
        if k in outputs:
            got[k] = h
        else:
            assert (h == sentinel).all(), k                          # a NULL output is skipped, and nothing else lands there
    return got


def _attrs(ver, seed=11):
    rng = np.random.default_rng(seed)
    V = np.reshape(ver, (-1, 3)).shape[0]
    return {"color": rng.uniform(-0.2, 1.2, size=(V, 3)).astype(F), "normal": rng.normal(size=(V, 3)).astype(F), "facing": None}


def _check(ver, tri, cams, what, modes=rref.MODES):
    """All three modes against the restatement, bit for bit; returns the restatement of the last mode."""
    attrs = _attrs(ver)
    for mode in modes:
        exp = rref.run_render(ver, tri, cams, mode, attrs[mode], BG)
        _same(_abi(ver, tri, cams, mode, attrs[mode]), exp, (what, mode))
    return exp


# ---- the kernels against the restatement ---------------------------------------------------------------------------------

@pytest.mark.parametrize("T", [1, 63, 64, 65, 257])
def test_soup_triangle_counts(T):
    ver, tri = mref.soup(400, 7)
    exp = _check(ver, tri[:T], [_frame(65, 33)], f"T={T}")
    assert (exp["triangle"] >= 0).any() or T == 1


@pytest.mark.parametrize("size", [(1, 1), (63, 5), (64, 64), (65, 33)])
def test_soup_frame_sizes(size):
    ver, tri = mref.soup(400, 7)
    exp = _check(ver, tri[:257], [_frame(*size)], f"frame {size}")
    assert exp["words"].shape == (size[0] * size[1],)


def test_run_of_three_cameras_of_different_sizes():
    """The binary search of pix0: a first image of ONE pixel, then 65 x 33 and 20 x 31; and a run inside a table."""
    ver, tri = mref.soup(400, 7)
    cams = [mref.camera(1, 1, 4, 4, 0, 0),
            mref.camera(65, 33, 40, 40, 32.25, 16.5),
            mref.camera(20, 31, 15, 18, 9.5, 15, mref.look_at((4.0, 0.0, -4.0), (0, 0, -4))),
            mref.camera(33, 17, 20, 20, 16, 8, mref.look_at((0.5, 0.2, 1.0), (0, 0, -4)))]
    attrs = _attrs(ver)
    exp = rref.run_render(ver, tri[:257], cams[:3], "color", attrs["color"], BG)
    _same(_abi(ver, tri[:257], cams[:3], "color", attrs["color"]), exp, "three cameras")
    assert exp["triangle"][0] >= 0 and all((exp["triangle"][s] >= 0).any() for s in (slice(1, 1 + 65 * 33), slice(1 + 65 * 33, None)))
    # a run inside the table: the words are numbered from the run's first image
    full = rref.run_render(ver, tri[:257], cams, "normal", attrs["normal"], BG)
    mid = _abi(ver, tri[:257], cams, "normal", attrs["normal"], first=1, count=2)
    _same(mid, {k: v[1:-33 * 17] for k, v in full.items()}, "run inside the table")


def test_large_and_small_boxes_in_one_launch():
    """A triangle over the whole 65 x 33 frame (a box of 2145 pixels: the wave path) behind a small soup, and in front of it."""
    cam = _frame(65, 33)
    ver, tri = mref.soup(400, 7)
    for z, what in ((-9.0, "behind"), (-0.5, "in front")):
        s = -z / 5.0
        big = np.array([[-9 * s, -5 * s, z], [9 * s, -5 * s, z], [0, 9 * s, z]], dtype=F)
        v = np.concatenate([ver[:3 * 65], big])
        t = np.concatenate([tri[:65], [[195, 196, 197]]]).astype(np.int32)
        exp = _check(v, t, [cam, _frame(64, 64)], what)
        assert (exp["triangle"][:65 * 33] >= 0).all()                # it fills the first frame
        share = (exp["triangle"][:65 * 33] == 65).mean()
        assert (share == 1.0) if z > -2 else (0.0 < share < 1.0), share


def test_salted_soup():
    """NaN and inf vertices, indices out of range, a degenerate, a behind, a straddling and an edge-on triangle: refused by
    the range and finiteness checks or missed by the ray test, and the others keep their numbers."""
    ver, tri = mref.soup(400, 7)
    ver, tri = ver[:3 * 130].copy(), tri[:130].copy()
    ver[3 * 5 + 1, 0] = np.nan
    ver[3 * 6] = [np.inf, 0, -3]
    ver[3 * 9 + 2] = ver[3 * 9 + 1]
    ver[3 * 12:3 * 12 + 3, 2] *= -1
    ver[3 * 70:3 * 70 + 3] = [[-1, -1, -3], [1, -1, -3], [0.3, 1, 1.5]]
    ver[3 * 71:3 * 71 + 3] = [[0, -1, -3], [0, 1, -3], [0, 0, -5]]
    tri[100] = [3, 4, 3 * 130]
    tri[101] = [-1, 4, 5]
    for cam in (_frame(65, 33), mref.camera(65, 33, 40, 40, 32, 16)):
        exp = _check(ver, tri, [cam], "salted")
        seen = set(np.unique(exp["triangle"]).tolist())
        assert 70 in seen and not seen & {5, 6, 9, 12, 100, 101}


def test_duplicated_triangles_fall_to_the_lower_index():
    ver, tri = mref.soup(400, 7)
    tri = np.concatenate([tri[:100], tri[:100][::-1], tri[:100]]).astype(np.int32)      # 100 + k and 299 - k repeat k
    exp = _check(ver, tri, [_frame(65, 33)], "duplicates", modes=("color",))
    assert exp["triangle"].max() < 100 and (exp["triangle"] >= 0).mean() > 0.1


def test_empty_mesh():
    cam = _frame(63, 5)
    ver, tri = mref.soup(4, 7)
    for v, t in ((np.zeros((0, 3), F), np.zeros((0, 3), np.int32)), (ver, np.zeros((0, 3), np.int32)),
                 (np.zeros((0, 3), F), tri)):
        got = _abi(v, t, [cam], "facing")
        assert (got["words"] == rref.EMPTY).all() and (got["triangle"] == -1).all() and (got["depth"] == np.inf).all()
        assert (got["rgb"] == np.array(BG, dtype=F)).all() and (got["rgb_u8"] == np.array([63, 127, 191], dtype=np.uint8)).all()


def test_shade_depth_is_bit_equal_to_mesh_depth():
    ver, tri = mref.soup(400, 7)
    cams = [_frame(65, 33), _frame(64, 64)]
    got = _abi(ver, tri[:257], cams, "facing")
    table = mref.table_of(cams)
    d_table = torch.from_numpy(table.view(np.uint8).reshape(-1).copy()).to(DEV)
    n = 65 * 33 + 64 * 64
    depth = torch.empty(n, dtype=torch.float32, device=DEV)
    geometry.images._run_depth(_dev(ver, F), _dev(tri[:257], np.int32), d_table, 2, 0, 2, depth)
    d = depth.cpu().numpy()
    assert np.array_equal(got["depth"].view(np.uint32), d.view(np.uint32))
    assert np.array_equal((got["words"] >> np.uint64(32)).astype(np.uint32)[np.isfinite(d)], d.view(np.uint32)[np.isfinite(d)])


def test_the_two_rasters_agree_word_for_word():
    """One walk for both rasters: on a run of two 65 x 33 images of the 65-triangle soup with a triangle across the frame
    that straddles the camera plane (the whole frame is its box: the wave path), nfl_mesh_depth gives +inf exactly where
    the visibility word is -1, and everywhere else the bits of the word's high half."""
    ver, tri = mref.soup(400, 7)
    ver = np.concatenate([ver[:3 * 65], np.array([[-40, 2, -12], [40, 2, -12], [0, -3, 1.5]], dtype=F)])
    tri = np.concatenate([tri[:65], [[195, 196, 197]]])
    cams = [_frame(65, 33), mref.camera(65, 33, 40, 40, 32, 16)]
    d_table = torch.from_numpy(mref.table_of(cams).view(np.uint8).reshape(-1).copy()).to(DEV)
    n = 2 * 65 * 33
    vis = torch.empty(n, dtype=torch.int64, device=DEV)
    depth = torch.empty(n, dtype=torch.float32, device=DEV)
    geometry.images._run_visibility(_dev(ver, F), _dev(tri, np.int32), d_table, 2, 0, 2, vis)
    geometry.images._run_depth(_dev(ver, F), _dev(tri, np.int32), d_table, 2, 0, 2, depth)
    empty = vis == -1
    assert torch.equal(depth[empty], torch.full_like(depth[empty], float("inf")))
    assert torch.equal((vis[~empty] >> 32).to(torch.int32), depth[~empty].view(torch.int32))
    winner = vis[~empty] & 0xFFFFFFFF
    assert 0.1 < empty.float().mean() < 0.5 and 0.5 < (winner == 65).float().mean() < 0.9 and winner.unique().numel() > 40


def test_null_outputs_are_skipped_and_untrusted_words_are_uncovered():
    ver, tri = mref.soup(400, 7)
    cam = _frame(65, 33)
    attrs = _attrs(ver)
    exp = rref.run_render(ver, tri[:65], [cam], "color", attrs["color"], BG)
    for outputs in (("rgb",), ("rgb_u8", "triangle"), ("depth",), ()):
        _same(_abi(ver, tri[:65], [cam], "color", attrs["color"], outputs=outputs), exp, outputs)
    # words that no raster wrote: a triangle number >= T, the largest 32-bit number, a triangle with an index out of range
    words = exp["words"].copy()
    words[::3] = (words[::3] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(65)
    words[1::7] = (words[1::7] & np.uint64(0xFFFFFFFF00000000)) | np.uint64(0xFFFFFFFE)
    t = tri[:65].copy()
    t[7] = [3, 4, 400 * 3]
    words[2::5] = (np.uint64(0x40400000) << np.uint64(32)) | np.uint64(7)
    want = rref.shade(ver, t, cam, words, "color", attrs["color"], BG)
    got = _abi(ver, t, [cam], "color", attrs["color"], words=words)
    _same(got, {k: want[k] for k in KEYS}, "untrusted words")
    assert (got["triangle"][::3] == -1).all() and (got["triangle"][2::5] == -1).all()


# ---- the ball of test_meshcolor_gpu.py, its cameras and its banks -------------------------------------------------------

SIZES = [(48, 40) if k % 2 == 0 else (40, 48) for k in range(6)]


def _bank(images, sizes=SIZES):
    """Six cameras on the axes at distance 3 looking at the origin, as test_meshcolor_gpu.py makes its banks."""
    K = np.stack([_intrinsics(w, h) for w, h in sizes])
    return ImageBank(images, np.stack([_pose(e) for e in EYES]), K, 2.0, 6.0, device=DEV)


def _affine_colors(ver):
    """Affine in position, mapped into [0.1, 0.9]: the ball lies in [-1, 1]^3."""
    return (0.1 + 0.8 * (ver + 1.0) / 2.0).clamp(0.1, 0.9).contiguous()


@pytest.fixture(scope="module")
def ball():
    """The 17-ring ball with colours, and banks rendered from it (black and white backgrounds): made once, never written to."""
    mesh = _ball_mesh()
    mesh["colors"] = _affine_colors(mesh["vertices"])
    assert mesh["vertices"].shape[0] > 300 and mesh["triangles"].shape[0] > 600
    first = {bg: [geometry.render_mesh(mesh, _pose(e), _intrinsics(w, h), h, w, background=(bg,) * 3) for e, (w, h) in zip(EYES, SIZES)]
             for bg in (0.0, 1.0)}
    banks = {bg: _bank([r["rgb"].cpu().numpy() for r in first[bg]]) for bg in first}
    ver, nrm, col, tri = (mesh[k].cpu().numpy() for k in ("vertices", "normals", "colors", "triangles"))
    return dict(mesh=mesh, first=first, banks=banks, ver=ver, nrm=nrm, col=col, tri=tri,
                cams=mref.cameras_of(banks[0.0].host_table))


def test_render_mesh_forms_equal_the_restatement(ball):
    b = ball
    for k in (0, 1):
        w, h = SIZES[k]
        exp = rref.render(b["ver"], b["tri"], b["cams"][k], "color", b["col"], (0.0,) * 3)
        free = b["first"][0.0][k]
        banked = geometry.render_mesh(b["mesh"], bank=b["banks"][0.0], image=k, background=(0.0, 0.0, 0.0))
        for r in (free, banked):
            assert r["rgb"].shape == (h, w, 3) and r["rgb"].dtype == torch.uint8 and r["rgb_float"].shape == (h * w, 3)
            assert r["depth"].shape == (h, w) and r["triangle"].dtype == torch.int32 and r["covered"].dtype == torch.bool
            assert np.array_equal(r["rgb"].cpu().numpy().reshape(-1, 3), exp["rgb_u8"])
            assert np.array_equal(_bits(r["rgb_float"].cpu().numpy()), _bits(exp["rgb"]))
            assert np.array_equal(_bits(r["depth"].cpu().numpy().reshape(-1)), _bits(exp["depth"]))
            assert np.array_equal(r["triangle"].cpu().numpy().reshape(-1), exp["triangle"])
            assert np.array_equal(r["covered"].cpu().numpy().reshape(-1), exp["triangle"] >= 0)
        vis = geometry.mesh_visibility(b["mesh"], bank=b["banks"][0.0], image=k)
        assert vis.shape == (h, w) and vis.dtype == torch.int64
        assert np.array_equal(vis.cpu().numpy().reshape(-1).view(np.uint64), exp["words"])
        assert torch.equal(geometry.mesh_depth(b["mesh"], bank=b["banks"][0.0], image=k), banked["depth"])
    assert 0.3 < (exp["triangle"] >= 0).mean() < 0.9
    # the other modes and explicit colours through the Python layer
    cam = b["cams"][2]
    for shade, attr in (("normal", b["nrm"]), ("facing", None)):
        r = geometry.render_mesh(b["mesh"], bank=b["banks"][0.0], image=2, shade=shade)
        exp = rref.render(b["ver"], b["tri"], cam, shade, attr, (1.0, 1.0, 1.0))
        assert np.array_equal(_bits(r["rgb_float"].cpu().numpy()), _bits(exp["rgb"]))
        assert np.array_equal(r["rgb"].cpu().numpy().reshape(-1, 3), exp["rgb_u8"])
    other = torch.flip(b["mesh"]["colors"], dims=(1,)).contiguous()
    r = geometry.render_mesh(b["mesh"], bank=b["banks"][0.0], image=2, colors=other)
    exp = rref.render(b["ver"], b["tri"], cam, "color", b["col"][:, ::-1], (1.0, 1.0, 1.0))
    assert np.array_equal(_bits(r["rgb_float"].cpu().numpy()), _bits(exp["rgb"]))
    bare = {k: b["mesh"][k] for k in ("vertices", "normals", "triangles")}
    assert geometry.render_mesh(bare, bank=b["banks"][0.0], image=2, shade="facing")["covered"].any()
    for bad in (dict(), dict(shade="flat"), dict(colors=other[:5]), dict(colors=other, background=(1.0, 2.0))):
        with pytest.raises(ValueError):
            geometry.render_mesh(bare, bank=b["banks"][0.0], image=2, **bad)
    with pytest.raises(ValueError):
        geometry.render_mesh(b["mesh"], _pose(EYES[0]), _intrinsics(48, 40), 40, 48, bank=b["banks"][0.0], image=0)
    with pytest.raises(ValueError):
        geometry.mesh_visibility(b["mesh"], bank=b["banks"][0.0], image=6)


def test_runs_of_1_4_plus_2_and_6_images_give_the_same_bits(ball):
    b = ball
    exp = rref.run_render(b["ver"], b["tri"], b["cams"], "color", b["col"], BG)
    sizes = [w * h for w, h in SIZES]
    for runs in ([(k, 1) for k in range(6)], [(0, 4), (4, 2)], [(0, 6)]):
        parts = [_abi(b["ver"], b["tri"], b["cams"], "color", b["col"], first=f, count=c) for f, c in runs]
        got = {k: np.concatenate([p[k] for p in parts]) for k in exp}
        assert got["words"].shape == (sum(sizes),)
        _same(got, exp, runs)


def test_no_host_synchronisation_with_device_arguments(ball):
    """render_mesh in both camera forms, mesh_visibility and render_mesh_video under torch's synchronisation check: a
    blocking copy or a read of a device value raises."""
    mesh, bank = ball["mesh"], ball["banks"][0.0]
    K = torch.from_numpy(_intrinsics(48, 40)).float().to(DEV)
    poses = torch.from_numpy(np.stack([_pose(e) for e in EYES[:3]])).float().to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        free = geometry.render_mesh(mesh, poses[1], K, 40, 48)
        banked = geometry.render_mesh(mesh, bank=bank, image=1, shade="normal", background=(0.0, 0.0, 0.0))
        vis_free = geometry.mesh_visibility(mesh, poses[2], K, 40, 48)
        vis_bank = geometry.mesh_visibility(mesh, bank=bank, image=3)
        first, frames = nfl_eval.render_mesh_video(mesh, poses, K, 40, 48, shade="facing")
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert free["rgb"].shape == (40, 48, 3) and banked["rgb"].shape == (48, 40, 3) and free["covered"].any() and banked["covered"].any()
    assert vis_free.shape == (40, 48) and vis_bank.shape == (48, 40) and (vis_free != -1).any() and (vis_bank != -1).any()
    assert first == 0 and frames.shape == (3, 40, 48, 3)


def test_render_mesh_video_shards_equal_the_frames_one_by_one(ball):
    mesh = ball["mesh"]
    K = _intrinsics(48, 40)
    poses = np.stack([_pose(e) for e in EYES[:5]])
    single = [geometry.render_mesh(mesh, p, K, 40, 48, background=BG)["rgb"] for p in poses]
    for rank, world in ((0, 1), (0, 2), (1, 2)):
        first, frames = nfl_eval.render_mesh_video(mesh, poses, K, 40, 48, rank=rank, world=world, background=BG)
        lo, hi = nfl_eval.parallel.shard_bounds(5, rank, world)
        assert first == lo and frames.shape == (hi - lo, 40, 48, 3) and frames.dtype == torch.uint8
        assert all(torch.equal(frames[k - lo], single[k]) for k in range(lo, hi))
    first, frames = nfl_eval.render_mesh_video(mesh, poses[:1], K, 40, 48, rank=1, world=2)
    assert frames.shape == (0, 40, 48, 3)


# ---- evaluate_mesh ----------------------------------------------------------------------------------------------------------

def test_evaluate_mesh_on_a_bank_rendered_from_the_mesh_itself(ball, monkeypatch):
    """Every image scores an error of exactly zero; ONE device-to-host copy, everything before it under the sync check."""
    mesh, bank = ball["mesh"], ball["banks"][0.0]
    copies = []
    real_cpu = torch.Tensor.cpu

    def counted_cpu(self, *args, **kwargs):
        copies.append(tuple(self.shape))
        torch.cuda.set_sync_debug_mode("default")
        try:
            return real_cpu(self, *args, **kwargs)
        finally:
            torch.cuda.set_sync_debug_mode("error")

    monkeypatch.setattr(torch.Tensor, "cpu", counted_cpu)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        res = nfl_eval.evaluate_mesh(mesh, bank, return_images=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.undo()
    assert copies == [(6, 8)]
    table = res["table"].cpu().numpy()
    col = {name: table[:, j] for j, name in enumerate(metrics.METRIC_COLUMNS)}
    assert (col["sse_valid"] == 0).all() and (col["sse"] == 0).all() and (col["count_valid"] > 0).all()
    assert np.isposinf(res["psnr_valid"].numpy()).all() and np.isposinf(res["psnr"].numpy()).all()
    assert res["ssim"].numpy() == pytest.approx(1.0, abs=1e-6)
    assert res["first"] == 0 and res["count"] == 6 and np.isposinf(res["mean_psnr_valid"])
    covered = [int(r["covered"].sum()) for r in ball["first"][0.0]]
    assert col["count_valid"].tolist() == [3 * c for c in covered]
    assert all(torch.equal(f, r["rgb"]) for f, r in zip(res["frames"], ball["first"][0.0]))
    # the white bank against the default (black: the bank is RGB) background: the covered pixels still score zero
    res = nfl_eval.evaluate_mesh(mesh, ball["banks"][1.0])
    assert np.isposinf(res["psnr_valid"].numpy()).all() and np.isfinite(res["psnr"].numpy()).all()
    assert np.isposinf(nfl_eval.evaluate_mesh(mesh, ball["banks"][1.0], background=(1.0, 1.0, 1.0))["psnr"].numpy()).all()


def test_evaluate_mesh_one_vertex_changed_and_two_ranks(ball):
    mesh, bank = ball["mesh"], ball["banks"][0.0]
    tri = ball["tri"]
    # the vertex furthest along +x: camera 0 sees it head-on, camera 3 (at -x) cannot
    v = int(np.argmax(ball["ver"][:, 0]))
    colors = mesh["colors"].clone()
    colors[v] = torch.tensor([0.9, 0.1, 0.9], device=DEV)
    assert (colors[v] - mesh["colors"][v]).abs().max() > 0.3
    res = nfl_eval.evaluate_mesh(mesh, bank, colors=colors)
    names = tri[(tri == v).any(axis=1)]
    assert len(names) >= 3
    changed, sees = [], []
    for k in range(6):
        again = geometry.render_mesh(mesh, bank=bank, image=k, colors=colors, background=(0.0, 0.0, 0.0))
        changed.append(not torch.equal(again["rgb"], ball["first"][0.0][k]["rgb"]))
        won = np.unique(again["triangle"].cpu().numpy())
        sees.append(bool(np.isin(won[won >= 0], np.nonzero((tri == v).any(axis=1))[0]).any()))
    assert changed[0] and not changed[3] and 1 <= sum(changed) < 6
    assert all(s or not c for s, c in zip(sees, changed))            # an image that changed sees the vertex
    psnr_valid = res["psnr_valid"].numpy()
    assert np.array_equal(np.isfinite(psnr_valid), np.array(changed)) and np.isposinf(psnr_valid[~np.array(changed)]).all()
    # two ranks: the tables sum to the single-rank table; a selection keeps its order
    halves = [nfl_eval.evaluate_mesh(mesh, bank, colors=colors, rank=r, world=2) for r in (0, 1)]
    assert halves[0]["first"] == 0 and halves[0]["count"] == 3 and halves[1]["first"] == 3
    assert torch.equal(halves[0]["table"] + halves[1]["table"], res["table"])
    assert (halves[0]["table"][3:] == 0).all() and (halves[1]["table"][:3] == 0).all()
    sel = nfl_eval.evaluate_mesh(mesh, bank, colors=colors, images=[4, 0])
    assert torch.equal(sel["table"], res["table"][[4, 0]])
    with pytest.raises(ValueError):
        nfl_eval.evaluate_mesh(mesh, bank, images=[6])


# ---- the closed loop: mesh -> images -> colours -> images -------------------------------------------------------------------

def test_closed_loop_equals_the_restatement_of_the_same_loop():
    """render_mesh, a uint8 bank, color_mesh_from_images(depth_tol = 0.05), render_mesh again: the second renders are
    bit-equal to meshrender_ref + meshcolor_ref.blend walking the same loop.  The loop's PSNR over the covered pixels is a
    property of the method (quantisation to bytes, bilinear sampling, the blend of six views) and is printed, not bounded."""
    mesh = _ball_mesh()
    mesh["colors"] = _affine_colors(mesh["vertices"])
    sizes = [(48, 40)] * 6
    first = [geometry.render_mesh(mesh, _pose(e), _intrinsics(48, 40), 40, 48) for e in EYES]
    bank = _bank([r["rgb"].cpu().numpy() for r in first], sizes)
    got = geometry.color_mesh_from_images(mesh, bank, 0.05)
    second = [geometry.render_mesh(mesh, bank=bank, image=k, colors=got["colors"]) for k in range(6)]
    # the same loop in numpy
    ver, nrm, col, tri = (mesh[k].cpu().numpy() for k in ("vertices", "normals", "colors", "triangles"))
    cams = mref.cameras_of(bank.host_table)
    r1 = [rref.render(ver, tri, c, "color", col) for c in cams]
    images = [r["rgb_u8"].reshape(40, 48, 3) for r in r1]
    for k in range(6):
        assert np.array_equal(first[k]["rgb"].cpu().numpy(), images[k]), k
    depths = [mref.depth_map(ver, tri, c) for c in cams]
    sums, views = mref.blend(ver, nrm, cams, images, depths, 0.05)
    col2 = mref.colors_of(sums, views)
    assert np.array_equal(_bits(got["colors"].cpu().numpy()), _bits(col2)) and np.array_equal(got["views"].cpu().numpy(), views)
    se = n = 0.0
    for k in range(6):
        exp = rref.render(ver, tri, cams[k], "color", col2)
        r = second[k]
        assert np.array_equal(_bits(r["rgb_float"].cpu().numpy()), _bits(exp["rgb"])), k
        assert np.array_equal(r["rgb"].cpu().numpy().reshape(-1, 3), exp["rgb_u8"]), k
        assert np.array_equal(_bits(r["depth"].cpu().numpy().reshape(-1)), _bits(exp["depth"])), k
        assert np.array_equal(r["triangle"].cpu().numpy().reshape(-1), exp["triangle"]), k
        cov = exp["triangle"] >= 0
        diff = exp["rgb_u8"][cov].astype(np.float64) / 255 - r1[k]["rgb_u8"][cov].astype(np.float64) / 255
        se, n = se + (diff ** 2).sum(), n + diff.size
    seen = views > 0
    print(f"closed loop: {seen.mean():.3f} of the vertices seen, {views[seen].mean():.2f} views each, PSNR over the covered "
          f"pixels of the six frames {-10 * np.log10(se / n):.2f} dB")
    assert seen.mean() > 0.9
