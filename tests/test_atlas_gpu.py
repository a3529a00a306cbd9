"""GPU checks of the texture atlas: the points, resolve and atlas-shade kernels (csrc/nfl_atlas.hip) against the numpy
restatement of tests/atlas_ref.py, through the C ABI and through geometry.bake_texture / render_mesh(texture=) and
eval.evaluate_mesh(texture=).

Both sides evaluate the same fp32 formulae with every operation rounded on its own (the library is built with
-ffp-contract=off; division and square root are correctly rounded on both), so EVERYTHING is held to equality: points,
normals, texels as floats and bytes, seen flags, rendered colours, depths and triangle indices.

The shapes are the smallest that cross the boundaries of the code: 1 / 2 / 3 triangles (an ownerless half, a full cell, a
partly empty last cell), 63 / 64 / 65 / 257 for the waves and the 256-thread workgroups (every atlas here has a last
workgroup that is not full, and the staged stores must stop at its end), cells of 6 (L = 1), 7 and 16 texels, one column,
three, and the default.  The restatement of a case is computed once and shared."""
import ctypes as C

import numpy as np
import pytest
import torch

import atlas_ref as aref
import meshcolor_ref as mref
import meshrender_ref as rref
from geom_gpu_util import (dev as _dev, F, field_bits as _bits, framed as _framed, PAD, ptr as _ptr,
                           same_fields as _same, stream as _stream, unframe as _unframe)
from gpu_util import DEV
from nerf_fl_amd import _lib, eval as nfl_eval, geometry, metrics
from nerf_fl_amd.data import ImageBank

pytestmark = pytest.mark.gpu

S_WORD, S_F, S_I, S_B = 0x0123456789ABCDEF, -7.0, -7, 0xAB
BG = (0.25, 0.5, 0.75)
KEYS = ("rgb", "rgb_u8", "depth", "triangle")


def _abi_points(ver, nrm, tri, lay, first=0, count=None):
    """nfl_atlas_points of texels first .. first + count - 1, both outputs framed by sentinels."""
    count = lay["width"] * lay["height"] - first if count is None else count
    d_ver, d_nrm, d_tri = _dev(np.reshape(ver, (-1, 3)), F), _dev(np.reshape(nrm, (-1, 3)), F), _dev(np.reshape(tri, (-1, 3)), np.int32)
    p, m = _framed(count, (3,), S_F, torch.float32), _framed(count, (3,), S_F, torch.float32)
    a = _lib.AtlasPointsArgs()
    a.d_vertices, a.d_vertex_normals, a.d_triangles = _ptr(d_ver), _ptr(d_nrm), _ptr(d_tri)
    a.n_vertices, a.n_triangles = d_ver.shape[0], d_tri.shape[0]
    a.cell, a.cols, a.rows, a.first_texel, a.n_texels = lay["cell"], lay["cols"], lay["rows"], first, count
    a.d_points, a.d_normals = p[PAD:].data_ptr(), m[PAD:].data_ptr()
    _lib.check(_lib.lib().nfl_atlas_points(C.byref(a), _stream()), "nfl_atlas_points")
    return {"points": _unframe(p, count, S_F, "points"), "normals": _unframe(m, count, S_F, "normals")}


RESOLVE_KEYS = ("texture", "texture_u8", "seen")


def _abi_resolve(tri, V, lay, sums, views, vcol=None, fallback=(0.5, 0.5, 0.5), background=BG, first=0, outputs=RESOLVE_KEYS):
    n = views.shape[0]
    d_tri = _dev(np.reshape(tri, (-1, 3)), np.int32)
    d_sum, d_views = _dev(sums, F), _dev(views, np.int32)
    d_col = None if vcol is None else _dev(vcol, F)
    bufs = {"texture": _framed(n, (3,), S_F, torch.float32), "texture_u8": _framed(n, (3,), S_B, torch.uint8),
            "seen": _framed(n, (), S_B, torch.uint8)}
    a = _lib.AtlasResolveArgs()
    a.d_triangles, a.n_vertices, a.n_triangles = _ptr(d_tri), V, d_tri.shape[0]
    a.cell, a.cols, a.rows, a.first_texel, a.n_texels = lay["cell"], lay["cols"], lay["rows"], first, n
    a.d_sum, a.d_views, a.d_vertex_colors = d_sum.data_ptr(), d_views.data_ptr(), _ptr(d_col)
    a.fallback[:], a.background[:] = fallback, background
    a.d_texture, a.d_texture_u8, a.d_seen = (bufs[k][PAD:].data_ptr() if k in outputs else None for k in RESOLVE_KEYS)
    _lib.check(_lib.lib().nfl_atlas_resolve(C.byref(a), _stream()), "nfl_atlas_resolve")
    got = {}
    for k, sentinel in zip(RESOLVE_KEYS, (S_F, S_B, S_B)):
        h = _unframe(bufs[k], n, sentinel, k)
        if k in outputs:
            got[k] = h
        else:
            assert (h == sentinel).all(), k                          # a NULL output is skipped, and nothing else lands there
    return got


def _abi_shade(ver, tri, cams, words, atlas, lay, outputs=KEYS, background=BG):
    """nfl_mesh_shade_atlas of the run `cams` over `words`; `atlas` (H, W, 3) fp32 or uint8, framed by sentinels too."""
    n = int(sum(c["width"] * c["height"] for c in cams))
    d_ver, d_tri = _dev(np.reshape(ver, (-1, 3)), F), _dev(np.reshape(tri, (-1, 3)), np.int32)
    d_table = torch.from_numpy(mref.table_of(cams).view(np.uint8).reshape(-1).copy()).to(DEV)
    vis = torch.full((n + 2 * PAD,), S_WORD, dtype=torch.int64, device=DEV)
    vis[PAD:PAD + n] = torch.from_numpy(np.asarray(words, dtype=np.uint64).view(np.int64).copy()).to(DEV)
    u8 = atlas.dtype == np.uint8
    d_atlas = torch.full((atlas.size + 2 * PAD,), 0xCD if u8 else float("nan"), dtype=torch.uint8 if u8 else torch.float32, device=DEV)
    d_atlas[PAD:PAD + atlas.size] = _dev(atlas.reshape(-1), atlas.dtype)
    bufs = {"rgb": _framed(n, (3,), S_F, torch.float32), "rgb_u8": _framed(n, (3,), S_B, torch.uint8),
            "depth": _framed(n, (), S_F, torch.float32), "triangle": _framed(n, (), S_I, torch.int32)}
    s = _lib.MeshShadeAtlasArgs()
    s.d_vertices, s.d_triangles, s.n_vertices, s.n_triangles = _ptr(d_ver), _ptr(d_tri), d_ver.shape[0], d_tri.shape[0]
    s.d_table, s.n_images, s.first, s.count = d_table.data_ptr(), len(cams), 0, len(cams)
    s.d_vis, s.n_vis = vis[PAD:].data_ptr(), n
    s.d_atlas, s.d_atlas_u8 = (None, d_atlas[PAD:].data_ptr()) if u8 else (d_atlas[PAD:].data_ptr(), None)
    s.cell, s.cols, s.rows = lay["cell"], lay["cols"], lay["rows"]
    s.background[:] = background
    s.d_rgb, s.d_rgb_u8, s.d_depth, s.d_triangle = (bufs[k][PAD:].data_ptr() if k in outputs else None for k in KEYS)
    _lib.check(_lib.lib().nfl_mesh_shade_atlas(C.byref(s), _stream()), "nfl_mesh_shade_atlas")
    got = {}
    for k, sentinel in zip(KEYS, (S_F, S_B, S_F, S_I)):
        h = _unframe(bufs[k], n, sentinel, k)
        if k in outputs:
            got[k] = h
        else:
            assert (h == sentinel).all(), k
    return got


# ---- the soup, its attributes and its visibility words: computed once ---------------------------------------------------

COUNTS = [1, 2, 3, 63, 64, 65, 257]
SOUP_CAM = mref.camera(**mref.SOUP_CAMERA)


@pytest.fixture(scope="module")
def soup():
    ver, tri = mref.soup(400, 7)
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=ver.shape).astype(F)
    nrm[3 * 40:3 * 40 + 3] = 0.0                                     # triangle 40: no normal anywhere
    nrm[3 * 41] = [1, 0, 0]
    nrm[3 * 41 + 1] = [-1, 0, 0]
    nrm[3 * 41 + 2] = [0, 0, 0]                                      # triangle 41: zero along a line through texels
    col = rng.uniform(-0.2, 1.2, size=ver.shape).astype(F)
    words = {T: rref.visibility(ver, tri[:T], SOUP_CAM).reshape(-1) for T in COUNTS}
    return dict(ver=ver, tri=tri, nrm=nrm, col=col, words=words)


def _blend_like(n, seed):
    """Sums and views as a blend might leave them, and as it never would: unseen texels, a zero weight, NaN, out of gamut."""
    rng = np.random.default_rng(seed)
    views = rng.integers(0, 3, size=n).astype(np.int32)
    w = rng.uniform(0.1, 3.0, size=(n, 1))
    sums = np.concatenate([rng.uniform(-0.1, 1.1, size=(n, 3)) * w, w], axis=1).astype(F)
    sums[::17, 3] = 0.0
    sums[5::23, 1] = np.nan
    views[3::29] = -1
    return sums, views


def _salted(tri, T):
    """triangles[:T] with triangle 1 naming a vertex that does not exist (from three triangles on)."""
    t = tri[:T].copy()
    if T >= 3:
        t[1] = [0, 1, 3 * 400]
    return t


@pytest.mark.parametrize("T", COUNTS)
def test_points_resolve_and_shade_equal_the_restatement(soup, T):
    ver, nrm, col = soup["ver"], soup["nrm"], soup["col"]
    tri = _salted(soup["tri"], T)
    words = soup["words"][T]
    for C_ in (6, 7, 16):
        for cols in (1, 3, None):
            if cols == 3 and T <= 2:
                continue                                             # the same atlas as one column, two cells wider
            lay = aref.layout(T, C_, cols)
            what = (T, C_, cols)
            n = lay["width"] * lay["height"]
            p, m = aref.points(ver, nrm, tri, lay)
            _same(_abi_points(ver, nrm, tri, lay), {"points": p, "normals": m}, what)
            sums, views = _blend_like(n, C_ + T)
            for vcol in (col, None):
                tex, tex8, seen = aref.resolve(tri, ver.shape[0], lay, sums, views, vcol, (0.1, 0.6, 1.3), BG)
                _same(_abi_resolve(tri, ver.shape[0], lay, sums, views, vcol, (0.1, 0.6, 1.3), BG),
                      {"texture": tex, "texture_u8": tex8, "seen": seen}, what)
            assert T < 3 or (seen.any() and not seen.all() and np.isnan(p).any())
            H, W = lay["height"], lay["width"]
            for atlas in (tex.reshape(H, W, 3), tex8.reshape(H, W, 3)):
                exp = aref.shade(ver, tri, SOUP_CAM, words, atlas, lay, BG)
                _same(_abi_shade(ver, tri, [SOUP_CAM], words, atlas, lay), exp, what + (atlas.dtype,))
    assert (exp["triangle"] >= 0).any()


def test_null_outputs_are_skipped(soup):
    ver, tri = soup["ver"], soup["tri"][:65]
    lay = aref.layout(65, 7, 3)
    n = lay["width"] * lay["height"]
    sums, views = _blend_like(n, 1)
    tex, tex8, seen = aref.resolve(tri, ver.shape[0], lay, sums, views, soup["col"], background=BG)
    for outputs in (("texture",), ("texture_u8",), ("seen",), ("texture_u8", "seen"), ()):
        _same(_abi_resolve(tri, ver.shape[0], lay, sums, views, soup["col"], outputs=outputs),
              {"texture": tex, "texture_u8": tex8, "seen": seen}, outputs)
    atlas = tex.reshape(lay["height"], lay["width"], 3)
    exp = aref.shade(ver, tri, SOUP_CAM, soup["words"][65], atlas, lay, BG)
    for outputs in (("rgb",), ("rgb_u8", "triangle"), ("depth",), ()):
        _same(_abi_shade(ver, tri, [SOUP_CAM], soup["words"][65], atlas, lay, outputs=outputs), exp, outputs)


def test_forged_words_are_uncovered_or_sampled_inside_the_atlas(soup):
    """Words no raster wrote.  Uncovered: a triangle number >= T, the largest 32-bit number, a triangle with a bad index.
    Covered all the same: EVERY pixel claimed by some triangle that its ray misses, so the barycentrics are arbitrary (and
    huge for the grazing ones); the lookup is clamped into the triangle's cell and the atlas' frame of NaNs is never read."""
    ver = soup["ver"]
    tri = _salted(soup["tri"], 65)
    lay = aref.layout(65, 7, 3)
    n = lay["width"] * lay["height"]
    tex, tex8, _ = aref.resolve(tri, ver.shape[0], lay, np.zeros((n, 4), F), np.zeros(n, np.int32), soup["col"])
    P = 65 * 33
    words = (np.uint64(0x40400000) << np.uint64(32)) | (np.arange(P, dtype=np.uint64) % np.uint64(65))
    words[::3] = (np.uint64(0x40400000) << np.uint64(32)) | np.uint64(65)
    words[1::7] = (np.uint64(0x40400000) << np.uint64(32)) | np.uint64(0xFFFFFFFE)
    words[2::11] = rref.EMPTY
    for atlas in (tex.reshape(lay["height"], lay["width"], 3), tex8.reshape(lay["height"], lay["width"], 3)):
        want = aref.shade(ver, tri, SOUP_CAM, words, atlas, lay, BG)
        got = _abi_shade(ver, tri, [SOUP_CAM], words, atlas, lay)
        _same(got, want, "forged")
        assert (got["triangle"][::3] == -1).all() and (got["triangle"][words & np.uint64(0xFFFFFFFF) == 1] == -1).all()
        assert (got["triangle"] >= 0).mean() > 0.4 and np.isfinite(got["rgb"][got["triangle"] >= 0]).all()


def test_both_shades_give_the_same_depth_and_triangle(soup):
    """One front for both shading passes: over ONE visibility buffer, written by the raster for two 65 x 33 images of the
    65-triangle soup with a triangle across the frame that straddles the camera plane, and with two words forged,
    nfl_mesh_shade and nfl_mesh_shade_atlas write the same depth bits and the same triangle index at every word."""
    ver = np.concatenate([soup["ver"][:3 * 65], np.array([[-40, 2, -12], [40, 2, -12], [0, -3, 1.5]], dtype=F)])
    tri = np.concatenate([soup["tri"][:65], [[195, 196, 197]]])
    cams = [SOUP_CAM, mref.camera(65, 33, 40, 40, 32, 16)]
    lib, n = _lib.lib(), 2 * 65 * 33
    d_ver, d_tri = _dev(ver, F), _dev(tri, np.int32)
    d_table = torch.from_numpy(mref.table_of(cams).view(np.uint8).reshape(-1).copy()).to(DEV)
    vis = torch.empty(n, dtype=torch.int64, device=DEV)
    geometry.images._run_visibility(d_ver, d_tri, d_table, 2, 0, 2, vis)
    vis[5] = (0x40400000 << 32) | 66                                 # no such triangle: uncovered
    vis[n - 7] = (0x40400000 << 32) | 3                              # a triangle the raster did not write there: covered
    lay = aref.layout(66, 6)
    atlas = torch.zeros(lay["height"], lay["width"], 3, dtype=torch.float32, device=DEV)
    out = []
    for name, s in (("nfl_mesh_shade", _lib.MeshShadeArgs()), ("nfl_mesh_shade_atlas", _lib.MeshShadeAtlasArgs())):
        depth = torch.full((n,), S_F, dtype=torch.float32, device=DEV)
        winner = torch.full((n,), S_I, dtype=torch.int32, device=DEV)
        s.d_vertices, s.d_triangles, s.n_vertices, s.n_triangles = d_ver.data_ptr(), d_tri.data_ptr(), 198, 66
        s.d_table, s.n_images, s.first, s.count = d_table.data_ptr(), 2, 0, 2
        s.d_vis, s.n_vis, s.d_depth, s.d_triangle = vis.data_ptr(), n, depth.data_ptr(), winner.data_ptr()
        if name == "nfl_mesh_shade":
            s.mode = _lib.SHADE_MODES["facing"]
        else:
            s.d_atlas, s.cell, s.cols, s.rows = atlas.data_ptr(), lay["cell"], lay["cols"], lay["rows"]
        _lib.check(getattr(lib, name)(C.byref(s), _stream()), name)
        out.append((depth.view(torch.int32), winner))
    (depth_a, winner_a), (depth_b, winner_b) = out
    assert torch.equal(depth_a, depth_b) and torch.equal(winner_a, winner_b)
    assert winner_a[5] == -1 and winner_a[n - 7] == 3
    for k in (-1, 65):                                               # uncovered words, the straddling triangle, the soup
        assert 0.1 < (winner_a == k).float().mean() < 0.8
    assert ((winner_a >= 0) & (winner_a < 65)).sum() > 100


def test_a_split_range_and_a_second_run_give_the_same_bits(soup):
    ver, nrm, tri = soup["ver"], soup["nrm"], _salted(soup["tri"], 257)
    lay = aref.layout(257, 7)
    n = lay["width"] * lay["height"]
    whole = _abi_points(ver, nrm, tri, lay)
    _same(_abi_points(ver, nrm, tri, lay), whole, "second run")
    sums, views = _blend_like(n, 2)
    tex = _abi_resolve(tri, ver.shape[0], lay, sums, views, soup["col"])
    for pieces in (2, 7):
        cuts = [n * k // pieces for k in range(pieces + 1)]
        parts = [_abi_points(ver, nrm, tri, lay, a, b - a) for a, b in zip(cuts, cuts[1:])]
        _same({k: np.concatenate([p[k] for p in parts]) for k in whole}, whole, pieces)
        parts = [_abi_resolve(tri, ver.shape[0], lay, sums[a:b], views[a:b], soup["col"], first=a) for a, b in zip(cuts, cuts[1:])]
        _same({k: np.concatenate([p[k] for p in parts]) for k in tex}, tex, pieces)
    assert n % 256 and any(c % 256 for c in cuts[1:-1])


# ---- the cube of atlas_ref.closed_loop, its cameras and its bank ---------------------------------------------------------------

def _mesh(ver, nrm, tri, col=None):
    mesh = {"vertices": _dev(ver, F), "normals": _dev(nrm, F), "triangles": _dev(tri, np.int32)}
    return mesh if col is None else dict(mesh, colors=_dev(col, F))


def _on_dev(atlas):
    return {k: (torch.from_numpy(np.ascontiguousarray(v)).to(DEV) if isinstance(v, np.ndarray) else v) for k, v in atlas.items()}


@pytest.fixture(scope="module")
def loop():
    """The restatement's walk of the closed loop, and the device's first leg of it: the cube rendered with the source atlas
    from the six cameras, and the uint8 bank of those frames.  Made once, never written to."""
    r = aref.closed_loop()
    mesh = _mesh(r["ver"], r["nrm"], r["tri"])
    source = _on_dev({k: r["source"][k] for k in ("texture_u8", "cell", "cols")})
    first = [geometry.render_mesh(mesh, r["poses"][k], r["Ks"][k], 40, 48, texture=source) for k in range(6)]
    bank = ImageBank([f["rgb"].cpu().numpy() for f in first], r["poses"], r["Ks"], 2.0, 6.0, device=DEV)
    # a second bank for the bake tests: six oblique cameras, so that a texel has up to three views that differ
    cams, poses, Ks = aref.cube_cameras(focal=40.0, eyes=aref.OBLIQUE_EYES)
    frames = [aref.render(r["ver"], r["tri"], c, r["source"]["texture_u8"], r["source"]) for c in cams]
    images = [f["rgb_u8"].reshape(40, 48, 3) for f in frames]
    oblique = dict(cams=cams, images=images, depths=[mref.depth_map(r["ver"], r["tri"], c) for c in cams],
                   bank=ImageBank(images, poses, Ks, 1.0, 6.0, device=DEV))
    return dict(r, mesh=mesh, dev_source=source, dev_first=first, bank=bank, oblique=oblique)


def _equal_render(got, exp, what):
    assert np.array_equal(_bits(got["rgb_float"].cpu().numpy()), _bits(exp["rgb"])), what
    assert np.array_equal(got["rgb"].cpu().numpy().reshape(-1, 3), exp["rgb_u8"]), what
    assert np.array_equal(_bits(got["depth"].cpu().numpy().reshape(-1)), _bits(exp["depth"])), what
    assert np.array_equal(got["triangle"].cpu().numpy().reshape(-1), exp["triangle"]), what


def _equal_bake(got, exp, what):
    assert (got["cell"], got["cols"], got["rows"]) == (exp["cell"], exp["cols"], exp["rows"]), what
    assert got["texture"].dtype == torch.float32 and got["texture_u8"].dtype == torch.uint8 and got["seen"].dtype == torch.bool
    for k in ("texture", "texture_u8", "seen", "views"):
        g = got[k].cpu().numpy()
        assert g.shape == exp[k].shape and np.array_equal(_bits(g), _bits(exp[k])), (what, k)


def test_the_closed_loop_equals_the_restatement_and_beats_vertex_colours(loop):
    """mesh + source atlas -> six uint8 frames -> bake_texture -> frames again, and beside it color_mesh_from_images -> frames:
    everything bit-equal to the restatement walking the same loop, and the textured loop's PSNR over the covered pixels HIGHER
    than the vertex-colour loop's (17.93 dB against 5.52 dB: twelve triangles cannot carry stripes a third of an edge wide in
    24 colours).  An ordering, no threshold."""
    r = loop
    for k in range(6):
        _equal_render(r["dev_first"][k], r["first"][k], ("first", k))
    got = geometry.color_mesh_from_images(r["mesh"], r["bank"], 0.05)
    assert np.array_equal(_bits(got["colors"].cpu().numpy()), _bits(r["colors"]))
    mesh = dict(r["mesh"], colors=got["colors"])
    baked = geometry.bake_texture(mesh, r["bank"], 0.05)
    _equal_bake(baked, r["baked"], "baked")
    textured = [geometry.render_mesh(mesh, bank=r["bank"], image=k, texture=baked) for k in range(6)]
    vertexed = [geometry.render_mesh(mesh, bank=r["bank"], image=k) for k in range(6)]
    for k in range(6):
        _equal_render(textured[k], r["textured"][k], ("textured", k))
        _equal_render(vertexed[k], r["vertexed"][k], ("vertex colours", k))
    truth = [f["rgb"].cpu().numpy().reshape(-1, 3) for f in r["dev_first"]]
    cov = [f["covered"].cpu().numpy().reshape(-1) for f in r["dev_first"]]
    psnr_t = aref.psnr_covered([f["rgb"].cpu().numpy().reshape(-1, 3) for f in textured], truth, cov)
    psnr_v = aref.psnr_covered([f["rgb"].cpu().numpy().reshape(-1, 3) for f in vertexed], truth, cov)
    print(f"closed loop on the device: textured {psnr_t:.2f} dB, vertex colours {psnr_v:.2f} dB")
    assert psnr_t == r["psnr_textured"] and psnr_v == r["psnr_vertex"]
    assert psnr_t > psnr_v
    # the byte atlas renders too, and render_mesh takes it when there is no float one
    bytes_only = {k: baked[k] for k in ("texture_u8", "cell", "cols")}
    exp = aref.render(r["ver"], r["tri"], r["cams"][1], r["baked"]["texture_u8"], r["baked"])
    _equal_render(geometry.render_mesh(mesh, bank=r["bank"], image=1, texture=bytes_only), exp, "byte atlas")


@pytest.mark.parametrize("case", ["plain", "reject", "uniform_weights", "cell7_flat"])
def test_bake_texture_equals_the_restatement(loop, case):
    """With and without `reject`, with the images in runs of 1, 4 + 2 and 6, and with texel batches smaller than the atlas."""
    r = loop
    mesh = dict(r["mesh"], colors=_dev(r["colors"], F))
    kw, ref_kw = dict(cell=16, fallback="colors"), dict(cell=16, vertex_colors=r["colors"])
    if case == "reject":
        kw, ref_kw = dict(kw, reject=0.02), dict(ref_kw, reject=0.02)
    elif case == "uniform_weights":
        w = [1.0, 0.5, 0.0, 2.0, 1.0, 0.25]
        kw, ref_kw = dict(kw, weighting="uniform", image_weights=w, min_cos=0.2), dict(ref_kw, weighting="uniform", image_weights=w, min_cos=0.2)
    elif case == "cell7_flat":
        kw = dict(cell=7, cols=2, fallback=(0.1, 0.2, 0.3), background=BG)
        ref_kw = dict(cell=7, cols=2, fallback=(0.1, 0.2, 0.3), background=BG)
    ob = r["oblique"]
    exp = aref.bake(r["ver"], r["nrm"], r["tri"], ob["cams"], ob["images"], 0.05, depths=ob["depths"], **ref_kw)
    n = exp["width"] * exp["height"]
    assert 0.2 < exp["seen"].mean() < 1.0 and exp["views"].max() >= 2
    if case == "reject":                                             # some texels lose every sample and keep the first pass's colour
        plain = aref.bake(r["ver"], r["nrm"], r["tri"], ob["cams"], ob["images"], 0.05, depths=ob["depths"], **dict(ref_kw, reject=None))
        lost = plain["seen"] & ~exp["seen"]
        assert lost.sum() > 100 and np.array_equal(exp["texture"][lost], plain["texture"][lost])
    for batch_pixels, texel_batch in ((1 << 26, 1 << 24), (48 * 40, n), (4 * 48 * 40, 500), (1 << 26, 256), (48 * 40, 777)):
        got = geometry.bake_texture(mesh, ob["bank"], 0.05, batch_pixels=batch_pixels, texel_batch=texel_batch, **kw)
        _equal_bake(got, exp, (case, batch_pixels, texel_batch))


def test_bake_texture_arguments(loop):
    r = loop
    mesh = dict(r["mesh"], colors=_dev(r["colors"], F))
    bare = r["mesh"]
    for m, bad in ((bare, dict()), (mesh, dict(fallback="colours")), (mesh, dict(fallback=(1.0, 2.0))), (mesh, dict(cell=5)),
                   (mesh, dict(cols=0)), (mesh, dict(texel_batch=0)), (mesh, dict(background=(1.0,))), (mesh, dict(weighting="sin")),
                   (mesh, dict(reject=-1.0)), (mesh, dict(images=[6])), (mesh, dict(batch_pixels=0))):
        with pytest.raises(ValueError):
            geometry.bake_texture(m, r["bank"], 0.05, **bad)
    with pytest.raises(ValueError):
        geometry.bake_texture(mesh, r["bank"], -0.05)
    assert geometry.bake_texture(bare, r["bank"], 0.05, fallback=(0.5, 0.5, 0.5))["seen"].any()         # no colours needed
    baked = _on_dev({k: r["baked"][k] for k in ("texture", "texture_u8", "cell", "cols")})
    for bad in (dict(baked, cell=8), dict(baked, cols=2), dict(baked, texture=baked["texture"][:16]),
                dict(baked, texture=baked["texture"].double()), dict(cell=16, cols=3), dict(baked, texture=baked["texture"][:, :, :2])):
        with pytest.raises(ValueError):
            geometry.render_mesh(mesh, bank=r["bank"], image=0, texture=bad)
    for shade in ("normal", "facing"):
        with pytest.raises(ValueError):
            geometry.render_mesh(mesh, bank=r["bank"], image=0, texture=baked, shade=shade)


def test_with_no_image_the_textured_render_is_the_vertex_colour_render():
    """images=[] and fallback='colors': every texel holds the vertex colours interpolated at it, and the bilinear lookup of
    that affine function gives the vertex-colour render back up to two evaluation orders of one affine function.  The bound
    is four times atlas_ref.SOUP_FIGURE, the worst difference of the fp32 restatement from the fp64 vertex-colour
    interpolation on the same soup and camera (2.46e-6, tests/test_atlas_cpu.py)."""
    ver, tri = mref.soup(400, 7)
    col = np.random.default_rng(11).uniform(size=(ver.shape[0], 3)).astype(F)
    nrm = np.random.default_rng(12).normal(size=ver.shape).astype(F)
    mesh = _mesh(ver, nrm, tri, col)
    K = np.array([[40.0, 0, 32.25], [0, 40.0, 16.5], [0, 0, 1]])
    pose = np.eye(4)[:3]
    bank = ImageBank([np.zeros((33, 65, 3), np.uint8)], pose[None], K[None], 2.0, 6.0, device=DEV)
    baked = geometry.bake_texture(mesh, bank, 0.05, images=[], fallback="colors")
    assert not baked["seen"].any() and (baked["views"] == 0).all()
    lay = aref.layout(400, 16)
    n = lay["width"] * lay["height"]
    tex, tex8, _ = aref.resolve(tri, ver.shape[0], lay, np.zeros((n, 4), F), np.zeros(n, np.int32), col)
    assert np.array_equal(_bits(baked["texture"].cpu().numpy().reshape(-1, 3)), _bits(tex))
    assert np.array_equal(baked["texture_u8"].cpu().numpy().reshape(-1, 3), tex8)
    textured = geometry.render_mesh(mesh, pose, K, 33, 65, texture=baked)
    vertexed = geometry.render_mesh(mesh, pose, K, 33, 65)
    _equal_render(textured, aref.render(ver, tri, SOUP_CAM, tex.reshape(lay["height"], lay["width"], 3), lay), "soup")
    assert torch.equal(textured["triangle"], vertexed["triangle"]) and torch.equal(textured["depth"], vertexed["depth"])
    cov = vertexed["covered"].reshape(-1)
    worst = (textured["rgb_float"][cov] - vertexed["rgb_float"][cov]).abs().max().item()
    print(f"soup, no image: textured against vertex-colour render, worst difference {worst:.3e} (bound {4 * aref.SOUP_FIGURE:.1e})")
    assert 0.5 < cov.float().mean().item() < 0.75
    assert worst <= 4 * aref.SOUP_FIGURE
    assert torch.equal(textured["rgb_float"][~cov], vertexed["rgb_float"][~cov])


# ---- evaluate_mesh(texture=) and the synchronisation checks --------------------------------------------------------------------

def test_evaluate_mesh_with_a_texture_on_a_bank_rendered_from_it(loop, monkeypatch):
    """A bank rendered from the textured mesh scores an error of exactly zero; ONE device-to-host copy, everything before it
    under the sync check."""
    r = loop
    mesh, atlas = r["mesh"], r["dev_source"]
    frames = [geometry.render_mesh(mesh, bank=r["bank"], image=k, texture=atlas, background=(0.0, 0.0, 0.0)) for k in range(6)]
    bank = ImageBank([f["rgb"].cpu().numpy() for f in frames], r["poses"], r["Ks"], 2.0, 6.0, device=DEV)
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
        res = nfl_eval.evaluate_mesh(mesh, bank, texture=atlas, return_images=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        monkeypatch.undo()
    assert copies == [(6, 8)]
    table = res["table"].cpu().numpy()
    col = {name: table[:, j] for j, name in enumerate(metrics.METRIC_COLUMNS)}
    assert (col["sse_valid"] == 0).all() and (col["sse"] == 0).all() and (col["count_valid"] > 0).all()
    assert np.isposinf(res["psnr_valid"].numpy()).all() and np.isposinf(res["psnr"].numpy()).all()
    assert all(torch.equal(f, g["rgb"]) for f, g in zip(res["frames"], frames))
    # the baked atlas is not the source: it scores finite, and above the vertex colours it was baked beside
    baked = _on_dev({k: r["baked"][k] for k in ("texture", "cell", "cols")})
    textured = nfl_eval.evaluate_mesh(mesh, bank, texture=baked)
    vertexed = nfl_eval.evaluate_mesh(mesh, bank, colors=_dev(r["colors"], F))
    assert np.isfinite(textured["psnr_valid"].numpy()).all()
    assert textured["mean_psnr_valid"] > vertexed["mean_psnr_valid"]


def test_no_host_synchronisation_in_bake_and_textured_render(loop):
    """bake_texture (one batch and several, with and without reject) and render_mesh(texture=) in the bank form under torch's
    synchronisation check: a blocking copy or a read of a device value raises."""
    r = loop
    mesh = dict(r["mesh"], colors=_dev(r["colors"], F))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        one = geometry.bake_texture(mesh, r["bank"], 0.05)
        several = geometry.bake_texture(mesh, r["bank"], 0.05, texel_batch=500, reject=0.02, batch_pixels=4 * 48 * 40)
        frame = geometry.render_mesh(mesh, bank=r["bank"], image=2, texture=one)
        frame8 = geometry.render_mesh(mesh, bank=r["bank"], image=3, texture={k: one[k] for k in ("texture_u8", "cell", "cols")})
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert one["texture"].shape == (32, 48, 3) and several["seen"].any() and frame["covered"].any() and frame8["covered"].any()


# ---- extract_mesh(texture=) -------------------------------------------------------------------------------------------------

def test_extract_mesh_bakes_after_colouring_and_writes_the_obj_set(loop, tmp_path):
    from PIL import Image
    from nerf_fl_amd import NeRF, PosEmbedding, synth
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(DEV)
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (17, 17, 17)
    bank = loop["bank"]
    with torch.no_grad():
        iso = geometry.density_lattice(model, emb, lo, hi, res).median().item()
        plain = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, color_from=bank, path=str(tmp_path / "plain.ply"))
        assert "atlas" not in plain and sorted(p.name for p in tmp_path.iterdir()) == ["plain.ply"]      # nothing changes without it
        mesh = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, color_from=bank, texture=8, simplify=0.5,
                                     color_kwargs=dict(weighting="uniform", images=[0, 1, 4]), path=str(tmp_path / "ball.obj"))
    assert 0 < mesh["triangles"].shape[0] < plain["triangles"].shape[0] and sorted(mesh) == sorted(list(plain) + ["atlas"])
    exp = geometry.bake_texture(mesh, bank, 2.0 * 2.0 / 16, cell=8, fallback="colors", weighting="uniform", images=[0, 1, 4])
    atlas = mesh["atlas"]
    assert (atlas["cell"], atlas["cols"], atlas["rows"]) == (8, exp["cols"], exp["rows"])
    assert all(torch.equal(atlas[k], exp[k]) for k in ("texture", "texture_u8", "seen", "views")) and atlas["seen"].any()
    assert sorted(p.name for p in tmp_path.iterdir()) == ["ball.mtl", "ball.obj", "ball.png", "plain.ply"]
    assert np.array_equal(np.asarray(Image.open(tmp_path / "ball.png").convert("RGB")), atlas["texture_u8"].cpu().numpy())
    faces = [line for line in open(tmp_path / "ball.obj") if line.startswith("f ")]
    assert len(faces) == mesh["triangles"].shape[0]
