"""A mesh and cameras: depth maps and visibility buffers, rendering, vertex colours and texture atlases from an ImageBank."""
import math

import numpy as np
import torch

from .. import _lib
from ._call import _camera_run, _is, _launch, _mesh_tensors, _on_device, _ptr, _three


def _run_raster(name, a, fields, ver, tri, table, n_images, first, count, words):
    """The raster `name` (its argument struct `a`) of images first .. first + count - 1 of `table` into `words`, one per
    pixel of the run; `fields` names the struct's pointer to them and their number.  On the current device's stream."""
    _camera_run(a, ver, tri, table, n_images, first, count)
    setattr(a, fields[0], _ptr(words))
    setattr(a, fields[1], words.numel())
    _launch(name, a)


def _run_depth(ver, tri, table, n_images, first, count, depth):
    """nfl_mesh_depth of images first .. first + count - 1 of `table` into `depth` (the run's pixels, fp32)."""
    _run_raster("nfl_mesh_depth", _lib.MeshDepthArgs(), ("d_depth", "n_depth"), ver, tri, table, n_images, first, count,
                depth)


def _run_visibility(ver, tri, table, n_images, first, count, vis):
    """nfl_mesh_visibility of images first .. first + count - 1 of `table` into `vis` (the run's pixels, int64 words)."""
    _run_raster("nfl_mesh_visibility", _lib.MeshVisibilityArgs(), ("d_vis", "n_vis"), ver, tri, table, n_images, first,
                count, vis)


def _camera_record(what, dev, c2w, K, H, W, bank, image):
    """The camera forms of mesh_depth, mesh_visibility and render_mesh, checked: (table, n_images, image, H, W), the
    record of a free camera written on the device (no synchronisation when `c2w` and `K` are tensors there)."""
    if bank is not None:
        if c2w is not None or K is not None or H is not None or W is not None or image is None:
            raise ValueError(f"{what}: either (c2w, K, H, W) or (bank=, image=)")
        if bank.device != dev:
            raise ValueError(f"{what}: the bank and the mesh are on different devices")
        image = int(image)
        if not 0 <= image < bank.n_images:
            raise ValueError(f"image: 0 .. {bank.n_images - 1}")
        H, W = int(bank.host_table[image]["height"]), int(bank.host_table[image]["width"])
        return bank.table, bank.n_images, image, H, W
    if c2w is None or K is None or H is None or W is None or image is not None:
        raise ValueError(f"{what}: either (c2w, K, H, W) or (bank=, image=)")
    H, W = int(H), int(W)
    if H < 1 or W < 1 or H * W > 1 << 38:
        raise ValueError(f"{what}: H and W are positive, and H * W is at most 2^38 pixels")
    c2w = torch.as_tensor(c2w, dtype=torch.float32, device=dev).detach()
    K = torch.as_tensor(K, dtype=torch.float32, device=dev).detach()
    if c2w.dim() != 2 or c2w.shape[0] not in (3, 4) or c2w.shape[1] != 4 or K.shape != (3, 3):
        raise ValueError(f"{what}: c2w (3|4, 4) and K (3, 3)")
    # one nfl_image_rec that owns no pixels, written on the device: 26 words, the integers first
    words = torch.zeros(26, dtype=torch.int32, device=dev)
    for at, value in ((4, W), (5, H), (6, 3)):                     # fill kernels: an indexed assignment of a Python
        words[at:at + 1].fill_(value)                               # number goes through a blocking copy instead
    f = words.view(torch.float32)
    f[8:12] = torch.stack([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    f[14:26] = c2w[:3].reshape(12)
    return words, 1, 0, H, W


def _raster_one(what, run, dtype, mesh, c2w, K, H, W, bank, image):
    """The body of mesh_depth and mesh_visibility: `run` of one camera into (H, W) words of `dtype`."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev = ver.device
    table, n_images, image, H, W = _camera_record(what, dev, c2w, K, H, W, bank, image)
    words = torch.empty(H, W, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        run(ver, tri, table, n_images, image, 1, words)
    return words


def mesh_depth(mesh, c2w=None, K=None, H=None, W=None, *, bank=None, image=None):
    """The depth map of `mesh` seen by one camera: (H, W) fp32, per pixel the distance from the camera centre to the
    nearest triangle its ray hits (the quantity rays[:, 6:8] and depth_fine are measured in when |rays_d| = 1), +inf
    where it hits none.  The surface occludes from both sides, pixel centres lie on the integers, and the definition is
    written out in include/nerf_fl_amd.h, "mesh colour".  Two forms:

        mesh_depth(mesh, c2w, K, H, W)          a free camera: c2w (3|4, 4), K (3, 3), tensors or arrays
        mesh_depth(mesh, bank=bank, image=i)    image i of a data.ImageBank on the mesh's device

    Besides a depth image of the geometry to set beside depth_fine, it is a per-pixel near / far tighter than an
    occupancy grid's.  The bank form never synchronises with the host.  The free-camera form does not either when `c2w`
    and `K` are tensors on the mesh's device (its record is then written by device-side fills and copies); an array, a
    list or a CPU tensor is uploaded first, and that copy waits for the stream."""
    return _raster_one("mesh_depth", _run_depth, torch.float32, mesh, c2w, K, H, W, bank, image)


def mesh_visibility(mesh, c2w=None, K=None, H=None, W=None, *, bank=None, image=None):
    """The visibility buffer of `mesh` seen by one camera: (H, W) int64 words, per pixel
    (bits of the fp32 distance << 32) | index of the nearest triangle its ray hits, the lowest index among equally near
    ones, and -1 (all 64 bits set) where it hits none: `word & 0xFFFFFFFF` is the triangle, `(word >> 32)` viewed as fp32
    the value mesh_depth gives.  The camera forms, and what they synchronise, are mesh_depth's; the definition is written
    out in include/nerf_fl_amd.h, "mesh render"."""
    return _raster_one("mesh_visibility", _run_visibility, torch.int64, mesh, c2w, K, H, W, bank, image)


def _atlas_of(texture, T, dev):
    """(fp32 texture or None, uint8 texture or None, cell, cols, rows) of the `texture` dict render_mesh takes, checked
    against a mesh of T triangles on `dev`."""
    try:
        cell, cols = int(texture["cell"]), int(texture["cols"])
        tex, tex8 = texture.get("texture"), texture.get("texture_u8")
    except (TypeError, KeyError, AttributeError):
        raise ValueError("texture: a dict with `texture` (H, W, 3) fp32 or `texture_u8`, `cell` and `cols`") from None
    if tex is not None:
        tex8 = None
    t = tex if tex is not None else tex8
    if t is None:
        raise ValueError("texture: a dict with `texture` (H, W, 3) fp32 or `texture_u8`, `cell` and `cols`")
    _on_device(t)
    if not _is(t, torch.float32 if tex is not None else torch.uint8, 3, (3,), dev):
        raise ValueError(f"texture: expected a contiguous (H, W, 3) fp32 or uint8 tensor on {dev}")
    rows = t.shape[0] // cell if cell > 0 else 0
    lay = atlas_layout(T, cell, cols)                                 # refuses a bad cell or cols
    if t.shape[1] != cols * cell or t.shape[0] != rows * cell or rows < lay["rows"]:
        raise ValueError(f"texture: {tuple(t.shape)} is not an atlas of cell {cell} and {cols} columns for {T} triangles")
    return tex, tex8, cell, cols, rows


def render_mesh(mesh, c2w=None, K=None, H=None, W=None, *, bank=None, image=None, colors=None, shade="color",
                background=(1.0, 1.0, 1.0), texture=None):
    """`mesh` rendered from one camera (the two forms of mesh_depth): the nearest triangle of every pixel
    (nfl_mesh_visibility) and its vertex attributes interpolated there (nfl_mesh_shade); include/nerf_fl_amd.h, "mesh
    render".  No anti-aliasing: a pixel is its centre's ray.  Returns a dict:

        rgb        uint8 (H, W, 3), by eval.to_uint8's rule (clamp, x 255, truncate)
        rgb_float  (H * W, 3) fp32, not clamped: the layout metrics.image_metrics takes
        depth      (H, W) fp32, bit-equal to mesh_depth; +inf where nothing is hit
        triangle   (H, W) int32, -1 where nothing is hit
        covered    bool (H, W)

    shade       "color": `colors` (V, 3) fp32 on the mesh's device, default the mesh's own `colors`; ValueError when
                there are none.  "normal": the mesh's normals as colours, 0.5 * n + 0.5 of the interpolated, normalised
                normal.  "facing": a headlight, |cos| between the triangle's plane normal and the pixel's ray; needs
                neither colours nor normals.
    background  3 numbers: the colour of the pixels that see nothing.
    texture     an atlas: the dict bake_texture returns, or any dict with `texture` ((H, W, 3) fp32) or `texture_u8`
                (uint8, used when `texture` is absent), `cell` and `cols`.  The colour of a covered pixel is then the
                bilinear lookup in its triangle's chart (nfl_mesh_shade_atlas; "mesh atlas" in the header) instead of
                interpolated vertex colours; `colors` is not read, and any `shade` but the default raises.

    It synchronises as mesh_depth does: never in the bank form, not in the free-camera form when `c2w` and `K` are
    tensors on the mesh's device."""
    ver, nrm, col, tri = _mesh_tensors(mesh)
    dev, V = ver.device, ver.shape[0]
    if shade not in _lib.SHADE_MODES:
        raise ValueError(f"shade: one of {sorted(_lib.SHADE_MODES)}, got {shade!r}")
    attr = atlas = None
    if texture is not None:
        if shade != "color":
            raise ValueError("render_mesh: a texture is a colour; shade must be left at 'color'")
        atlas = _atlas_of(texture, tri.shape[0], dev)
    elif shade == "color":
        attr = col if colors is None else colors
        if attr is None:
            raise ValueError("render_mesh: shade='color' needs `colors` or a mesh that has them")
        _on_device(attr)
        if not _is(attr, torch.float32, 2, (3,), dev) or attr.shape[0] != V:
            raise ValueError(f"colors: expected a contiguous fp32 ({V}, 3) tensor on {dev}")
    elif shade == "normal":
        attr = nrm
    background = _three(background, "background: 3 numbers")
    table, n_images, image, H, W = _camera_record("render_mesh", dev, c2w, K, H, W, bank, image)
    vis = torch.empty(H * W, dtype=torch.int64, device=dev)
    out = {"rgb": torch.empty(H, W, 3, dtype=torch.uint8, device=dev),
           "rgb_float": torch.empty(H * W, 3, dtype=torch.float32, device=dev),
           "depth": torch.empty(H, W, dtype=torch.float32, device=dev),
           "triangle": torch.empty(H, W, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        _run_visibility(ver, tri, table, n_images, image, 1, vis)
        a = _camera_run(_lib.MeshShadeArgs() if atlas is None else _lib.MeshShadeAtlasArgs(), ver, tri, table, n_images,
                        image, 1)
        a.d_vis, a.n_vis = _ptr(vis), H * W
        a.background[:] = background
        a.d_rgb, a.d_rgb_u8, a.d_depth, a.d_triangle = (_ptr(out[k]) for k in ("rgb_float", "rgb", "depth", "triangle"))
        if atlas is None:
            a.mode, a.d_attr = _lib.SHADE_MODES[shade], _ptr(attr)
            _launch("nfl_mesh_shade", a)
        else:
            a.d_atlas, a.d_atlas_u8, a.cell, a.cols, a.rows = _ptr(atlas[0]), _ptr(atlas[1]), *atlas[2:]
            _launch("nfl_mesh_shade_atlas", a)
    out["covered"] = out["triangle"] >= 0
    return out


def _image_runs(bank, images, batch_pixels):
    """[(first, count, pixels)]: the selected images of `bank` in ascending order, cut into runs of consecutive images whose
    pixels stay within `batch_pixels` (an image larger than that is a run of its own)."""
    n = bank.n_images
    if images is None:
        sel = list(range(n))
    else:
        sel = sorted({int(i) for i in images})
        if sel and not 0 <= sel[0] <= sel[-1] < n:
            raise ValueError(f"images: indices in 0 .. {n - 1}")
    size = lambda i: int(bank.host_table[i]["width"]) * int(bank.host_table[i]["height"])
    runs = []
    for i in sel:
        if runs and runs[-1][0] + runs[-1][1] == i and runs[-1][2] + size(i) <= batch_pixels:
            runs[-1] = (runs[-1][0], runs[-1][1] + 1, runs[-1][2] + size(i))
        else:
            runs.append((i, 1, size(i)))
    return runs


class _BlendWalk:
    """The walk over the image runs that color_mesh_from_images and bake_texture share: per run the depth map of the MESH
    (nfl_mesh_depth; kept for later passes when `keep` and all of them fit in `batch_pixels`, otherwise rasterised again
    into one scratch) and nfl_mesh_blend of any points with normals, continuing the caller's accumulators."""

    def __init__(self, ver, tri, bank, runs, weights, weighting, min_cos, depth_tol, reject, batch_pixels, keep):
        self.ver, self.tri, self.bank, self.runs = ver, tri, bank, runs
        self.weights, self.weighting, self.min_cos, self.depth_tol, self.reject = weights, weighting, min_cos, depth_tol, reject
        dev = ver.device
        self.keep = keep and sum(r[2] for r in runs) <= batch_pixels
        self.scratch = None if self.keep or not runs else torch.empty(max(r[2] for r in runs), dtype=torch.float32, device=dev)
        self.kept = {}

    def blend(self, points, normals, center, sums, views):
        """One pass over all runs: `sums` (n, 4) and `views` (n,) begin at zero; with `center` (n, 3) the samples further
        than `reject` from it are left out.  On the current device's stream."""
        bank, dev = self.bank, self.ver.device
        a = _lib.MeshBlendArgs()
        a.d_vertices, a.d_normals, a.n_vertices, a.d_pixels = _ptr(points), _ptr(normals), points.shape[0], _ptr(bank.pixels)
        a.d_table, a.n_images, a.weighting = _ptr(bank.table), bank.n_images, _lib.BLEND_WEIGHTINGS[self.weighting]
        a.d_image_weights, a.d_center, a.min_cos, a.depth_tol = _ptr(self.weights), _ptr(center), self.min_cos, self.depth_tol
        a.reject = float(self.reject) if center is not None else 0.0
        a.d_sum, a.d_views = _ptr(sums), _ptr(views)
        for k, (first, count, pixels) in enumerate(self.runs or [(0, 0, 0)]):
            if count and first in self.kept:
                depth = self.kept[first]
            elif count:
                depth = torch.empty(pixels, dtype=torch.float32, device=dev) if self.keep else self.scratch[:pixels]
                _run_depth(self.ver, self.tri, bank.table, bank.n_images, first, count, depth)
                if self.keep:
                    self.kept[first] = depth
            else:
                depth = None
            a.first, a.count, a.start = first, count, int(k == 0)
            a.d_depth, a.n_depth = _ptr(depth), pixels
            _launch("nfl_mesh_blend", a)


def _blend_arguments(what, mesh_dev, bank, depth_tol, images, image_weights, min_cos, weighting, reject, batch_pixels):
    """The blend arguments color_mesh_from_images and bake_texture share, checked: (depth_tol, min_cos, batch_pixels, runs,
    weights)."""
    if getattr(bank, "device", None) != mesh_dev or bank.table is None:
        raise ValueError(f"{what}: `bank` is a data.ImageBank on the mesh's device")
    if weighting not in _lib.BLEND_WEIGHTINGS:
        raise ValueError(f"weighting: one of {sorted(_lib.BLEND_WEIGHTINGS)}, got {weighting!r}")
    depth_tol, min_cos = float(depth_tol), float(min_cos)
    if not depth_tol >= 0.0:
        raise ValueError("depth_tol: a non-negative number")
    if not (min_cos >= 0.0 or (weighting != "cos" and min_cos == min_cos)):
        raise ValueError("min_cos: a number, not negative with weighting='cos' (a weight is never negative)")
    if reject is not None and not float(reject) >= 0.0:
        raise ValueError("reject: a non-negative number")
    batch_pixels = int(batch_pixels)
    if batch_pixels < 1:
        raise ValueError("batch_pixels must be positive")
    runs = _image_runs(bank, images, batch_pixels)
    weights = None
    if image_weights is not None:
        weights = torch.as_tensor(image_weights, dtype=torch.float32, device=mesh_dev).detach().contiguous()
        if weights.shape != (bank.n_images,):
            raise ValueError(f"image_weights: expected ({bank.n_images},)")
    return depth_tol, min_cos, batch_pixels, runs, weights


def color_mesh_from_images(mesh, bank, depth_tol, *, images=None, image_weights=None, min_cos=0.0, weighting="cos",
                           reject=None, fallback=None, batch_pixels=1 << 26):
    """Colour the vertices of `mesh` from the images of `bank` (a data.ImageBank on the mesh's device) that see them:
    every vertex is projected into every selected image, the views in which it lies inside the frame, faces the camera
    (cos of the angle between its normal and the direction to the camera > `min_cos`; a zero normal passes) and is not
    hidden behind the mesh are kept, and their bilinear samples are averaged.  The definition is written out in
    include/nerf_fl_amd.h, "mesh colour".  Returns a dict:

        colors (V, 3) fp32 in [0, 1]; weight (V,) fp32, the sum of the weights; views (V,) int32; seen (V,) bool

    depth_tol     a vertex counts as visible in an image when its distance to the camera is at most the mesh depth map's
                  value at its nearest pixel plus `depth_tol` (world units).  It has no default, as occupancy_grid's
                  threshold has none.  Too small and vertices lose their own views: the depth map is sampled at a pixel
                  centre, up to half a pixel from where the vertex projects, and on a slanted surface that is a depth
                  difference of its own.  Too large and what lies behind a thin structure shows through it.
    images        indices of the images to use (default all); an unselected image costs no raster work.
    image_weights (n_images,) non-negative weights (default 1); a zero weight drops the image from the blend.
    weighting     "cos": a view counts by image weight x cos (head-on views dominate; needs min_cos >= 0); "uniform".
    reject        r: the blend runs twice, and the second pass keeps, for a vertex seen in the first, only the samples
                  within r (largest channel difference) of the first pass's colour: a passer-by in 3 of 40 photographs does
                  not tint the wall.  When the depth maps of all selected images fit in `batch_pixels` they are kept for
                  the second pass; otherwise they are rasterised again.
                  A vertex seen in the first pass whose samples are ALL rejected in the second (two views further than r
                  from their own mean, say) keeps its first-pass colour; its views and weight are 0 and seen is False.
    fallback      colours of the vertices no image sees: (V, 3) or 3 numbers (default 0.5 grey).
    batch_pixels  depth words held at a time: the images are walked in runs of consecutive images within it, each run
                  a fill, a raster and a blend that continues the accumulators.

    No host synchronisation of its own: `image_weights` and `fallback` given as tensors on the device (or left at their
    defaults) are used as they are; given as lists, arrays or CPU tensors they are uploaded first, and that copy waits
    for the stream."""
    ver, nrm, _, tri = _mesh_tensors(mesh)
    dev, V = ver.device, ver.shape[0]
    depth_tol, min_cos, batch_pixels, runs, weights = _blend_arguments(
        "color_mesh_from_images", dev, bank, depth_tol, images, image_weights, min_cos, weighting, reject, batch_pixels)
    if fallback is None:
        fallback = torch.full((3,), 0.5, dtype=torch.float32, device=dev)
    fallback = torch.as_tensor(fallback, dtype=torch.float32, device=dev).detach()
    if fallback.shape not in ((3,), (V, 3)):
        raise ValueError(f"fallback: 3 numbers or ({V}, 3)")
    walk = _BlendWalk(ver, tri, bank, runs, weights, weighting, min_cos, depth_tol, reject, batch_pixels,
                      keep=reject is not None)
    sums = torch.empty(V, 4, dtype=torch.float32, device=dev)
    views = torch.empty(V, dtype=torch.int32, device=dev)

    def one_pass(center, fallback):
        walk.blend(ver, nrm, center, sums, views)
        seen = views > 0
        colors = torch.where(seen[:, None], (sums[:, :3] / sums[:, 3:4]).clamp(0.0, 1.0), fallback.expand(V, 3))
        return colors.contiguous(), seen

    with torch.cuda.device(dev):
        colors, seen = one_pass(None, fallback)
        if reject is not None:
            colors, seen = one_pass(colors, colors)                       # all samples rejected: the first pass's colour stays
    return {"colors": colors, "weight": sums[:, 3].contiguous(), "views": views, "seen": seen}


def atlas_layout(n_triangles, cell, cols=None):
    """The texture atlas of a mesh of `n_triangles` (include/nerf_fl_amd.h, "mesh atlas"): one chart per triangle, two
    triangles to a square cell of `cell` x `cell` texels (6 .. 1024), `cols` cells a row (default
    ceil(sqrt(ceil(T / 2))), a square atlas), at least one row and one column.  Returns a dict: cell, cols, rows, width,
    height."""
    T, cell = int(n_triangles), int(cell)
    if T < 0 or 3 * T > 2 ** 31 - 1:
        raise ValueError("n_triangles: 0 .. (2^31 - 1) / 3")
    if not _lib.ATLAS_MIN_CELL <= cell <= _lib.ATLAS_MAX_CELL:
        raise ValueError(f"cell: {_lib.ATLAS_MIN_CELL} .. {_lib.ATLAS_MAX_CELL} texels")
    cells = max((T + 1) // 2, 1)
    if cols is None:
        cols = math.isqrt(cells - 1) + 1                              # ceil(sqrt(cells)) in integers
    cols = int(cols)
    if cols < 1:
        raise ValueError("cols must be positive")
    rows = (cells + cols - 1) // cols
    if cols * cell * rows * cell > 2 ** 31 - 1:
        raise ValueError(f"an atlas of {cols * cell} x {rows * cell} texels: more than int32 addresses")
    return {"cell": cell, "cols": cols, "rows": rows, "width": cols * cell, "height": rows * cell}


def atlas_uv(layout, n_triangles):
    """(T, 3, 2) fp64 array: where the three corners of every triangle lie in the atlas, (x, y) in texel units (texel
    centres on the integers, row 0 first).  They lie ON texels: (1, 1), (C - 4, 1), (1, C - 4) of the cell in half 0,
    the cell turned by 180 degrees in half 1."""
    C_, cols = int(layout["cell"]), int(layout["cols"])
    tr = np.arange(int(n_triangles))
    k, h = tr // 2, tr % 2
    L = C_ - 5
    local = np.array([[1, 1], [1 + L, 1], [1, 1 + L]], dtype=np.float64)[None, :, :].repeat(len(tr), axis=0)
    local = np.where(h[:, None, None] == 1, (C_ - 1) - local, local)
    origin = np.stack([(k % cols) * C_, (k // cols) * C_], axis=1).astype(np.float64)
    return local + origin[:, None, :]


def bake_texture(mesh, bank, depth_tol, *, cell=16, cols=None, fallback="colors", background=(0.0, 0.0, 0.0),
                 texel_batch=1 << 24, images=None, image_weights=None, min_cos=0.0, weighting="cos", reject=None,
                 batch_pixels=1 << 26):
    """A texture atlas of `mesh` baked from the images of `bank`: every texel of atlas_layout(T, cell, cols) becomes a
    point of its triangle with a normal (nfl_atlas_points), the points are coloured exactly as color_mesh_from_images
    colours vertices -- the same projection, facing and depth tests against the depth maps of the MESH, the same
    bilinear samples and weights, `images`, `image_weights`, `min_cos`, `weighting`, `reject` and `batch_pixels` as
    there -- and the sums become texels (nfl_atlas_resolve).  The definition is written out in include/nerf_fl_amd.h,
    "mesh atlas".  Returns a dict that render_mesh(texture=) and write_obj take:

        texture (H, W, 3) fp32 in [0, 1] where seen; texture_u8 (H, W, 3) uint8 (clamp, x 255, truncate);
        seen (H, W) bool; views (H, W) int32; cell, cols, rows

    fallback     the colour of a texel no image sees: "colors" interpolates the mesh's vertex `colors` (ValueError when it
                 has none), 3 numbers give a flat colour.  With `reject`, a texel seen in the first pass whose samples are
                 all rejected in the second keeps its first-pass colour (and is not `seen`), as a vertex does.
    background   3 numbers: texels of cells and half-cells that no triangle owns.
    texel_batch  texels coloured at a time (each needs 44 bytes of points, normals and sums); the result does not depend
                 on it.  With more than one batch the depth maps are kept between them when they fit in `batch_pixels`.

    No host synchronisation of its own, as color_mesh_from_images."""
    ver, nrm, col, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    depth_tol, min_cos, batch_pixels, runs, weights = _blend_arguments(
        "bake_texture", dev, bank, depth_tol, images, image_weights, min_cos, weighting, reject, batch_pixels)
    lay = atlas_layout(T, cell, cols)
    cell, cols, rows, W, H = (lay[k] for k in ("cell", "cols", "rows", "width", "height"))
    texel_batch = int(texel_batch)
    if texel_batch < 1:
        raise ValueError("texel_batch must be positive")
    vcol, flat = None, [0.0, 0.0, 0.0]
    if isinstance(fallback, str):
        if fallback != "colors":
            raise ValueError("fallback: 'colors' or 3 numbers")
        if col is None:
            raise ValueError("bake_texture: fallback='colors' needs a mesh that has `colors`")
        vcol = col
    else:
        flat = _three(fallback, "fallback: 'colors' or 3 numbers")
    background = _three(background, "background: 3 numbers")
    N = W * H
    walk = _BlendWalk(ver, tri, bank, runs, weights, weighting, min_cos, depth_tol, reject, batch_pixels,
                      keep=reject is not None or N > texel_batch)
    out = {"texture": torch.empty(H, W, 3, dtype=torch.float32, device=dev),
           "texture_u8": torch.empty(H, W, 3, dtype=torch.uint8, device=dev),
           "seen": torch.empty(H, W, dtype=torch.uint8, device=dev),
           "views": torch.empty(H, W, dtype=torch.int32, device=dev)}
    tex, tex8, seen, views = out["texture"].view(N, 3), out["texture_u8"].view(N, 3), out["seen"].view(N), out["views"].view(N)
    n_max = min(N, texel_batch)
    pts, nor = (torch.empty(n_max, 3, dtype=torch.float32, device=dev) for _ in range(2))
    sums = torch.empty(n_max, 4, dtype=torch.float32, device=dev)

    def resolve(first, n, texture, texture_u8, seen_):
        r = _lib.AtlasResolveArgs()
        r.d_triangles, r.n_vertices, r.n_triangles = _ptr(tri), V, T
        r.cell, r.cols, r.rows, r.first_texel, r.n_texels = cell, cols, rows, first, n
        r.d_sum, r.d_views, r.d_vertex_colors = _ptr(sums), _ptr(views[first:first + n]), _ptr(vcol)
        r.fallback[:], r.background[:] = flat, background
        r.d_texture, r.d_texture_u8, r.d_seen = _ptr(texture), _ptr(texture_u8), _ptr(seen_)
        _launch("nfl_atlas_resolve", r)

    with torch.cuda.device(dev):
        for first in range(0, N, texel_batch):
            n = min(texel_batch, N - first)
            a = _lib.AtlasPointsArgs()
            a.d_vertices, a.d_vertex_normals, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(nrm), _ptr(tri), V, T
            a.cell, a.cols, a.rows, a.first_texel, a.n_texels = cell, cols, rows, first, n
            a.d_points, a.d_normals = _ptr(pts), _ptr(nor)
            _launch("nfl_atlas_points", a)
            piece = slice(first, first + n)
            walk.blend(pts[:n], nor[:n], None, sums[:n], views[piece])
            resolve(first, n, tex[piece], tex8[piece], seen[piece])
            if reject is not None:
                first_tex, first_u8 = tex[piece].clone(), tex8[piece].clone()
                walk.blend(pts[:n], nor[:n], first_tex, sums[:n], views[piece])
                resolve(first, n, tex[piece], tex8[piece], seen[piece])
                lost = (seen[piece] == 0)[:, None]                        # all samples rejected: the first pass's colour stays
                tex[piece] = torch.where(lost, first_tex, tex[piece])
                tex8[piece] = torch.where(lost, first_u8, tex8[piece])
    out["seen"] = out["seen"].view(torch.bool)
    return dict(out, cell=cell, cols=cols, rows=rows)
