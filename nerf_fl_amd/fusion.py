"""Depth fusion: the surface the cameras SEE, instead of a level set of the density.  A depth map is rendered from every
camera of an ImageBank, the maps are fused into a truncated signed distance function (TSDF) on a lattice, and the surface
is that function's zero set, without the faces that stand on lattice points no camera has observed.

    fuse_mesh        the whole route: depth_maps -> fuse_depth per run, tsdf_lattice, extract_surface, drop_unsupported, clean_mesh
    depth_maps       depth and weight of a run of the bank's images, rendered through the inference path
    fuse_depth       nfl_tsdf_fuse: a run of depth maps into the accumulators (any depth maps: geometry.mesh_depth's too)
    tsdf_lattice     nfl_tsdf_resolve: the accumulators as a lattice and its observed flags
    surface_support  nfl_tsdf_support: which vertices of a surface stand on observed lattice points only
    drop_unsupported the surface without the others

The definitions are written out in include/nerf_fl_amd.h, "depth fusion"; DESIGN.md section 32.  Conventions are the geometry
package's: boxes and lattices in (x, y, z) order, lattices (nz, ny, nx) fp32 on the device, depths measured from the camera
centre.  The result of fuse_mesh is a mesh dict: color_mesh_from_images, smooth_mesh, simplify_mesh and bake_texture of
nerf_fl_amd.geometry take it as it is."""
import torch

from . import _lib
from .geometry import clean_mesh, extract_surface, filter_mesh
from .geometry._call import _is, _launch, _mesh_tensors, _on_device, _ptr
from .geometry.images import _image_runs
from .geometry.lattice import _box

__all__ = ["depth_maps", "fuse_depth", "tsdf_lattice", "surface_support", "drop_unsupported", "fuse_mesh"]


def _bank_on_device(what, bank):
    if getattr(bank, "device", None) is None or getattr(bank, "table", None) is None:
        raise ValueError(f"{what}: `bank` is a data.ImageBank on a ROCm device")
    return bank.device


def _run(bank, first, count):
    """(first, count, pixels) of the run first .. first + count - 1 of `bank`, checked."""
    first = int(first)
    count = bank.n_images - first if count is None else int(count)
    if first < 0 or count < 0 or first + count > bank.n_images:
        raise ValueError(f"first, count: a run inside the bank's {bank.n_images} images")
    t = bank.host_table
    return first, count, sum(int(t[i]["width"]) * int(t[i]["height"]) for i in range(first, first + count))


def _words(t, n, what, dev):
    """`t` as the (n,) fp32 words of a run on `dev`: any shape with n elements, contiguous."""
    _on_device(t)
    if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous() or t.device != dev:
        raise ValueError(f"{what}: expected a contiguous fp32 tensor of the run's {n} pixels on {dev}")
    return t.detach().view(n)


def fuse_depth(bank, depth, lo, hi, res, trunc, *, first=0, count=None, pixel_weights=None, image_weights=None, into=None):
    """Fuse the depth maps of images first .. first + count - 1 of `bank` (a data.ImageBank on a device; only its cameras
    are read) into the TSDF accumulators of the lattice `res` = (nx, ny, nz) over the box [lo, hi] (nfl_tsdf_fuse).

    depth          fp32, the run's pixels back to back (any shape): per pixel the distance from the camera centre to the
                   surface along the pixel's ray, +inf where the ray hits nothing (the lattice points along it are then
                   free space), NaN or <= 0 where nothing is known.  geometry.mesh_depth and depth_maps give this.
    trunc          the truncation distance, world units, positive: a point further than this behind a depth is hidden
                   and takes nothing from that image; in front of it the signed distance saturates at -trunc.
    pixel_weights  fp32 like `depth`, or None for 1: a pixel's weight; <= 0 or NaN drops the pixel.
    image_weights  (n_images,) fp32, indexed by the bank's image number, or None for 1; <= 0 or NaN drops the image.
    into           the dict an earlier call returned: its accumulators are continued (same box, res and trunc, or
                   ValueError), so a bank may be fused run by run; the result does not depend on the split.

    Returns a dict: acc (nz, ny, nx, 2) fp32 (sum of w * phi, sum of w), views (nz, ny, nx) int32, lo, hi, res, trunc.
    With `into` it is that dict, updated in place.  No host synchronisation."""
    dev = _bank_on_device("fuse_depth", bank)
    lo, sp, res = _box(lo, hi, res)
    hi = [float(h) for h in hi]                                       # three finite numbers: _box has looked
    nx, ny, nz = res
    if nx * ny * nz > 1 << 30 or ny > 65535 or nz > 65535:
        raise ValueError(f"lattice {nx} x {ny} x {nz}: at most 2^30 points, and 65535 rows and planes")
    trunc = float(trunc)
    if not trunc > 0.0:
        raise ValueError("trunc: a positive number")
    first, count, pixels = _run(bank, first, count)
    depth = _words(depth, pixels, "depth", dev)
    if pixel_weights is not None:
        pixel_weights = _words(pixel_weights, pixels, "pixel_weights", dev)
    if image_weights is not None:
        image_weights = torch.as_tensor(image_weights, dtype=torch.float32, device=dev).detach().contiguous()
        if image_weights.shape != (bank.n_images,):
            raise ValueError(f"image_weights: expected ({bank.n_images},)")
    if into is None:
        out = {"acc": torch.empty(nz, ny, nx, 2, dtype=torch.float32, device=dev),
               "views": torch.empty(nz, ny, nx, dtype=torch.int32, device=dev),
               "lo": lo, "hi": hi, "res": res, "trunc": trunc}
    else:
        out = into
        _accumulators(out, dev)
        if (out["lo"], out["hi"], out["res"], out["trunc"]) != (lo, hi, res, trunc):
            raise ValueError("into: accumulators of another box, res or trunc")
    a = _lib.TsdfFuseArgs()
    a.d_table, a.n_images, a.first, a.count, a.start = _ptr(bank.table), bank.n_images, first, count, int(into is None)
    a.d_depth, a.n_depth, a.d_pixel_weights, a.d_image_weights = _ptr(depth), pixels, _ptr(pixel_weights), _ptr(image_weights)
    a.nx, a.ny, a.nz, a.trunc = nx, ny, nz, trunc
    a.lo[:], a.spacing[:] = lo, sp
    a.d_acc, a.d_views = _ptr(out["acc"]), _ptr(out["views"])
    with torch.cuda.device(dev):
        _launch("nfl_tsdf_fuse", a)
    return out


def _accumulators(acc, dev=None):
    """(acc, views, nx, ny, nz) of the dict fuse_depth returns, checked."""
    try:
        sums, views = acc["acc"], acc["views"]
        nx, ny, nz = acc["res"]
    except (TypeError, KeyError, ValueError):
        raise ValueError("accumulators: the dict fuse_depth returns (acc, views, lo, hi, res, trunc)") from None
    _on_device(sums, views)
    if not _is(sums, torch.float32, 4, (nz, ny, nx, 2), dev) or not _is(views, torch.int32, 3, (nz, ny, nx), sums.device):
        raise ValueError(f"accumulators: acc fp32 ({nz}, {ny}, {nx}, 2) and views int32 ({nz}, {ny}, {nx}), contiguous, on one device")
    return sums, views, nx, ny, nz


def tsdf_lattice(acc, min_weight=0.5, min_views=1, fill=-1.0):
    """The accumulators of fuse_depth as a lattice (nfl_tsdf_resolve): returns (lattice (nz, ny, nx) fp32, known (nz, ny, nx)
    uint8).  A point is KNOWN when its weights sum to at least `min_weight` (positive) over at least `min_views` (>= 1)
    images; its value is then the weighted mean of phi = (distance to the camera - depth) / trunc clamped to [-1, 1]:
    positive behind the surface, the inside of extract_surface(lattice, 0.0, lo, hi).  Every other point holds `fill`
    (default -1: free space, so that extract_surface closes the observed band -- drop_unsupported takes that wall away
    again).  The default min_weight, half an image's weight, is a convention.  No host synchronisation."""
    sums, views, nx, ny, nz = _accumulators(acc)
    dev = sums.device
    min_weight, min_views, fill = float(min_weight), int(min_views), float(fill)
    if not min_weight > 0.0:
        raise ValueError("min_weight: a positive number")
    if min_views < 1:
        raise ValueError("min_views: at least 1")
    if fill != fill:
        raise ValueError("fill: a number, not NaN")
    lattice = torch.empty(nz, ny, nx, dtype=torch.float32, device=dev)
    known = torch.empty(nz, ny, nx, dtype=torch.uint8, device=dev)
    a = _lib.TsdfResolveArgs()
    a.d_acc, a.d_views, a.nx, a.ny, a.nz, a.min_views = _ptr(sums), _ptr(views), nx, ny, nz, min_views
    a.min_weight, a.fill, a.d_lattice, a.d_known = min_weight, fill, _ptr(lattice), _ptr(known)
    with torch.cuda.device(dev):
        _launch("nfl_tsdf_resolve", a)
    return lattice, known


def surface_support(mesh, known, lo, hi):
    """(V,) bool: which vertices of `mesh` (extract_surface of a fused lattice over the box [lo, hi]) stand on observed
    lattice points only (nfl_tsdf_support).  A vertex lies on a lattice edge -- an axis edge, a face diagonal or a body
    diagonal -- and is supported when `known` ((nz, ny, nx) uint8 or bool, tsdf_lattice's) holds at every lattice point
    of that edge's segment, face or cell.  No host synchronisation."""
    ver = _mesh_tensors(mesh)[0]
    dev, V = ver.device, ver.shape[0]
    _on_device(known)
    if known.dtype == torch.bool:
        known = known.view(torch.uint8)
    if not _is(known, torch.uint8, 3, device=dev):
        raise ValueError("known: expected a contiguous uint8 or bool (nz, ny, nx) tensor on the mesh's device")
    nz, ny, nx = known.shape
    lo, sp, _ = _box(lo, hi, (nx, ny, nz))
    support = torch.empty(V, dtype=torch.uint8, device=dev)
    a = _lib.TsdfSupportArgs()
    a.d_vertices, a.n_vertices, a.d_known, a.nx, a.ny, a.nz = _ptr(ver), V, _ptr(known), nx, ny, nz
    a.lo[:], a.spacing[:] = lo, sp
    a.d_support = _ptr(support)
    with torch.cuda.device(dev):
        _launch("nfl_tsdf_support", a)
    return support.view(torch.bool)


def drop_unsupported(mesh, known, lo, hi):
    """`mesh` without its unsupported vertices (surface_support) and without the triangles that name one: filter_mesh
    with every vertex a component of its own.  ONE host synchronisation, filter_mesh's."""
    support = surface_support(mesh, known, lo, hi)
    V = support.shape[0]
    own = {"component": torch.arange(V, dtype=torch.int32, device=support.device), "n_components": V}
    return filter_mesh(mesh, support, components=own)


@torch.no_grad()
def depth_maps(models, embeddings, bank, first, count, N_samples, N_importance, *, opaque=0.9, empty=0.1, **render_kwargs):
    """Depth and weight of images first .. first + count - 1 of `bank`, as fuse_depth takes them: (depth, pixel_weights),
    fp32, the run's pixels back to back.  Every image is rendered from its record's camera through the inference path
    (eval.batched_inference at test time, N_samples + N_importance samples, ts = the image's id) with
    output_transient=False, so the depth is the STATIC scene's; `render_kwargs` (chunk, white_back -- default: the
    bank's --, use_disp, ...) go there.

        depth = depth_fine   where opacity_fine >= opaque: the ray ends on a surface;
                +inf         where opacity_fine <= empty: the ray hit nothing, the space along it is free;
                NaN          between: nothing is known, and fuse_depth leaves the pixel out;
        pixel_weights = opacity_fine.

    The two thresholds are CONVENTIONS: nobody has measured them against a scene.  What they stand for is that a
    composited depth is a mean over the ray, and means the surface only when the weights sum to nearly 1."""
    from . import eval as ev
    dev = _bank_on_device("depth_maps", bank)
    first, count, pixels = _run(bank, first, count)
    opaque, empty = float(opaque), float(empty)
    if not 0.0 <= empty < opaque <= 1.0:
        raise ValueError("opaque, empty: 0 <= empty < opaque <= 1")
    if int(N_importance) < 1:
        raise ValueError("depth_maps: the depth is the fine model's; N_importance must be positive")
    kw = dict(render_kwargs)
    kw.setdefault("white_back", bank.white_back)
    kw["output_transient"] = False
    depth = torch.empty(pixels, dtype=torch.float32, device=dev)
    weights = torch.empty(pixels, dtype=torch.float32, device=dev)
    inf = torch.full((), float("inf"), dtype=torch.float32, device=dev)
    nan = torch.full((), float("nan"), dtype=torch.float32, device=dev)
    at = 0
    for i in range(first, first + count):
        rec = bank.host_table[i]
        H, W = int(rec["height"]), int(rec["width"])
        c2w = torch.from_numpy(rec["c2w"].reshape(3, 4).copy())
        K = torch.tensor([[float(rec["fx"]), 0.0, float(rec["cx"])], [0.0, float(rec["fy"]), float(rec["cy"])], [0.0, 0.0, 1.0]])
        cam = ev.CameraRays(c2w, K, H, W, float(rec["near"]), float(rec["far"]), dev)
        ts = torch.full((H * W,), int(rec["id"]), dtype=torch.long, device=dev)
        res = ev.batched_inference(models, embeddings, cam, ts, N_samples, N_importance, **kw)
        d, o = res["depth_fine"], res["opacity_fine"]
        depth[at:at + H * W] = torch.where(o >= opaque, d, torch.where(o <= empty, inf, nan))
        weights[at:at + H * W] = o
        at += H * W
    return depth, weights


def fuse_mesh(models, embeddings, bank, lo, hi, res, *, N_samples=64, N_importance=64, trunc=None, images=None,
              image_weights=None, run_pixels=1 << 24, min_weight=0.5, min_views=1, opaque=0.9, empty=0.1, largest=None,
              min_triangles=1, **render_kwargs):
    """The surface the images of `bank` see, from the fields `models`: the bank is walked in runs of consecutive images of
    at most `run_pixels` pixels (an image larger than that is a run of its own), each run through depth_maps and
    fuse_depth, so the device holds the depth and weight of one run at a time; then tsdf_lattice,
    extract_surface(lattice, 0.0, lo, hi), drop_unsupported and clean_mesh(largest, min_triangles).  The result does not
    depend on `run_pixels`.

    res            (nx, ny, nz) lattice points over the box [lo, hi].
    trunc          the truncation distance; None means 3 x the largest spacing.  That is a convention: the band has to be
                   a few cells wide for the zero crossing to be interpolated between observed points, and 3 and 4 cells
                   both gave a closed surface within one spacing of an analytic sphere.
    images         indices of the images to use (default all).
    image_weights, min_weight, min_views, opaque, empty, N_samples, N_importance, render_kwargs: as fuse_depth,
                   tsdf_lattice and depth_maps take them.
    largest, min_triangles: clean_mesh's criteria; the default drops the vertices the filter left without a triangle.

    Returns the mesh dict (vertices, normals, triangles) plus `lattice` and `known`.  Colouring, smoothing, simplifying
    and texturing are the caller's next calls: color_mesh_from_images, smooth_mesh, simplify_mesh and bake_texture take
    the result.  Host synchronisations: extract_surface's, filter_mesh's and clean_mesh's."""
    dev = _bank_on_device("fuse_mesh", bank)
    lo, sp, res = _box(lo, hi, res)
    if trunc is None:
        trunc = 3.0 * max(sp)
    run_pixels = int(run_pixels)
    if run_pixels < 1:
        raise ValueError("run_pixels must be positive")
    if not float(trunc) > 0.0:
        raise ValueError("trunc: a positive number")
    acc = None
    for first, count, _ in _image_runs(bank, images, run_pixels):
        depth, weights = depth_maps(models, embeddings, bank, first, count, N_samples, N_importance, opaque=opaque,
                                    empty=empty, **render_kwargs)
        acc = fuse_depth(bank, depth, lo, hi, res, trunc, first=first, count=count, pixel_weights=weights,
                         image_weights=image_weights, into=acc)
    if acc is None:
        raise ValueError("fuse_mesh: no image selected")
    lattice, known = tsdf_lattice(acc, min_weight=min_weight, min_views=min_views)
    mesh = drop_unsupported(extract_surface(lattice, 0.0, lo, hi), known, lo, hi)
    mesh = clean_mesh(mesh, largest=largest, min_triangles=min_triangles)
    return dict(mesh, lattice=lattice, known=known)
