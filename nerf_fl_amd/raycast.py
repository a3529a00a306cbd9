"""Rays against a triangle mesh, on the device: where an arbitrary ray first hits a surface, whether it hits it at all, and
what follows from that one primitive -- ambient occlusion per vertex, and render rays clipped to a band round a surface.

    cast_rays          nfl_mesh_cast: the first hit (t, triangle, corner weights, point) or any hit of many rays, through the
                       triangle grid of meshdist.triangle_grid or trying every triangle
    vertex_occlusion   nfl_mesh_occlusion: the share of the hemisphere over every vertex (or given point) that the mesh leaves
                       open, from cosine-weighted any-hit rays
    clip_rays_to_mesh  the near and far of render rays tightened to t -+ band / |d| round their first hit
    MeshBand           a grid and a band, which eval.clipped_inference and eval.render_frame take where they take an
                       OccupancyGrid

The definitions are written out in include/nerf_fl_amd.h, "mesh cast"; DESIGN.md section 36.  A mesh is the geometry package's
dict (vertices, normals, triangles on a ROCm device); a ray is a row [o, d, near, far] of an fp32 (R, 8) matrix, as the
renderer takes them, and t is in the ray's own parameter.  Grid mode returns exactly the bits of brute mode."""
import math

import torch

from . import _lib
from .geometry._call import _call, _f32, _is, _mesh_tensors, _on_device, _positive, _ptr, _seed
from .meshdist import TriangleGrid, _mesh_or_grid, triangle_grid

__all__ = ["cast_rays", "vertex_occlusion", "clip_rays_to_mesh", "MeshBand"]

MAX_RAYS_PER_POINT = 4096                # NC_MAX_DIRECTIONS


def _grid_args(ver, tri, grid, rows):
    """The mesh and grid arguments both entry points share, in the header's order."""
    if grid is None:
        return (_ptr(ver), _ptr(tri), ver.shape[0], tri.shape[0], None, None, 0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0)
    off, ent = (grid.offsets, grid.entries) if rows else (None, None)
    return (_ptr(ver), _ptr(tri), ver.shape[0], tri.shape[0], _ptr(off), _ptr(ent), grid.entries.shape[0] if rows else 0,
            *grid.lo, grid.cell, *grid.dims)


def _rays(rays, dev):
    _on_device(rays)
    if not _is(rays, torch.float32, 2, (8,), contiguous=False):
        raise ValueError("rays: expected an fp32 (R, 8) tensor")
    if rays.device != dev:
        raise ValueError("rays and mesh on different devices")
    return rays.detach().contiguous()


def cast_rays(rays, mesh_or_grid, mode="first", method="grid"):
    """Cast every row [o, d, near, far] of `rays` ((R, 8) fp32 on the mesh's device) against a mesh.

    mode="first"   a dict: `t` (R,) fp32, the parameter of the first hit inside [near, far] (+inf on a miss), `triangle` (R,)
                   int32 (-1), `bary` (R, 3), the weights of the triangle's three corners as closest_on_mesh returns them,
                   and `point` (R, 3), the hit point (NaN on a miss).  Among hits at the same t the lowest triangle answers;
    mode="any"     a dict: `t` (0 for a ray that hits anything, +inf otherwise) and `hit` (R,) bool: cheaper, the walk stops
                   at the first hit it finds -- shadow rays, visibility of a point from a point;
    mesh_or_grid   a mesh dict, or a meshdist.TriangleGrid to cast against one mesh many times;
    method         "grid" walks the grid's cells along the ray; "brute" tries every triangle.  Both faces of a triangle hit.
                   Space outside the grid's box is empty: with a TriangleGrid, "brute" applies the same box, so both methods
                   answer the same question and return the same bits; "brute" with a mesh dict has no box.

    The direction need not be normalised.  A ray with a non-finite origin or direction, a NaN bound, a zero direction or
    near > far hits nothing.  No host synchronisation when handed a TriangleGrid (or with method="brute"); with a mesh
    dict, triangle_grid's."""
    if mode not in _lib.CAST_MODES:
        raise ValueError(f"mode: 'first' or 'any', got {mode!r}")
    ver, tri, grid, rows = _mesh_or_grid(mesh_or_grid, method)
    dev = ver.device
    r = _rays(rays, dev)
    R = r.shape[0]
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
    out = {"t": new(R)}
    if mode == "first":
        out.update(triangle=new(R, dtype=torch.int32), bary=new(R, 3), point=new(R, 3))
    with torch.cuda.device(dev):
        _call("nfl_mesh_cast", _ptr(r), R, *_grid_args(ver, tri, grid, rows), _lib.CAST_MODES[mode], _ptr(out["t"]),
              _ptr(out.get("triangle")), _ptr(out.get("bary")), _ptr(out.get("point")))
    if mode == "any":
        out["hit"] = out["t"] == 0
    return out


def _occlusion(points, normals, grid, rays, radius, bias, seed):
    """nfl_mesh_occlusion: (hits (N,) int32, open (N,) fp32)."""
    dev, N = points.device, points.shape[0]
    hits = torch.empty(N, dtype=torch.int32, device=dev)
    opn = torch.empty(N, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _call("nfl_mesh_occlusion", _ptr(points), _ptr(normals), N, *_grid_args(grid.vertices, grid.triangles, grid, True), rays,
              radius, bias, seed, _ptr(hits), _ptr(opn))
    return hits, opn


def vertex_occlusion(mesh, rays=64, radius=None, bias=None, seed=0, grid=None, points=None, normals=None):
    """Ambient occlusion: the openness in [0, 1] of every vertex of `mesh` ((V,) fp32), or of the given `points` with their
    unit `normals` ((N, 3) fp32 each).  From p + bias * n, `rays` (1 .. 4096) directions are drawn cosine-weighted about the
    normal (hashed from the seed, the point and the ray: the same seed gives the same bits) and cast in any-hit mode;
    openness = the share that hits nothing within `radius`.  1 is open sky, 0 a sealed hole.  A point or normal that is not
    finite, or a zero normal (a vertex no triangle uses), gives NaN.

    radius   None: no limit inside the grid's box (space outside it is empty);
    bias     None: 1e-3 of the grid's cell.  A small fraction of the feature size is the usual practice and NOT a measured
             choice: it must clear the rounding of the vertex's own triangles (so that they do not shadow it) and stay below
             the features that should;
    grid     the mesh's meshdist.TriangleGrid, to reuse one; None builds it (triangle_grid's synchronisations, else none).

    The intended use is to darken what the mesh renderer draws, or what a file carries:
        openness = vertex_occlusion(mesh)
        render_mesh(mesh, ..., colors=colors * openness[:, None])
        write_ply(path, mesh, colors * openness[:, None])"""
    if isinstance(rays, bool) or int(rays) != rays or not 1 <= rays <= MAX_RAYS_PER_POINT:
        raise ValueError(f"rays: an integer in [1, {MAX_RAYS_PER_POINT}]")
    radius = _positive(radius, "radius: None or a positive number")
    if bias is not None and not (float(bias) >= 0.0 and math.isfinite(_f32(bias))):
        raise ValueError("bias: None or a finite number, not negative")
    seed = _seed(seed, "seed: an integer in [0, 2^64)")
    if (points is None) != (normals is None):
        raise ValueError("points and normals come together")
    if grid is not None and not isinstance(grid, TriangleGrid):
        raise ValueError("grid: what meshdist.triangle_grid returns")
    ver, nrm, _, _ = _mesh_tensors(mesh)
    dev = ver.device
    if points is None:
        points, normals = ver, nrm
    else:
        _on_device(points, normals)
        if not (_is(points, torch.float32, 2, (3,), dev) and _is(normals, torch.float32, 2, tuple(points.shape), dev)):
            raise ValueError("points, normals: expected contiguous fp32 (N, 3) tensors on the mesh's device")
    if grid is None:
        grid = triangle_grid(mesh)
    elif grid.vertices.device != dev:
        raise ValueError("grid and mesh on different devices")
    bias = 1e-3 * grid.cell if bias is None else float(bias)
    return _occlusion(points.detach(), normals.detach(), grid, int(rays), radius, bias, seed)[1]


def clip_rays_to_mesh(mesh_or_grid, rays, band):
    """Tighten render rays to a band round a surface.  Returns (rays', hit) with the contract of geometry.clip_rays: rays' is a
    copy of `rays` ((R, 8) fp32) whose columns 6 and 7 hold, for a ray whose first hit lies at t,
        near' = max(near, t - band / |d|)        far' = min(far, t + band / |d|)
    (`band` is a distance in space, t the ray's own parameter), and the ray's own near and far when it misses; hit (R,) bool
    tells the two apart.  Only the FIRST surface a ray meets gets a band.  Space outside the grid's box is empty.
    Everything after the cast is torch elementwise work: no host synchronisation when handed a TriangleGrid."""
    band = float(band)
    if not (band >= 0.0 and math.isfinite(band)):
        raise ValueError("band: a finite distance, not negative")
    t = cast_rays(rays, mesh_or_grid)["t"]
    out = rays.detach().clone(memory_format=torch.contiguous_format)
    hit = torch.isfinite(t)
    near, far = out[:, 6], out[:, 7]
    w = band / out[:, 3:6].norm(dim=1)
    out[:, 6] = torch.where(hit, torch.maximum(near, t - w), near)
    out[:, 7] = torch.where(hit, torch.minimum(far, t + w), far)
    return out, hit


class MeshBand:
    """A surface and a band round it, for rendering: `grid` (a meshdist.TriangleGrid, or a mesh dict, whose grid is built here)
    and `band`, a distance.  clip(rays) is clip_rays_to_mesh; eval.clipped_inference(..., grid=) and eval.render_frame(...,
    occupancy=) take a MeshBand where they take an OccupancyGrid, and then render only between t -+ band / |d| of the pixels
    that see the surface.  A mesh from extract_mesh or fuse_mesh is the surface itself, where an occupancy grid is a cell
    thick at best; what the field holds outside the band -- a second surface behind the first, a haze -- is not rendered."""

    def __init__(self, grid, band):
        band = float(band)
        if not (band >= 0.0 and math.isfinite(band)):
            raise ValueError("band: a finite distance, not negative")
        self.grid = grid if isinstance(grid, TriangleGrid) else triangle_grid(grid)
        self.band = band

    def clip(self, rays):
        return clip_rays_to_mesh(self.grid, rays, self.band)
