"""Geometry out of a trained field: the static density on a lattice, its iso-surface as an indexed mesh, a PLY file.

    density_lattice   static sigma on a regular lattice, through the fused render kernel (no encoded points in memory)
    extract_surface   marching tetrahedra on the device (csrc/nfl_surface.hip): welded vertices, normals, triangles
    surface_colors    static rgb at the vertices, seen along -normal
    write_ply         binary little-endian PLY (numpy only)
    mesh_components   connected components of a mesh and their table, on the device (csrc/nfl_mesh.hip)
    filter_mesh       the mesh of the components a keep flag names: vertices, normals, colours, re-indexed triangles
    clean_mesh        keep by size, rank or bounding box (the floaters of an in-the-wild field go here)
    simplify_mesh     the same surface with fewer triangles: uniform vertex clustering on the device (csrc/nfl_simplify.hip)
    mesh_adjacency    the neighbours and the incident triangle corners of every vertex, sorted, and the boundary flags (csrc/nfl_meshsmooth.hip)
    smooth_mesh       Laplacian / Taubin smoothing over that adjacency, normals recomputed from the triangles
    vertex_normals    vertex normals from the triangles alone, area- or uniformly weighted
    extract_mesh      all of it in a row
    occupancy_grid    one bit per cell of a lattice: occupied where a corner reaches a threshold, dilated (csrc/nfl_occupancy.hip)
    clip_rays         rays walked through such a grid: a tightened [near, far] per ray and a flag for rays that hit nothing
    mesh_depth        the depth map of a mesh seen by a camera: a z-buffer on the device (csrc/nfl_meshcolor.hip)
    color_mesh_from_images   vertex colours from the images of an ImageBank that see each vertex, hidden views left out
    mesh_visibility   which triangle a camera sees at every pixel, and how far: a visibility buffer (csrc/nfl_meshrender.hip)
    render_mesh       a coloured mesh as an image: vertex colours, normals or a headlight interpolated at the winning triangles
    atlas_layout      the texture atlas of a mesh: a chart per triangle, two to a square cell (csrc/nfl_atlas.hip)
    bake_texture      such an atlas filled from the images of an ImageBank; render_mesh(texture=) samples it
    write_obj         OBJ + MTL + PNG of a mesh and its atlas (numpy and Pillow)

Conventions: `lo`, `hi` and `res` are 3 numbers in (x, y, z) order; a lattice is a (nz, ny, nx) fp32 tensor, x fastest,
whose point (x, y, z) lies at lo + (x, y, z) * spacing with spacing = (hi - lo) / (res - 1): `lattice_points` returns
exactly the fp32 positions both the field pass and the extraction use.  A point is inside the surface when its value is
>= iso.  The definition of the extraction (split, order, formulae) is written out in include/nerf_fl_amd.h.

There is no CPU path.

The package is cut by stage: lattice.py (the field on a lattice and its surface), occupancy.py, mesh.py (a mesh worked
on as a mesh), images.py (a mesh and cameras), files.py (the writers); _call.py holds what they all call.
"""
import torch

from .files import write_obj, write_ply
from .images import (atlas_layout, atlas_uv, bake_texture, color_mesh_from_images, mesh_depth, mesh_visibility,
                     render_mesh)
from .lattice import density_lattice, extract_surface, lattice_points, surface_colors
from .mesh import (clean_mesh, filter_mesh, mesh_adjacency, mesh_components, simplify_mesh, smooth_mesh,
                   vertex_normals)
from .occupancy import OccupancyGrid, clip_rays, occupancy_grid
from .lattice import _box                                             # the checks extract_mesh makes ahead of its stages
from .mesh import _simplify_arguments, _smooth_arguments

__all__ = ["density_lattice", "extract_surface", "surface_colors", "write_ply", "extract_mesh", "lattice_points",
           "mesh_components", "filter_mesh", "clean_mesh", "simplify_mesh", "mesh_adjacency", "smooth_mesh",
           "vertex_normals", "OccupancyGrid", "occupancy_grid", "clip_rays",
           "mesh_depth", "color_mesh_from_images", "mesh_visibility", "render_mesh", "atlas_layout", "atlas_uv",
           "bake_texture", "write_obj"]


def extract_mesh(models, embeddings, lo, hi, res, iso, chunk=1 << 20, a_embedded=None, path=None, largest=None,
                 min_triangles=None, simplify=None, placement="mean", color_from=None, depth_tol=None, color_kwargs=None,
                 texture=None, smooth=None, smooth_kwargs=None):
    """density_lattice -> extract_surface -> surface_colors (-> write_ply when `path` is given) for the fine model of
    `models` (the coarse one when there is no fine one).  Returns the mesh dict with `colors` (V, 3) added.

    With `color_from` = a data.ImageBank the colours come from the images that see the surface
    (color_mesh_from_images, after cleaning and simplifying; `color_kwargs` are passed on to it) and the mesh also gets
    `seen` (V,) bool.  surface_colors is then the fallback for the vertices no image sees, unless the model encodes
    appearance and no `a_embedded` is given, when they stay grey.  `depth_tol` = None means twice the largest lattice
    spacing: that is the usual practice and not a measured choice (the extracted surface lies within a cell of the
    field's, and a vertex should not lose its own views to that).

    With `largest` or `min_triangles` (as in clean_mesh) the small components are dropped BEFORE the colour pass, so the
    field is never evaluated at a discarded vertex.

    With `simplify` = a cell size the cleaned mesh goes through simplify_mesh (origin = `lo`, `placement` as there), also
    before the colour pass: the field is evaluated at the simplified vertices only, seen along their new normals.

    With `smooth` = a number of iterations the cleaned mesh goes through smooth_mesh (`smooth_kwargs`: its lam, mu,
    boundary and normals) BEFORE it is simplified and coloured, so that the quadric placement and the colour pass see the
    smoothed surface and its recomputed normals.

    With `texture` = a cell size (and `color_from`) a texture atlas is baked from the same bank after the vertex colours
    exist (bake_texture with the `color_kwargs` that apply to it; the vertex colours are its fallback); the mesh gets
    `atlas`, and `path` is then written as an OBJ set (write_obj) instead of a PLY."""
    if texture is not None:
        if color_from is None:
            raise ValueError("extract_mesh: texture= bakes from the images; give color_from")
        atlas_layout(0, texture)                                          # refused before anything is evaluated
    if simplify is not None:
        _simplify_arguments(simplify, lo, placement)                      # refused before anything is evaluated
    if smooth is not None:                                                # refused before anything is evaluated
        smooth_kwargs = dict(smooth_kwargs or {})
        if set(smooth_kwargs) - {"lam", "mu", "boundary", "normals"}:
            raise ValueError(f"smooth_kwargs: lam, mu, boundary and normals, got {sorted(smooth_kwargs)}")
        _smooth_arguments(smooth, *(smooth_kwargs.get(k, d) for k, d in (("lam", 0.5), ("mu", -0.53), ("boundary", "fixed"),
                                                                         ("normals", "area"))))
    model = models["fine"] if "fine" in models else models["coarse"]
    lattice = density_lattice(model, embeddings, lo, hi, res, chunk=chunk)
    mesh = extract_surface(lattice, iso, lo, hi)
    mesh = clean_mesh(mesh, largest=largest, min_triangles=min_triangles)
    if smooth is not None:
        mesh = smooth_mesh(mesh, smooth, **smooth_kwargs)
    if simplify is not None:
        mesh = simplify_mesh(mesh, simplify, origin=lo, placement=placement)
    if mesh["vertices"].shape[0] == 0 and not (largest is None and min_triangles is None and simplify is None):
        mesh["colors"] = torch.empty_like(mesh["vertices"])               # the filter kept nothing: nothing to colour
        if color_from is not None:
            mesh["seen"] = torch.zeros(0, dtype=torch.bool, device=mesh["vertices"].device)
    elif color_from is None:
        mesh["colors"] = surface_colors(model, embeddings, mesh["vertices"], mesh["normals"], a_embedded=a_embedded)
    else:
        fallback = None
        if a_embedded is not None or not model.encode_appearance:
            fallback = surface_colors(model, embeddings, mesh["vertices"], mesh["normals"], a_embedded=a_embedded)
        if depth_tol is None:
            depth_tol = 2.0 * max(_box(lo, hi, res)[1])
        got = color_mesh_from_images(mesh, color_from, depth_tol, **dict({"fallback": fallback}, **(color_kwargs or {})))
        mesh["colors"], mesh["seen"] = got["colors"], got["seen"]
        if texture is not None:
            kw = {k: v for k, v in (color_kwargs or {}).items() if k != "fallback"}
            mesh["atlas"] = bake_texture(mesh, color_from, depth_tol, cell=texture, fallback="colors", **kw)
    if path is not None and mesh.get("atlas") is not None:
        write_obj(path, mesh, mesh["atlas"])
    elif path is not None:
        write_ply(path, mesh, mesh["colors"])
    return mesh
