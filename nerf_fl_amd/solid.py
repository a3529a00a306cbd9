"""The inside of a closed triangle mesh, on the device: how often a ray crosses a mesh, whether a point lies inside it, and what
follows from that one primitive -- a signed distance, the mesh back on a lattice (re-meshing, offsetting), and the volume two
meshes share.

    count_crossings   nfl_mesh_crossings: the number of triangles each of many rays crosses, through the triangle grid of
                      meshdist.triangle_grid or trying every triangle
    inside_mesh       nfl_mesh_inside: the parity of the crossings along K fixed directions, and the majority of them
    signed_distance   closest_on_mesh's distance, negative inside
    solid_lattice     the truncated signed distance at the points of a lattice, in tsdf_lattice's convention: the inverse of
                      extract_surface
    remesh            extract_surface of that lattice: the mesh at a uniform resolution, grown or shrunk by an offset
    volume_overlap    the lattice points inside each of two meshes, inside both and inside either: volumes and IoU
    mesh_volume       the signed volume by the divergence theorem

The definitions are written out in include/nerf_fl_amd.h, "mesh solid"; DESIGN.md section 38.  A mesh is the geometry package's
dict (vertices, normals, triangles on a ROCm device).  Grid mode returns exactly the integers of brute mode.  An OPEN mesh has no
inside: the votes tell how far the directions disagree, and nothing here refuses such a mesh."""
import torch

from . import _lib
from .geometry import extract_surface, lattice_points
from .geometry._call import _call, _f32, _is, _mesh_tensors, _on_device, _positive, _ptr
from .geometry.lattice import _box
from .meshdist import _mesh_or_grid, closest_on_mesh, triangle_grid
from .raycast import _grid_args, _rays

__all__ = ["count_crossings", "inside_mesh", "signed_distance", "solid_lattice", "remesh", "volume_overlap", "mesh_volume"]


def _directions(directions):
    if isinstance(directions, bool) or not isinstance(directions, int) or directions not in range(1, _lib.SOLID_MAX_DIRECTIONS + 1, 2):
        raise ValueError(f"directions: 1, 3, 5 or 7, got {directions!r}")
    return directions


def _points(points, dev):
    _on_device(points)
    if not _is(points, torch.float32, 2, (3,), dev):
        raise ValueError("points: expected a contiguous fp32 (N, 3) tensor on the mesh's device")
    return points.detach()


def count_crossings(rays, mesh_or_grid, method="grid"):
    """The number of triangles of a mesh that every row [o, d, near, far] of `rays` ((R, 8) fp32 on the mesh's device) crosses
    inside [near, far]: an (R,) int32 tensor.  The ray test is cast_rays': both faces cross, the direction need not be
    normalised, far = +inf is served, a ray that can hit nothing counts 0, and every triangle counts at most once.

    mesh_or_grid   a mesh dict, or a meshdist.TriangleGrid to ask one mesh many times;
    method         "grid" walks the grid's cells along the whole ray; "brute" tries every triangle.  Space outside the grid's
                   box is empty; with a TriangleGrid both methods apply that box and return the same integers.

    No host synchronisation when handed a TriangleGrid (or with method="brute"); with a mesh dict, triangle_grid's."""
    ver, tri, grid, rows = _mesh_or_grid(mesh_or_grid, method)
    r = _rays(rays, ver.device)
    count = torch.empty(r.shape[0], dtype=torch.int32, device=ver.device)
    with torch.cuda.device(ver.device):
        _call("nfl_mesh_crossings", _ptr(r), r.shape[0], *_grid_args(ver, tri, grid, rows), _ptr(count))
    return count


def _inside(points, ver, tri, grid, rows, directions):
    """nfl_mesh_inside: (inside (N,) bool, votes (N,) uint8)."""
    dev, N = ver.device, points.shape[0]
    votes = torch.empty(N, dtype=torch.uint8, device=dev)
    flags = torch.empty(N, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _call("nfl_mesh_inside", _ptr(points), N, *_grid_args(ver, tri, grid, rows), directions, _ptr(votes), _ptr(flags))
    return flags != 0, votes


def inside_mesh(points, mesh_or_grid, directions=3, method="grid"):
    """Whether every row of `points` ((N, 3) fp32 on the mesh's device) lies inside a closed mesh: a dict with `inside` (N,) bool
    and `votes` (N,) uint8.  From the point, `directions` (1, 3, 5 or 7) rays run to infinity along the first of seven fixed
    directions, none along a lattice line or a face of an axis-aligned box; a ray with an odd number of crossings votes
    inside, and the majority decides.  On a closed mesh the votes are 0 or `directions` but for rays through an edge or a
    vertex, which the majority absorbs; on an open mesh they say how far the directions disagree.  A point with a
    non-finite coordinate gets votes = 255 and is not inside; a point on the surface gets the side the roundings give.

    mesh_or_grid, method   as count_crossings takes them.  No host synchronisation when handed a TriangleGrid."""
    directions = _directions(directions)
    ver, tri, grid, rows = _mesh_or_grid(mesh_or_grid, method)
    inside, votes = _inside(_points(points, ver.device), ver, tri, grid, rows, directions)
    return {"inside": inside, "votes": votes}


def signed_distance(points, mesh_or_grid, directions=3, max_distance=None, method="grid"):
    """closest_on_mesh's dict (distance, triangle, point, bary) with `distance` negated where the point is inside, plus
    inside_mesh's `inside` and `votes`.  The magnitude has closest_on_mesh's bits.  A query with nothing within `max_distance`
    keeps an infinite distance, -inf inside and +inf outside.  With a mesh dict and method="grid" one grid is built and
    serves both queries."""
    directions = _directions(directions)
    _positive(max_distance, "max_distance: None or a positive number")
    ver, tri, grid, rows = _mesh_or_grid(mesh_or_grid, method)
    target = grid if grid is not None else mesh_or_grid
    out = closest_on_mesh(points, target, max_distance=max_distance, method=method)
    inside, votes = _inside(_points(points, ver.device), ver, tri, grid, rows, directions)
    out["distance"] = torch.where(inside, -out["distance"], out["distance"])
    out.update(inside=inside, votes=votes)
    return out


def _trunc(trunc, sp):
    """The truncation distance: None means 3 x the largest spacing, fuse_mesh's convention."""
    trunc = 3.0 * max(sp) if trunc is None else float(trunc)
    if not trunc > 0.0 or not _f32(trunc) > 0.0 or trunc == float("inf"):
        raise ValueError("trunc: None or a positive finite number")
    return trunc


def _solid_lattice(mesh, lo, hi, res, trunc, directions):
    lo, sp, res = _box(lo, hi, res)
    trunc, directions = _trunc(trunc, sp), _directions(directions)
    ver, _, _, _ = _mesh_tensors(mesh)
    grid = triangle_grid(mesh)                                                # one grid, both queries
    points = lattice_points(lo, hi, res, ver.device).reshape(-1, 3)
    sd = signed_distance(points, grid, directions=directions, max_distance=trunc)
    shape = (res[2], res[1], res[0])
    lattice = (sd["distance"] * (-1.0 / trunc)).clamp_(-1.0, 1.0)           # a query with nothing within trunc: -+inf, then -+1
    return lattice.view(shape), sd["inside"].view(shape), trunc


def solid_lattice(mesh, lo, hi, res, trunc=None, directions=3):
    """A closed mesh back on a lattice: (lattice (nz, ny, nx) fp32, inside (nz, ny, nx) bool) at geometry.lattice_points(lo,
    hi, res), the points density_lattice evaluates and extract_surface places.

        lattice = clamp(signed distance * fp32(-1 / trunc), -1, 1)

    positive inside: tsdf_lattice's convention, so extract_surface(lattice, 0.0, lo, hi) is the mesh again at the lattice's
    resolution, and occupancy_grid, surface_support and everything else that takes a lattice take this one.  `trunc` is the
    truncation distance, None meaning 3 x the largest spacing (fuse_mesh's convention).  The closest point is sought within
    `trunc` only, so a far point costs a shell of cells or two, and holds +1 or -1 by its side.  One triangle grid is built
    and serves the distance and the side.  Host synchronisations: triangle_grid's."""
    lattice, inside, _ = _solid_lattice(mesh, lo, hi, res, trunc, directions)
    return lattice, inside


def remesh(mesh, lo, hi, res, offset=0.0, trunc=None, directions=3):
    """The mesh again, extracted from solid_lattice(mesh, lo, hi, res, trunc, directions) at the level that moves the surface
    OUTWARD by `offset` (inward when negative): a uniform resolution whatever the input's, the union of what overlapped, a
    margin for a MeshBand.  |offset| must stay below `trunc`, beyond which the lattice is flat; a vertex lies within one
    lattice spacing of the offset surface.  Host synchronisations: triangle_grid's and extract_surface's."""
    offset = float(offset)
    _, sp, _ = _box(lo, hi, res)
    if not abs(offset) < _trunc(trunc, sp):
        raise ValueError("offset: its magnitude must stay below trunc")
    lattice, _, trunc = _solid_lattice(mesh, lo, hi, res, trunc, directions)
    return extract_surface(lattice, -offset / trunc, lo, hi)


def volume_overlap(a, b, lo, hi, res, directions=3):
    """How much volume two closed meshes share, counted on the lattice `res` over the box [lo, hi]: a dict with the integers
    `cells_a`, `cells_b`, `intersection` and `union` (lattice points inside a, inside b, inside both, inside either), `iou` =
    intersection / union (NaN when neither mesh holds a point), and `volume_a`, `volume_b`, `volume_intersection` = the
    counts times the cell volume, the product of the three spacings.  The sums are integer sums on the device, exact and the
    same on every run; they leave it in ONE copy, the host read of this function (besides triangle_grid's, per mesh)."""
    _, sp, _ = _box(lo, hi, res)
    directions = _directions(directions)
    dev = _mesh_tensors(a)[0].device
    if _mesh_tensors(b)[0].device != dev:
        raise ValueError("a and b on different devices")
    points = lattice_points(lo, hi, res, dev).reshape(-1, 3)
    in_a, in_b = (inside_mesh(points, m, directions=directions)["inside"] for m in (a, b))
    sums = torch.stack([in_a.sum(), in_b.sum(), (in_a & in_b).sum(), (in_a | in_b).sum()]).cpu()       # THE host read
    ca, cb, both, either = (int(v) for v in sums)
    cell = sp[0] * sp[1] * sp[2]
    return {"cells_a": ca, "cells_b": cb, "intersection": both, "union": either, "iou": both / either if either else float("nan"),
            "volume_a": ca * cell, "volume_b": cb * cell, "volume_intersection": both * cell}


def mesh_volume(mesh):
    """The signed volume of a mesh by the divergence theorem, the sum over its triangles of a . (b x c) / 6 in fp64 (torch): a ()
    fp64 tensor on the mesh's device, so nothing here synchronises; float() reads it.  It is the number the lattice count of
    volume_overlap converges to, and a cheap check of a mesh: positive for a closed mesh wound outward, as extract_surface
    winds, negative for one wound inward, and of no meaning for an open one.  Triangles with an index out of range or a
    non-finite corner add nothing."""
    ver, _, _, tri = _mesh_tensors(mesh)
    V = ver.shape[0]
    if V == 0 or tri.shape[0] == 0:
        return torch.zeros((), dtype=torch.float64, device=ver.device)
    t = tri.long()
    ok = ((t >= 0) & (t < V)).all(dim=1)
    c = ver.double()[t.clamp(0, V - 1)]
    six = (c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum(dim=1)
    return torch.where(ok & torch.isfinite(six), six, torch.zeros_like(six)).sum() / 6.0
