"""The distance between two triangle meshes, geometry against geometry: how far a simplification or a smoothing moved a
surface, how far apart the density level set and the depth-fusion surface of one field are, how close an extracted mesh is
to a ground-truth one (Chamfer distance, Hausdorff distance, F-score: what reconstruction papers report).

    triangle_grid    nfl_trigrid_count / _emit: a uniform grid of triangle lists over a mesh
    closest_on_mesh  nfl_mesh_closest: the closest point of a mesh for many queries, through the grid or trying every triangle
    sample_surface   nfl_mesh_sample_count / _emit: area-weighted random points of a surface, with their triangles and normals
    mesh_distance    both directions between two meshes, reduced on the device (nfl_meshdist_reduce), as plain numbers
    read_ply         what write_ply writes, and the plain variants ground-truth meshes come in, back as a mesh dict
                     (geometry/files.py, beside write_ply; this module is where it is public)

The definitions are written out in include/nerf_fl_amd.h, "mesh distance"; DESIGN.md section 33.  A mesh is the geometry
package's dict (vertices, normals, triangles on a ROCm device); grid mode returns exactly the bits of brute mode."""
import math

import numpy as np
import torch

from . import _lib
from .geometry._call import (_count, _f32, _is, _launch, _mesh_tensors, _on_device, _positive, _ptr, _refuse_outside,
                             _scratch, _seed)
from .geometry.files import read_ply

__all__ = ["triangle_grid", "closest_on_mesh", "sample_surface", "mesh_distance", "read_ply"]

MAX_CELLS = 1 << 30                      # NG_MAX_POINTS
MAX_DIM = 65535
DEFAULT_MAX_CELLS = 1 << 24              # what the default cell is raised to stay under
INT32_MAX = 2 ** 31 - 1


class TriangleGrid:
    """A uniform grid of triangle lists (triangle_grid): `lo` (3 floats), `cell`, `dims` (nx, ny, nz), `offsets`
    (cells + 1,) int64 and `entries` (E,) int32 on the device -- row c, the triangles whose bounding box meets cell c, is
    entries[offsets[c]:offsets[c + 1]], in no defined order -- and `vertices`, `triangles`, the mesh tensors it indexes."""

    def __init__(self, lo, cell, dims, offsets, entries, vertices, triangles):
        self.lo, self.cell, self.dims = lo, cell, dims
        self.offsets, self.entries, self.vertices, self.triangles = offsets, entries, vertices, triangles

    def row(self, x, y, z):
        """The triangles of cell (x, y, z), sorted: a host copy, for looking at a grid."""
        nx, ny, _ = self.dims
        c = (z * ny + y) * nx + x
        o = self.offsets[c:c + 2].tolist()
        return sorted(self.entries[o[0]:o[1]].tolist())


def _finite_box(p, rows):
    """(lo, hi) of the finite part of p ((N, 3), N > 0) as device tensors: +inf and -inf where nothing is finite.  `rows`:
    a row with any non-finite coordinate is left out whole; else every coordinate counts on its own."""
    fin = torch.isfinite(p)
    if rows:
        fin = fin.all(dim=1, keepdim=True)
    inf = torch.full((), float("inf"), dtype=p.dtype, device=p.device)
    return torch.where(fin, p, inf).amin(0), torch.where(fin, p, -inf).amax(0)


def _mesh_box(ver, tri):
    """(lo, hi, mean longest bounding-box side of the triangles) of a mesh over its finite coordinates: torch reductions and
    ONE host read.  An empty mesh, or one without a finite vertex, gives the box [0, 0]^3; no triangle, the extent 0."""
    V, T = ver.shape[0], tri.shape[0]
    if V == 0:
        return [0.0] * 3, [0.0] * 3, 0.0
    lo, hi = _finite_box(ver, rows=False)
    ext = torch.zeros((), dtype=torch.float64, device=ver.device)
    if T:
        corners = ver[tri.long().clamp(0, V - 1)]                       # (T, 3, 3); an index out of range is refused later
        side = (corners.amax(1) - corners.amin(1)).amax(1).double()
        ok = torch.isfinite(side)
        ext = torch.where(ok, side, torch.zeros_like(side)).sum() / ok.sum().clamp(min=1)
    host = torch.cat([lo.double(), hi.double(), ext.view(1)]).cpu().numpy()
    lo, hi = host[:3], host[3:6]
    if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
        lo, hi = np.zeros(3), np.zeros(3)
    return [float(v) for v in lo], [float(v) for v in hi], float(host[6])


def _dims(lo, hi, cell):
    return [max(1, int(math.floor((h - l) / cell)) + 1) for l, h in zip(lo, hi)]


def triangle_grid(mesh, cell=None, margin=0.0):
    """A TriangleGrid over `mesh`: cubic cells of size `cell` over the mesh's bounding box grown by `margin` each way; a
    triangle is listed in every cell its bounding box meets, so every point of it lies in a cell that lists it.

    cell=None means twice the mean longest bounding-box side of the triangles, raised until the grid has at most 2^24
    cells.  Two triangle extents is usual practice, and it is MEASURED (tests/time_meshdist.py): on
    660 k triangles and 10^6 queries, 1 x the extent answers queries that lie ON the surface in 1.2 ms against 1.7 ms, but
    queries four extents off it in 36 ms against 25 ms (4 x: 3.5 ms and 30 ms), and its offsets take 8 x the memory.

    ValueError: a cell that is not positive and finite, a negative or non-finite margin, more than 2^30 cells or more than
    65535 along an axis, more than INT32_MAX entries ("choose a larger cell"), a triangle with an index outside the vertices.
    TWO host synchronisations: the box and default cell (one read), and the totals of the counting call."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    margin = float(margin)
    if not (margin >= 0.0 and math.isfinite(margin)):
        raise ValueError("margin: a finite number, not negative")
    if cell is not None:
        cell = float(cell)
        if not (cell > 0.0 and math.isfinite(cell)) or not _f32(cell) > 0.0 or not math.isfinite(_f32(cell)):
            raise ValueError("cell: a positive finite number")
    lo, hi, extent = _mesh_box(ver, tri)
    lo, hi = [_f32(l - margin) for l in lo], [h + margin for h in hi]
    if cell is None:
        cell = 2.0 * extent if extent > 0.0 else max(max(h - l for l, h in zip(lo, hi)), 1.0)
        while max(_dims(lo, hi, _f32(cell))) > MAX_DIM or math.prod(_dims(lo, hi, _f32(cell))) > DEFAULT_MAX_CELLS:
            cell *= 1.25
    cell = _f32(cell)
    dims = _dims(lo, hi, cell)
    if max(dims) > MAX_DIM or math.prod(dims) > MAX_CELLS:
        raise ValueError(f"grid {dims[0]} x {dims[1]} x {dims[2]}: at most 2^30 cells and 65535 along an axis; choose a larger cell")
    cells = math.prod(dims)
    a = _lib.TriGridArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(tri), V, T
    a.lo[:], a.cell, a.dims[:] = lo, cell, dims
    with torch.cuda.device(dev):
        entries, outside = _count(a, "nfl_trigrid_count", _lib.lib().nfl_trigrid_bytes(*dims), 2, dev)
        _refuse_outside(outside, T, V)
        if entries > INT32_MAX:
            raise ValueError(f"grid: {entries} entries, more than int32 addresses; choose a larger cell")
        offsets = torch.empty(cells + 1, dtype=torch.int64, device=dev)
        rows = torch.empty(entries, dtype=torch.int32, device=dev)
        a.n_entries, a.d_offsets, a.d_entries = entries, _ptr(offsets), _ptr(rows)
        _launch("nfl_trigrid_emit", a)
    return TriangleGrid(lo, cell, dims, offsets, rows, ver, tri)


def _mesh_or_grid(mesh_or_grid, method):
    """(vertices, triangles, grid or None, whether its rows are walked) of what a query was handed: a TriangleGrid as it
    is, whatever the method (its box still holds for a cast that tries every triangle); a mesh dict with its grid built
    here when the method walks one."""
    if method not in ("grid", "brute"):
        raise ValueError(f"method: 'grid' or 'brute', got {method!r}")
    rows = method == "grid"
    if isinstance(mesh_or_grid, TriangleGrid):
        return mesh_or_grid.vertices, mesh_or_grid.triangles, mesh_or_grid, rows
    ver, _, _, tri = _mesh_tensors(mesh_or_grid)
    return ver, tri, triangle_grid(mesh_or_grid) if rows else None, rows


def closest_on_mesh(points, mesh_or_grid, max_distance=None, method="grid", normals=None):
    """The closest point of a mesh for every row of `points` ((N, 3) fp32 on the mesh's device): a dict with `distance`
    (N,) fp32, `triangle` (N,) int32, `point` (N, 3) and `bary` (N, 3), the barycentrics of the triangle's three corners.
    Among equally close triangles the lowest index answers.

    mesh_or_grid   a mesh dict, or a TriangleGrid (triangle_grid) to query one mesh many times;
    max_distance   positive, or None: a query with nothing within it gets distance +inf, triangle -1, NaN point and bary
                   (so do a query with a non-finite coordinate, and every query of an empty mesh);
    method         "grid" walks the shells of grid cells round the query until nothing outside them can be closer;
                   "brute" tries every triangle.  Both return the same bits;
    normals        (N, 3) fp32, a vector per query: the result gains `dot` (N,), its dot product with the unit face normal
                   of the answering triangle (NaN without an answer).

    No host synchronisation when handed a TriangleGrid (or with method="brute"); with a mesh dict, triangle_grid's."""
    ver, tri, grid, rows = _mesh_or_grid(mesh_or_grid, method)
    dev = ver.device
    _on_device(points)
    if not _is(points, torch.float32, 2, (3,), dev):
        raise ValueError("points: expected a contiguous fp32 (N, 3) tensor on the mesh's device")
    N = points.shape[0]
    if normals is not None:
        _on_device(normals)
        if not _is(normals, torch.float32, 2, (N, 3), dev):
            raise ValueError(f"normals: expected a contiguous fp32 ({N}, 3) tensor on the mesh's device")
    limit = _positive(max_distance, "max_distance: None or a positive number")
    new = lambda *shape, dtype=torch.float32: torch.empty(*shape, dtype=dtype, device=dev)
    out = {"distance": new(N), "triangle": new(N, dtype=torch.int32), "point": new(N, 3), "bary": new(N, 3)}
    if normals is not None:
        out["dot"] = new(N)
    a = _lib.MeshClosestArgs()
    a.d_points, a.n_points, a.d_vertices, a.d_triangles = _ptr(points.detach()), N, _ptr(ver), _ptr(tri)
    a.n_vertices, a.n_triangles, a.max_distance = ver.shape[0], tri.shape[0], limit
    if rows:
        a.d_offsets, a.d_entries, a.n_entries = _ptr(grid.offsets), _ptr(grid.entries), grid.entries.shape[0]
        a.lo[:], a.cell, a.dims[:] = grid.lo, grid.cell, grid.dims
    a.d_normals, a.d_dot = _ptr(normals), _ptr(out.get("dot"))
    a.d_distance, a.d_triangle, a.d_point, a.d_bary = (_ptr(out[k]) for k in ("distance", "triangle", "point", "bary"))
    with torch.cuda.device(dev):
        _launch("nfl_mesh_closest", a)
    return out


def _total_area(ver, tri):
    """The area of the usable triangles in fp64 (torch): ONE host read."""
    V = ver.shape[0]
    if V == 0 or tri.shape[0] == 0:
        return 0.0
    c = ver.double()[tri.long().clamp(0, V - 1)]
    area = 0.5 * torch.linalg.cross(c[:, 1] - c[:, 0], c[:, 2] - c[:, 0]).norm(dim=1)
    return float(torch.where(torch.isfinite(area), area, torch.zeros_like(area)).sum().item())


def sample_surface(mesh, density=None, n=None, seed=0):
    """Random points of the surface of `mesh`, uniform by area: exactly one of `density` (samples per unit area) and `n`
    (about that many samples: density = n / the total area, which is computed in fp64 with torch).  Triangle t gets
    floor(area_t * density + u_t) samples, u_t uniform in [0, 1) hashed from (seed, t): stochastic rounding, so the expected
    count is exact and small triangles are not starved.  The same seed gives the same samples, bit for bit.

    Returns a dict: `points` (N, 3) fp32, `triangles` (N,) int32 (the triangle of each sample; samples lie in triangle
    order) and `normals` (N, 3), the unit face normals.  Degenerate and non-finite triangles get no sample.
    ValueError: a density that is negative or not finite, a triangle that would get 2^24 samples or more, more than INT32_MAX
    samples, a triangle with an index outside the vertices.  ONE host synchronisation, the totals of the counting call,
    and with `n` a second one, the area."""
    if (density is None) == (n is None):
        raise ValueError("sample_surface: exactly one of `density` and `n`")
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    seed = _seed(seed, "seed: an integer in [0, 2^64)")
    if n is not None:
        if isinstance(n, bool) or int(n) != n or n < 0:
            raise ValueError("n: a non-negative integer")
        area = _total_area(ver, tri)
        density = n / area if area > 0.0 else 0.0
    density = float(density)
    if not (density >= 0.0 and math.isfinite(density) and math.isfinite(_f32(density))):
        raise ValueError("density: a finite number, not negative")
    a = _lib.MeshSampleArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(tri), V, T
    a.seed, a.density = seed, density
    with torch.cuda.device(dev):
        N, outside, dense = _count(a, "nfl_mesh_sample_count", _lib.lib().nfl_mesh_sample_bytes(T), 3, dev)
        _refuse_outside(outside, T, V)
        if dense:
            raise ValueError(f"sample_surface: {dense} triangles would get 2^24 samples or more; choose a smaller density")
        if N > INT32_MAX:
            raise ValueError(f"sample_surface: {N} samples, more than int32 addresses; choose a smaller density")
        out = {"points": torch.empty(N, 3, dtype=torch.float32, device=dev),
               "triangles": torch.empty(N, dtype=torch.int32, device=dev),
               "normals": torch.empty(N, 3, dtype=torch.float32, device=dev)}
        a.n_samples = N
        a.d_points, a.d_sample_triangles, a.d_normals = _ptr(out["points"]), _ptr(out["triangles"]), _ptr(out["normals"])
        _launch("nfl_mesh_sample_emit", a)
    return out


def _reduce(distance, dot, thresholds):
    """nfl_meshdist_reduce: the (13,) fp64 row of a run of distances, on the device.  No host synchronisation."""
    dev, N = distance.device, distance.shape[0]
    row = torch.empty(_lib.MESHDIST_COLUMNS, dtype=torch.float64, device=dev)
    scratch = _scratch(_lib.lib().nfl_meshdist_reduce_bytes(N), dev)
    a = _lib.MeshDistReduceArgs()
    a.d_distance, a.d_dot, a.n, a.n_tau = _ptr(distance), _ptr(dot), N, len(thresholds)
    a.tau[:len(thresholds)] = thresholds
    a.d_scratch, a.scratch_bytes, a.d_row = _ptr(scratch), scratch.numel() * 8, _ptr(row)
    with torch.cuda.device(dev):
        _launch("nfl_meshdist_reduce", a)
    return row


def _one_way(src, dst, n, thresholds, max_distance, seed, points):
    """The row of distances from `src` to `dst`, and the number of query points."""
    if points == "samples":
        s = sample_surface(src, n=n, seed=seed)
        p, nrm = s["points"], s["normals"]
    else:
        ver, nrm, _, _ = _mesh_tensors(src)
        p = ver
    got = closest_on_mesh(p, dst, max_distance=max_distance, normals=nrm)
    return _reduce(got["distance"], got["dot"], thresholds), p.shape[0]


def mesh_distance(a, b, n=100_000, thresholds=(), max_distance=None, seed=0, points="samples"):
    """How far apart the surfaces of two meshes are, both ways, as plain Python numbers.

    points="samples"   about `n` random points of each surface (sample_surface with `seed`) are the queries;
    points="vertices"  the vertices themselves are: the per-vertex displacement of a simplification or a smoothing;
    thresholds         up to 8 distances tau for precision, recall and F-score;
    max_distance       queries with nothing within it are `missing` and enter no mean.

    Returns a dict:
        a_to_b, b_to_a      {mean, rms, max, n, missing}: the distances from the points of one to the surface of the other;
        chamfer             the mean of the two means;        hausdorff   the larger of the two maxima;
        normal_consistency  the mean of the two means of |query normal . face normal of the closest triangle| (sample
                            normals are face normals, vertex queries use the mesh's vertex normals);
        precision, recall, fscore    a list per threshold: the share of a's points within tau of b, of b's within tau of a
                            (missing points count as not within), and their harmonic mean (0 when both are 0).
    A mean over no point is NaN.  mesh_distance(b, a) is mesh_distance(a, b) with the directions swapped, bit for bit.
    The two rows are reduced on the device in a fixed order and leave it in ONE copy at the end; before that come the
    synchronisations of triangle_grid and sample_surface, for each mesh."""
    if points not in ("samples", "vertices"):
        raise ValueError(f"points: 'samples' or 'vertices', got {points!r}")
    try:
        thresholds = [float(t) for t in thresholds]
    except (TypeError, ValueError):
        raise ValueError("thresholds: up to 8 numbers") from None
    if len(thresholds) > _lib.MESHDIST_MAX_TAU or any(t != t for t in thresholds):
        raise ValueError("thresholds: up to 8 numbers")
    row_ab, n_a = _one_way(a, b, n, thresholds, max_distance, seed, points)
    row_ba, n_b = _one_way(b, a, n, thresholds, max_distance, seed, points)
    rows = torch.stack([row_ab, row_ba]).cpu().numpy()

    def side(r, total):
        cnt = r[0]
        nan = float("nan")
        return {"mean": float(r[1] / cnt) if cnt else nan, "rms": float(math.sqrt(r[2] / cnt)) if cnt else nan,
                "max": float(r[3]), "n": int(total), "missing": int(total - cnt)}, (float(r[12] / cnt) if cnt else nan)

    ab, nc_ab = side(rows[0], n_a)
    ba, nc_ba = side(rows[1], n_b)
    prec = [float(rows[0][4 + k] / n_a) if n_a else float("nan") for k in range(len(thresholds))]
    rec = [float(rows[1][4 + k] / n_b) if n_b else float("nan") for k in range(len(thresholds))]
    fs = [2.0 * p * r / (p + r) if p + r > 0.0 else 0.0 for p, r in zip(prec, rec)]
    return {"a_to_b": ab, "b_to_a": ba, "chamfer": 0.5 * (ab["mean"] + ba["mean"]), "hausdorff": max(ab["max"], ba["max"]),
            "normal_consistency": 0.5 * (nc_ab + nc_ba), "thresholds": thresholds, "precision": prec, "recall": rec,
            "fscore": fs}
