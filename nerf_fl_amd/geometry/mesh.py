"""A mesh worked on as a mesh: components and filtering, simplification, adjacency, normals, smoothing."""
import ctypes as C

import numpy as np
import torch

from .. import _lib
from ._call import (_count, _empty_mesh, _is, _launch, _mesh_tensors, _on_device, _ptr, _refuse_outside, _scratch,
                    _three)


def mesh_components(mesh):
    """The connected components of `mesh` (the dict extract_surface returns) as a dict: component (V,) int32, the id of
    every vertex; n_components C; and the table vertices (C,) int32, triangles (C,) int32 (a triangle counts for the
    component of its first index), bounds (C, 2, 3) fp32 (per-axis min and max of the vertex positions).  Two vertices
    are connected when a triangle names both; a vertex no triangle names is a component of its own; ids run in ascending
    order of a component's smallest vertex index.  Everything is integer work or min / max: two calls give the same bits.

    ONE host synchronisation: C and the number of out-of-range triangles are read from the device to size the table.
    ValueError when a triangle has an index outside [0, V)."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    component = torch.empty(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        n_comp, ignored = 0, T
        if V:
            a = _lib.MeshLabelArgs()
            a.d_triangles, a.n_vertices, a.n_triangles, a.d_component = _ptr(tri), V, T, _ptr(component)
            n_comp, ignored = _count(a, "nfl_mesh_label", _lib.lib().nfl_mesh_label_bytes(V, T), 2, dev)
        _refuse_outside(ignored, T, V)
        out = {"component": component, "n_components": n_comp,
               "vertices": torch.empty(n_comp, dtype=torch.int32, device=dev),
               "triangles": torch.empty(n_comp, dtype=torch.int32, device=dev),
               "bounds": torch.empty(n_comp, 2, 3, dtype=torch.float32, device=dev)}
        s = _lib.MeshStatsArgs()
        s.d_component, s.d_positions, s.d_triangles = _ptr(component), _ptr(ver), _ptr(tri)
        s.n_vertices, s.n_triangles, s.n_components = V, T, n_comp
        s.d_n_vertices, s.d_n_triangles, s.d_bounds = _ptr(out["vertices"]), _ptr(out["triangles"]), _ptr(out["bounds"])
        _launch("nfl_mesh_stats", s)
    return out


def filter_mesh(mesh, keep, components=None):
    """The part of `mesh` whose components `keep` ((C,) bool, on the device) names: a new dict with vertices, normals,
    triangles (and colors when `mesh` has them); kept rows stay in their order and the triangles index the kept vertices.
    `components` is what mesh_components(mesh) returned; without it that call is made here (its synchronisation too).

    ONE host synchronisation: the two kept totals are read from the device to size the outputs."""
    ver, nrm, col, tri = _mesh_tensors(mesh)
    if components is None:
        components = mesh_components(mesh)
    component, n_comp = components["component"], int(components["n_components"])
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    _on_device(keep)
    if not _is(keep, torch.bool, 1, (n_comp,), dev):
        raise ValueError(f"keep: expected a contiguous bool ({n_comp},) tensor on the mesh's device")
    if not _is(component, torch.int32, 1, (V,), dev):
        raise ValueError(f"components: component: expected a contiguous int32 ({V},) tensor on the mesh's device")
    if V + T == 0:
        return _empty_mesh(0, 0, col is not None, dev)
    a = _lib.MeshCompactArgs()
    a.d_component, a.d_keep, a.d_triangles = _ptr(component), _ptr(keep.view(torch.uint8)), _ptr(tri)
    a.n_vertices, a.n_triangles, a.n_components = V, T, n_comp
    with torch.cuda.device(dev):
        Vk, Tk = _count(a, "nfl_mesh_compact_count", _lib.lib().nfl_mesh_compact_bytes(V, T), 2, dev)
        out = _empty_mesh(Vk, Tk, col is not None, dev)
        a.n_kept_vertices, a.n_kept_triangles = Vk, Tk
        a.d_vertices, a.d_normals, a.d_colors = _ptr(ver), _ptr(nrm), _ptr(col)
        a.d_out_vertices, a.d_out_normals = _ptr(out["vertices"]), _ptr(out["normals"])
        a.d_out_colors, a.d_out_triangles = _ptr(out.get("colors")), _ptr(out["triangles"])
        _launch("nfl_mesh_compact_emit", a)
    return out


def clean_mesh(mesh, largest=None, min_triangles=None, box=None):
    """`mesh` without the components that fail a criterion; each criterion is judged on its own, over all components, and
    a component is kept when it passes every one that is given:
        min_triangles   its triangle count is at least this;
        box             (lo, hi), 3 numbers each: the bounds of its vertices lie inside, ends included; a component
                        with no finite coordinate on some axis has no bounds there (+inf / -inf) and fails;
        largest         it is among the `largest` components by triangle count; ties go to the lower id.
    The flags are built on the device from the table of mesh_components and handed to filter_mesh: two host
    synchronisations in all.  With no criterion the input is returned unchanged."""
    if largest is None and min_triangles is None and box is None:
        return mesh
    if largest is not None and int(largest) < 0:
        raise ValueError("largest must not be negative")
    comps = mesh_components(mesh)
    n_tri, dev = comps["triangles"], comps["component"].device
    keep = torch.ones(comps["n_components"], dtype=torch.bool, device=dev)
    if min_triangles is not None:
        keep &= n_tri >= int(min_triangles)
    if box is not None:
        message = "box: (lo, hi), 3 numbers each, in (x, y, z) order"
        try:
            lo, hi = box
        except (TypeError, ValueError):
            raise ValueError(message) from None
        lo, hi = (torch.tensor(_three(b, message), dtype=torch.float32, device=dev) for b in (lo, hi))
        bmin, bmax = comps["bounds"][:, 0], comps["bounds"][:, 1]
        keep &= ((bmin <= bmax) & (bmin >= lo) & (bmax <= hi)).all(dim=1)
    if largest is not None:
        order = torch.sort(n_tri.to(torch.int64), descending=True, stable=True).indices
        among = torch.zeros_like(keep)
        among[order[:int(largest)]] = True
        keep &= among
    return filter_mesh(mesh, keep, comps)


def _simplify_arguments(cell, origin, placement):
    """(cell, origin, placement code) of simplify_mesh, checked."""
    try:
        cell = float(cell)
    except (TypeError, ValueError):
        raise ValueError("cell: a finite positive number") from None
    if not (np.isfinite(cell) and cell > 0.0):
        raise ValueError(f"cell: a finite positive number, got {cell}")
    if placement not in _lib.SIMPLIFY_PLACEMENTS:
        raise ValueError(f"placement: one of {sorted(_lib.SIMPLIFY_PLACEMENTS)}, got {placement!r}")
    origin = _three(origin, "origin: 3 finite numbers, in (x, y, z) order")
    if not all(np.isfinite(origin)):
        raise ValueError("origin: 3 finite numbers, in (x, y, z) order")
    return cell, origin, _lib.SIMPLIFY_PLACEMENTS[placement]


def simplify_mesh(mesh, cell, origin=(0.0, 0.0, 0.0), placement="mean", return_map=False):
    """`mesh` simplified by uniform vertex clustering: the vertices that share a cube of side `cell` of the unbounded grid
    through `origin` become ONE vertex, triangles that lose a corner that way or repeat another one are dropped, and
    everything is re-indexed.  Returns a new dict with vertices, normals, triangles (and colors when `mesh` has them);
    with `return_map` also cluster (V,) int32, the new id of every input vertex (-1: a non-finite vertex, or one more
    than 2^20 cells from the origin).  The definition is written out in include/nerf_fl_amd.h, "mesh simplification":

        ids        clusters in ascending order of their smallest input vertex; surviving triangles in their input order,
                   the lowest index of each set of duplicates (equal up to rotation; a reversed triangle is another one);
        placement  "mean": the mean of the members, in int64 fixed point relative to the cell centre: bit-reproducible;
                   "quadric": the minimum of the members' triangle-plane quadric, regularised towards the mean and
                   clamped to the cell, which keeps corners and edges sharp where the mean rounds them off;
        normal     the normalised sum, colour the mean of the members'; a cluster of one keeps its member bit for bit.

    A cluster none of whose triangles survive stays as a vertex that no triangle names: clean_mesh(min_triangles=1)
    removes those.  ValueError when a triangle has an index outside [0, V).

    ONE host synchronisation: the four totals are read from the device to size the outputs and to raise."""
    cell, origin, code = _simplify_arguments(cell, origin, placement)
    ver, nrm, col, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        Vo, To, outside = 0, 0, T
        if V:
            a = _lib.MeshSimplifyArgs()
            a.d_vertices, a.d_normals, a.d_colors, a.d_triangles = _ptr(ver), _ptr(nrm), _ptr(col), _ptr(tri)
            a.n_vertices, a.n_triangles, a.cell, a.placement = V, T, cell, code
            a.origin[:] = origin
            a.d_cluster = _ptr(cluster)
            Vo, To, outside, _ = _count(a, "nfl_mesh_simplify_count", _lib.lib().nfl_mesh_simplify_bytes(V, T), 4, dev)
        _refuse_outside(outside, T, V)
        out = _empty_mesh(Vo, To, col is not None, dev)
        if V:
            a.n_out_vertices, a.n_out_triangles = Vo, To
            a.d_out_vertices, a.d_out_normals = _ptr(out["vertices"]), _ptr(out["normals"])
            a.d_out_colors, a.d_out_triangles = _ptr(out.get("colors")), _ptr(out["triangles"])
            _launch("nfl_mesh_simplify_emit", a)
    return (out, cluster) if return_map else out


def mesh_adjacency(mesh):
    """The vertex adjacency of `mesh` as two sorted CSR structures (include/nerf_fl_amd.h, "mesh smoothing"), a dict:

        tri_offsets (V + 1,) int64, incident (I,) int32    the entries 3 t + c of the triangle corners that name vertex v,
                                                           ascending, at incident[tri_offsets[v]:tri_offsets[v + 1]];
        offsets (V + 1,) int64, neighbors (N,) int32       the distinct vertices that share a triangle with v, ascending;
        boundary (V,) bool, n_boundary                     v lies on an edge that has a single triangle on it.

    Integer work, and every row is sorted: two calls give the same bits.  ValueError when a triangle has an index outside
    [0, V).

    ONE host synchronisation: the four totals are read from the device to size the outputs and to raise."""
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    with torch.cuda.device(dev):
        I, N, outside, n_boundary = 0, 0, T, 0
        if V:
            a = _lib.MeshAdjacencyArgs()
            a.d_triangles, a.n_vertices, a.n_triangles = _ptr(tri), V, T
            I, N, outside, n_boundary = _count(a, "nfl_mesh_adjacency_count", _lib.lib().nfl_mesh_adjacency_bytes(V, T), 4,
                                               dev)
        _refuse_outside(outside, T, V)
        new = lambda n, dtype: torch.empty(n, dtype=dtype, device=dev)
        out = {"offsets": new(V + 1, torch.int64), "neighbors": new(N, torch.int32), "boundary": new(V, torch.bool),
               "tri_offsets": new(V + 1, torch.int64), "incident": new(I, torch.int32), "n_boundary": n_boundary}
        if V:
            a.n_incident, a.n_neighbors = I, N
            a.d_tri_offsets, a.d_incident = _ptr(out["tri_offsets"]), _ptr(out["incident"])
            a.d_offsets, a.d_neighbors, a.d_boundary = _ptr(out["offsets"]), _ptr(out["neighbors"]), _ptr(out["boundary"])
            _launch("nfl_mesh_adjacency_emit", a)
        else:
            out["offsets"].zero_()
            out["tri_offsets"].zero_()
    return out


def _adjacency_of(adjacency, mesh, V, dev):
    """`adjacency` (what mesh_adjacency returned) checked against V vertices on `dev`; built from `mesh` when None."""
    if adjacency is None:
        return mesh_adjacency(mesh)
    try:
        rows = [adjacency[k] for k in ("offsets", "neighbors", "boundary", "tri_offsets", "incident")]
    except (TypeError, KeyError):
        raise ValueError("adjacency: the dict mesh_adjacency returns") from None
    _on_device(*rows)
    off, nbr, bnd, toff, inc = rows
    if not (_is(off, torch.int64, 1, (V + 1,), dev) and _is(toff, torch.int64, 1, (V + 1,), dev)
            and _is(bnd, torch.bool, 1, (V,), dev) and _is(nbr, torch.int32, 1, device=dev)
            and _is(inc, torch.int32, 1, device=dev)):
        raise ValueError(f"adjacency: not the adjacency of a mesh of {V} vertices on the mesh's device")
    return adjacency


def _smooth_arguments(iterations, lam, mu, boundary, normals):
    """(the factors of the steps, fix_boundary, weighting name or None) of smooth_mesh, checked."""
    if isinstance(iterations, bool) or not isinstance(iterations, (int, np.integer)) or not 0 <= iterations <= 512:
        raise ValueError(f"iterations: an int in [0, 512], got {iterations!r}")
    try:
        lam = float(lam)
    except (TypeError, ValueError):
        raise ValueError("lam: a finite number with 0 < lam <= 1") from None
    if not (np.isfinite(lam) and 0.0 < lam <= 1.0):
        raise ValueError(f"lam: a finite number with 0 < lam <= 1, got {lam}")
    if mu is not None:
        try:
            mu = float(mu)
        except (TypeError, ValueError):
            raise ValueError("mu: None, or a finite number < 0") from None
        if not (np.isfinite(mu) and mu < 0.0):
            raise ValueError(f"mu: None, or a finite number < 0, got {mu}")
    if boundary not in ("fixed", "free"):
        raise ValueError(f"boundary: 'fixed' or 'free', got {boundary!r}")
    if normals is not None and normals not in _lib.NORMAL_WEIGHTINGS:
        raise ValueError(f"normals: None or one of {sorted(_lib.NORMAL_WEIGHTINGS)}, got {normals!r}")
    factors = [lam] * int(iterations) if mu is None else [lam, mu] * int(iterations)
    return factors, boundary == "fixed", normals


def vertex_normals(mesh, weighting="area", adjacency=None, fallback=None):
    """(V, 3) fp32 vertex normals of `mesh` from its triangles (its own `normals` are not read): the normalised sum, over
    the triangle corners that name the vertex, of the triangle vector (p1 - p0) x (p2 - p0) (`weighting` "area": larger
    triangles count for more) or of that vector normalised ("uniform").  With the winding of extract_surface they point
    outwards.  A vertex whose sum is zero or not finite (no triangle, degenerate ones only) gets its row of `fallback`
    ((V, 3) fp32) bit for bit, or zeros.  The sums are fp64 in a fixed order: two calls give the same bits.
    `adjacency` is what mesh_adjacency(mesh) returned; without it that call is made here (its synchronisation too)."""
    if weighting not in _lib.NORMAL_WEIGHTINGS:
        raise ValueError(f"weighting: one of {sorted(_lib.NORMAL_WEIGHTINGS)}, got {weighting!r}")
    ver, _, _, tri = _mesh_tensors(mesh)
    dev, V, T = ver.device, ver.shape[0], tri.shape[0]
    if fallback is not None:
        _on_device(fallback)
        if not _is(fallback, torch.float32, 2, (V, 3), dev):
            raise ValueError(f"fallback: expected a contiguous fp32 ({V}, 3) tensor on the mesh's device")
    adj = _adjacency_of(adjacency, mesh, V, dev)
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    if V:
        a = _lib.MeshNormalsArgs()
        a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(tri), V, T
        a.d_tri_offsets, a.d_incident, a.n_incident = _ptr(adj["tri_offsets"]), _ptr(adj["incident"]), adj["incident"].shape[0]
        a.weighting, a.d_fallback_normals, a.d_out_normals = _lib.NORMAL_WEIGHTINGS[weighting], _ptr(fallback), _ptr(out)
        with torch.cuda.device(dev):
            _launch("nfl_mesh_normals", a)
    return out


def smooth_mesh(mesh, iterations=10, lam=0.5, mu=-0.53, boundary="fixed", pinned=None, adjacency=None, normals="area"):
    """`mesh` smoothed over its vertex adjacency (include/nerf_fl_amd.h, "mesh smoothing"): a new dict whose `vertices`
    are smoothed and whose `normals` are recomputed from the triangles (vertex_normals with weighting `normals`, the input
    normals as the fallback; `normals=None` passes the input normals through); `triangles` and `colors` are the input's.

    A step moves every vertex by a factor f towards the mean of its neighbours, all at once (Jacobi).  With `mu` an
    iteration is Taubin's pair of steps, f = lam then f = mu < 0, which smooths without the shrinkage of the plain
    Laplacian; `mu=None` is the plain Laplacian, one step of f = lam an iteration.  lam = 0.5, mu = -0.53 is the pair of
    Taubin's paper: a convention, not a measurement made here.

    boundary   "fixed": vertices on an edge with a single triangle stay where they are; "free": they move like the rest;
    pinned     (V,) bool or uint8: vertices that stay;
    adjacency  what mesh_adjacency(mesh) returned; without it that call is made here (its synchronisation too).

    A vertex with a non-finite coordinate stays and is left out of its neighbours' means.  The sums are fp64 in the order
    of the sorted rows: two calls give the same bits.  No host synchronisation of its own."""
    factors, fix, weighting = _smooth_arguments(iterations, lam, mu, boundary, normals)
    ver, nrm, col, tri = _mesh_tensors(mesh)
    dev, V = ver.device, ver.shape[0]
    if pinned is not None:
        _on_device(pinned)
        if not (_is(pinned, torch.bool, 1, (V,), dev) or _is(pinned, torch.uint8, 1, (V,), dev)):
            raise ValueError(f"pinned: expected a contiguous bool or uint8 ({V},) tensor on the mesh's device")
    adj = _adjacency_of(adjacency, mesh, V, dev)
    out = {"vertices": torch.empty_like(ver), "normals": nrm, "triangles": tri}
    if col is not None:
        out["colors"] = col
    if V:
        scratch = _scratch(_lib.lib().nfl_mesh_smooth_bytes(V), dev)
        host = (C.c_double * max(len(factors), 1))(*factors)
        a = _lib.MeshSmoothArgs()
        a.d_vertices, a.d_offsets, a.d_neighbors = _ptr(ver), _ptr(adj["offsets"]), _ptr(adj["neighbors"])
        a.n_vertices, a.n_neighbors = V, adj["neighbors"].shape[0]
        a.d_boundary, a.d_pinned, a.fix_boundary = _ptr(adj["boundary"]), _ptr(pinned), int(fix)
        a.n_steps, a.factors = len(factors), host
        a.d_scratch, a.scratch_bytes, a.d_out_vertices = _ptr(scratch), scratch.numel() * 8, _ptr(out["vertices"])
        with torch.cuda.device(dev):
            _launch("nfl_mesh_smooth", a)
    if weighting is not None:
        out["normals"] = vertex_normals(out, weighting=weighting, adjacency=adj, fallback=nrm)
    return out
