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
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib, rendering

__all__ = ["density_lattice", "extract_surface", "surface_colors", "write_ply", "extract_mesh", "lattice_points",
           "mesh_components", "filter_mesh", "clean_mesh", "simplify_mesh", "mesh_adjacency", "smooth_mesh",
           "vertex_normals", "OccupancyGrid", "occupancy_grid", "clip_rays",
           "mesh_depth", "color_mesh_from_images", "mesh_visibility", "render_mesh", "atlas_layout", "atlas_uv",
           "bake_texture", "write_obj"]

# Longest piece of an x-row handed to the render pass as one ray.  nfl_render_pass accepts any n_samples >= 1; the cut is
# a scheduling choice, not a limit of the ABI: the kernel gives whole rays to workgroups (contiguous ray ranges, one
# workgroup per CU), so a lattice of few, long rows would leave most CUs idle; 256 samples (8 segments of 32) keeps a ray
# near the lengths the renderer's own tests and benchmark exercise (64 + 64, 64 + 128).
_MAX_ROW_SAMPLES = 256


def _box(lo, hi, res):
    try:
        lo, hi = [float(v) for v in lo], [float(v) for v in hi]
        res = [int(v) for v in res]
    except TypeError:
        raise ValueError("lo, hi and res are 3 numbers each, in (x, y, z) order") from None
    if not len(lo) == len(hi) == len(res) == 3:
        raise ValueError("lo, hi and res are 3 numbers each, in (x, y, z) order")
    if min(res) < 2:
        raise ValueError(f"res {tuple(res)}: a lattice has at least 2 points along every axis")
    if not all(np.isfinite(lo + hi)) or not all(h > l for l, h in zip(lo, hi)):
        raise ValueError("lo and hi must be finite with hi > lo along every axis")
    return lo, [(h - l) / (n - 1) for l, h, n in zip(lo, hi, res)], res


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


def _row(v, n, what, dev):
    v = torch.as_tensor(v, dtype=torch.float32, device=dev).detach().reshape(1, -1)
    if v.shape[1] != n:
        raise ValueError(f"{what}: expected {n} numbers, got {v.shape[1]}")
    return v


def _scratch(nbytes, dev):
    return torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=dev)


def _on_device(*tensors):
    for t in tensors:
        if not torch.is_tensor(t) or t.device.type != "cuda":
            raise RuntimeError("nerf_fl_amd.geometry needs tensors on a ROCm device (this build has no CPU path)")


def _is(t, dtype, dim, tail=(), device=None, contiguous=True):
    """Whether `t` has this dtype and `dim` axes, the last ones `tail` long, is contiguous and (when given) on `device`."""
    return (t.dtype == dtype and t.dim() == dim and t.shape[dim - len(tail):] == tail
            and (t.is_contiguous() or not contiguous) and (device is None or t.device == device))


def _lattice(lattice, lo, hi):
    """(nx, ny, nz, lo, spacing) of a lattice tensor over the box [lo, hi], checked."""
    _on_device(lattice)
    if not _is(lattice, torch.float32, 3):
        raise ValueError("lattice: expected a contiguous fp32 (nz, ny, nx) tensor")
    nz, ny, nx = lattice.shape
    lo, sp, _ = _box(lo, hi, (nx, ny, nz))
    return nx, ny, nz, lo, sp


def _empty_mesh(V, T, colors, dev):
    """A mesh dict of V vertices and T triangles to be written by a kernel, with a colour row when `colors`."""
    rows = lambda: torch.empty(V, 3, dtype=torch.float32, device=dev)
    mesh = {"vertices": rows(), "normals": rows(), "triangles": torch.empty(T, 3, dtype=torch.int32, device=dev)}
    return dict(mesh, colors=rows()) if colors else mesh


def _axis(lo, spacing, n, device):
    """fp32 positions lo + i * spacing of one axis: the product and the sum rounded separately, as the kernels do."""
    return torch.arange(n, dtype=torch.float32, device=device) * np.float32(spacing) + np.float32(lo)


def lattice_points(lo, hi, res, device):
    """(nz, ny, nx, 3) fp32: the position of every lattice point, as density_lattice evaluates and extract_surface
    places it."""
    lo, sp, res = _box(lo, hi, res)
    x, y, z = (_axis(lo[k], sp[k], res[k], device) for k in range(3))
    zz, yy, xx = torch.meshgrid(z, y, x, indexing="ij")
    return torch.stack([xx, yy, zz], dim=-1)


def density_lattice(model, embeddings, lo, hi, res, chunk=1 << 20, a_embedded=None, view_dir=None):
    """Static sigma of `model` (a NeRF module; its transient head is never evaluated) at the points of the lattice
    `res` = (nx, ny, nz) over the box [lo, hi]: a (nz, ny, nx) fp32 tensor on the model's device.

    The x-rows of the lattice are handed to nfl_render_pass as rays (origin at the row's start, direction +x, explicit
    depths i * spacing), so the positions are encoded inside the fused kernel and no (points, 63) matrix exists in device
    memory; the pass writes its per-sample field outputs (d_field_raw, 36 B per point) and the density column is copied
    out of them.  The render kernel works on segments of 32 samples and masks the tail of a row itself; rows longer than
    256 points are cut into equal pieces (a multiple of 32 long), and the samples a last piece has past the row's end are
    evaluated and dropped.  One pass takes as many whole rows as fit into `chunk` evaluated points, and at least one row
    (a padded row longer than `chunk` still runs in one pass).

    Colour is not wanted by default (the pass runs sigma_only).  With `view_dir` (3 numbers; plus `a_embedded`, (n_a,),
    for a model that encodes appearance) the static colour head runs too and the result is (sigma, rgb (nz, ny, nx, 3)).
    Nothing here synchronises with the host."""
    lo, sp, res = _box(lo, hi, res)
    nx, ny, nz = res
    try:
        dev = next(model.parameters()).device
    except (AttributeError, StopIteration):
        raise ValueError("density_lattice: `model` must be a NeRF module with parameters") from None
    if dev.type != "cuda":
        raise RuntimeError("nerf_fl_amd.geometry needs the model on a ROCm device (this build has no CPU path)")
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be positive")
    color = view_dir is not None
    if a_embedded is not None and not color:
        raise ValueError("density_lattice: a_embedded only matters with view_dir (static sigma does not depend on it)")
    with torch.cuda.device(dev):
        field = rendering._field(model, rendering._n_freqs(embeddings["xyz"]), rendering._n_freqs(embeddings["dir"]), dev)
        if color:
            view_dir = _row(view_dir, 3, "view_dir", dev)
            if field.desc.encode_appearance:
                if a_embedded is None:
                    raise ValueError("density_lattice: this model encodes appearance; colour needs a_embedded")
                a_embedded = _row(a_embedded, int(field.desc.n_a), "a_embedded", dev)
            else:
                a_embedded = None
        # pieces of an x-row: n_piece equal pieces of S samples, S a multiple of the kernel's 32-sample segment
        cdiv = lambda p, q: -(-p // q)
        n_piece = cdiv(nx, _MAX_ROW_SAMPLES)
        S = cdiv(cdiv(nx, n_piece), 32) * 32 if n_piece > 1 else nx
        z_piece = _axis(0.0, sp[0], n_piece * S, dev).view(n_piece, S)       # depth of sample i of piece p: (p S + i) spacing
        ys, zs = _axis(lo[1], sp[1], ny, dev), _axis(lo[2], sp[2], nz, dev)
        n_rows = ny * nz
        rows_per_pass = max(1, min(n_rows, chunk // (n_piece * S)))
        sigma = torch.empty(nz, ny, nx, dtype=torch.float32, device=dev)
        rgb = torch.empty(nz, ny, nx, 3, dtype=torch.float32, device=dev) if color else None
        sig_rows, rgb_rows = sigma.view(n_rows, nx), (rgb.view(n_rows, nx, 3) if color else None)
        for r0 in range(0, n_rows, rows_per_pass):
            r1 = min(r0 + rows_per_pass, n_rows)
            n = r1 - r0
            row = torch.arange(r0, r1, device=dev)
            rays = torch.zeros(n, n_piece, 8, dtype=torch.float32, device=dev)
            rays[:, :, 0] = float(np.float32(lo[0]))
            rays[:, :, 1] = ys[row % ny, None]
            rays[:, :, 2] = zs[row // ny, None]
            rays[:, :, 3] = 1.0
            R = n * n_piece
            z = z_piece.expand(n, n_piece, S).contiguous()
            raw = torch.empty(R * S, 9, dtype=torch.float32, device=dev)
            # filled here rather than through rendering._run_pass: that one always allocates and writes weights (R, S) and
            # opacity, which a lattice has no use for; only d_field_raw and the status word are set
            a = _lib.PassArgs()
            a.d_rays, a.n_rays, a.n_samples, a.d_z = _ptr(rays), R, S, _ptr(z)
            a.sigma_only, a.d_field_raw, a.d_status = int(not color), _ptr(raw), _ptr(rendering._status_word(dev))
            keep = []
            if color:
                keep = [view_dir.expand(R, 3).contiguous(), None if a_embedded is None else a_embedded.expand(R, -1).contiguous()]
                a.d_view_dir, a.d_a_emb = _ptr(keep[0]), _ptr(keep[1])
            _lib.check(_lib.lib().nfl_render_pass(field.h_plan, _ptr(field.d_plan), _ptr(field.packed), C.byref(a),
                                                  rendering._stream()), "nfl_render_pass")
            raw = raw.view(n, n_piece * S, 9)
            sig_rows[r0:r1] = raw[:, :nx, 3]
            if color:
                rgb_rows[r0:r1] = raw[:, :nx, :3]
    return (sigma, rgb) if color else sigma


def extract_surface(lattice, iso, lo, hi):
    """The surface {value == iso} of `lattice` ((nz, ny, nx) fp32, contiguous, on the device) over the box [lo, hi] as a
    dict: vertices (V, 3) fp32 world coordinates, normals (V, 3) fp32 (unit, pointing from inside -- value >= iso -- to
    outside; zero where the gradient vanishes), triangles (T, 3) int32 indices into vertices, wound so that their normal
    points outwards too.  Vertices are shared between triangles; the order is fixed (vertices by lattice point and edge
    type, triangles by cell and tetrahedron) and two calls give the same bits.

    ONE host synchronisation: the two totals are read from the device to size the outputs."""
    nx, ny, nz, lo, sp = _lattice(lattice, lo, hi)
    dev = lattice.device
    lib = _lib.lib()
    nbytes = lib.nfl_surface_bytes(nx, ny, nz)
    if nbytes == 0:
        raise ValueError(f"lattice {nx} x {ny} x {nz}: at most 2^30 points, and 65535 rows and planes")
    scratch = _scratch(nbytes, dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    a = _lib.SurfaceArgs()
    a.d_lattice, a.nx, a.ny, a.nz, a.iso = _ptr(lattice), nx, ny, nz, float(iso)
    a.lo[:], a.spacing[:] = lo, sp
    a.d_scratch, a.scratch_bytes, a.d_totals = _ptr(scratch), scratch.numel() * 8, _ptr(totals)
    with torch.cuda.device(dev):
        stream = rendering._stream()
        _lib.check(lib.nfl_surface_count(C.byref(a), stream), "nfl_surface_count")
        V, T = (int(v) for v in totals.tolist())                       # the host synchronisation
        if V > 2 ** 31 - 1 or 3 * T > 2 ** 31 - 1:
            raise ValueError(f"the surface has {V} vertices and {T} triangles: more than int32 indices address")
        mesh = _empty_mesh(V, T, False, dev)
        a.n_vertices, a.n_triangles = V, T
        a.d_vertices, a.d_normals, a.d_triangles = _ptr(mesh["vertices"]), _ptr(mesh["normals"]), _ptr(mesh["triangles"])
        _lib.check(lib.nfl_surface_emit(C.byref(a), stream), "nfl_surface_emit")
    return mesh


def surface_colors(model, embeddings, vertices, normals, a_embedded=None):
    """Static rgb (V, 3) fp32 of `model` at `vertices`, each seen along -normal (the direction of a ray that meets the
    surface head-on), through nfl_posenc and the fused field kernel; `a_embedded` (n_a,) for a model that encodes
    appearance.  The transient head is not evaluated."""
    for t, what in ((vertices, "vertices"), (normals, "normals")):
        _on_device(t)
        if not _is(t, torch.float32, 2, (3,)):
            raise ValueError(f"{what}: expected a contiguous fp32 (V, 3) tensor")
    if vertices.shape != normals.shape or vertices.device != normals.device:
        raise ValueError("vertices and normals differ in shape or device")
    dev, V = vertices.device, vertices.shape[0]
    cols = [rendering.posenc(vertices, rendering._n_freqs(embeddings["xyz"])),
            rendering.posenc(-normals, rendering._n_freqs(embeddings["dir"]))]
    if model.encode_appearance:
        if a_embedded is None:
            raise ValueError("surface_colors: this model encodes appearance; give a_embedded")
        cols.append(_row(a_embedded, int(model.in_channels_a), "a_embedded", dev).expand(V, -1))
    return rendering.field_forward(model, torch.cat(cols, dim=1), output_transient=False)[:, :3].contiguous()


def write_ply(path, mesh, colors=None):
    """Write `mesh` (the dict extract_surface returns; tensors or arrays) as a binary little-endian PLY: per vertex x, y,
    z, nx, ny, nz as float32 and, with `colors` ((V, 3) in [0, 1]), red, green, blue as uint8 (rounded); per face a
    uint8 count of 3 and three int32 indices."""
    arr = lambda v: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
    ver, nrm, tri = arr(mesh["vertices"]), arr(mesh["normals"]), arr(mesh["triangles"])
    V, T = ver.shape[0], tri.shape[0]
    if ver.shape != (V, 3) or nrm.shape != (V, 3) or tri.shape != (T, 3):
        raise ValueError("mesh: vertices (V, 3), normals (V, 3), triangles (T, 3)")
    if T and (tri.min() < 0 or tri.max() >= V):
        raise ValueError("mesh: a triangle index lies outside the vertices")
    fields = [(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")]
    if colors is not None:
        col = arr(colors)
        if col.shape != (V, 3):
            raise ValueError(f"colors: expected ({V}, 3), got {col.shape}")
        fields += [(n, "u1") for n in ("red", "green", "blue")]
    vrec = np.empty(V, dtype=fields)
    for k, n in enumerate(("x", "y", "z")):
        vrec[n], vrec["n" + n] = ver[:, k], nrm[:, k]
    if colors is not None:
        c8 = np.rint(np.clip(np.nan_to_num(col.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        for k, n in enumerate(("red", "green", "blue")):
            vrec[n] = c8[:, k]
    frec = np.empty(T, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"], frec["v"] = 3, tri
    kinds = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", "comment nerf_fl_amd.geometry", f"element vertex {V}"]
    header += [f"property {kinds[t]} {n}" for n, t in fields]
    header += [f"element face {T}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def _mesh_tensors(mesh):
    """(vertices, normals, colors or None, triangles) of a mesh dict, checked: device, dtype, shape, contiguity."""
    try:
        ver, nrm, tri = mesh["vertices"], mesh["normals"], mesh["triangles"]
    except (TypeError, KeyError):
        raise ValueError("mesh: a dict with vertices (V, 3), normals (V, 3) and triangles (T, 3)") from None
    col = mesh.get("colors")
    _on_device(ver, nrm, tri, *(() if col is None else (col,)))
    for t, what in ((ver, "vertices"), (nrm, "normals"), (col, "colors")):
        if t is not None and not _is(t, torch.float32, 2, (3,)):
            raise ValueError(f"mesh: {what}: expected a contiguous fp32 (V, 3) tensor")
    if not _is(tri, torch.int32, 2, (3,)):
        raise ValueError("mesh: triangles: expected a contiguous int32 (T, 3) tensor")
    if nrm.shape != ver.shape or (col is not None and col.shape != ver.shape):
        raise ValueError("mesh: vertices, normals and colors differ in shape")
    if any(t.device != ver.device for t in (nrm, tri) + (() if col is None else (col,))):
        raise ValueError("mesh: tensors on different devices")
    if ver.shape[0] > 2 ** 31 - 1 or 3 * tri.shape[0] > 2 ** 31 - 1:
        raise ValueError(f"mesh: {ver.shape[0]} vertices and {tri.shape[0]} triangles: more than int32 indices address")
    return ver, nrm, col, tri


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
    lib = _lib.lib()
    component = torch.empty(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        stream = rendering._stream()
        if V:
            scratch = _scratch(lib.nfl_mesh_label_bytes(V, T), dev)
            totals = torch.empty(2, dtype=torch.int64, device=dev)
            a = _lib.MeshLabelArgs()
            a.d_triangles, a.n_vertices, a.n_triangles = _ptr(tri), V, T
            a.d_scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * 8
            a.d_component, a.d_totals = _ptr(component), _ptr(totals)
            _lib.check(lib.nfl_mesh_label(C.byref(a), stream), "nfl_mesh_label")
            n_comp, ignored = (int(v) for v in totals.tolist())            # the host synchronisation
        else:
            n_comp, ignored = 0, T
        if ignored:
            raise ValueError(f"mesh: {ignored} of {T} triangles have an index outside [0, {V})")
        out = {"component": component, "n_components": n_comp,
               "vertices": torch.empty(n_comp, dtype=torch.int32, device=dev),
               "triangles": torch.empty(n_comp, dtype=torch.int32, device=dev),
               "bounds": torch.empty(n_comp, 2, 3, dtype=torch.float32, device=dev)}
        s = _lib.MeshStatsArgs()
        s.d_component, s.d_positions, s.d_triangles = _ptr(component), _ptr(ver), _ptr(tri)
        s.n_vertices, s.n_triangles, s.n_components = V, T, n_comp
        s.d_n_vertices, s.d_n_triangles, s.d_bounds = _ptr(out["vertices"]), _ptr(out["triangles"]), _ptr(out["bounds"])
        _lib.check(lib.nfl_mesh_stats(C.byref(s), stream), "nfl_mesh_stats")
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
    lib = _lib.lib()
    keep8 = keep.view(torch.uint8)
    scratch = _scratch(lib.nfl_mesh_compact_bytes(V, T), dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    a = _lib.MeshCompactArgs()
    a.d_component, a.d_keep, a.d_triangles = _ptr(component), _ptr(keep8), _ptr(tri)
    a.n_vertices, a.n_triangles, a.n_components = V, T, n_comp
    a.d_scratch, a.scratch_bytes, a.d_totals = _ptr(scratch), scratch.numel() * 8, _ptr(totals)
    with torch.cuda.device(dev):
        stream = rendering._stream()
        if V + T:
            _lib.check(lib.nfl_mesh_compact_count(C.byref(a), stream), "nfl_mesh_compact_count")
            Vk, Tk = (int(v) for v in totals.tolist())                     # the host synchronisation
        else:
            Vk, Tk = 0, 0
        out = _empty_mesh(Vk, Tk, col is not None, dev)
        a.n_kept_vertices, a.n_kept_triangles = Vk, Tk
        a.d_vertices, a.d_normals, a.d_colors = _ptr(ver), _ptr(nrm), _ptr(col)
        a.d_out_vertices, a.d_out_normals = _ptr(out["vertices"]), _ptr(out["normals"])
        a.d_out_colors, a.d_out_triangles = _ptr(out.get("colors")), _ptr(out["triangles"])
        if V + T:
            _lib.check(lib.nfl_mesh_compact_emit(C.byref(a), stream), "nfl_mesh_compact_emit")
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
        try:
            lo, hi = ([float(v) for v in b] for b in box)
        except (TypeError, ValueError):
            raise ValueError("box: (lo, hi), 3 numbers each, in (x, y, z) order") from None
        if len(lo) != 3 or len(hi) != 3:
            raise ValueError("box: (lo, hi), 3 numbers each, in (x, y, z) order")
        lo, hi = (torch.tensor(b, dtype=torch.float32, device=dev) for b in (lo, hi))
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
    try:
        origin = [float(v) for v in origin]
    except (TypeError, ValueError):
        raise ValueError("origin: 3 finite numbers, in (x, y, z) order") from None
    if len(origin) != 3 or not all(np.isfinite(origin)):
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
    lib = _lib.lib()
    cluster = torch.empty(V, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        a = _lib.MeshSimplifyArgs()
        if V:
            stream = rendering._stream()
            scratch = _scratch(lib.nfl_mesh_simplify_bytes(V, T), dev)
            totals = torch.empty(4, dtype=torch.int64, device=dev)
            a.d_vertices, a.d_normals, a.d_colors, a.d_triangles = _ptr(ver), _ptr(nrm), _ptr(col), _ptr(tri)
            a.n_vertices, a.n_triangles, a.cell, a.placement = V, T, cell, code
            a.origin[:] = origin
            a.d_scratch, a.scratch_bytes = _ptr(scratch), scratch.numel() * 8
            a.d_totals, a.d_cluster = _ptr(totals), _ptr(cluster)
            _lib.check(lib.nfl_mesh_simplify_count(C.byref(a), stream), "nfl_mesh_simplify_count")
            Vo, To, outside, _ = (int(v) for v in totals.tolist())         # the host synchronisation
        else:
            Vo, To, outside = 0, 0, T
        if outside:
            raise ValueError(f"mesh: {outside} of {T} triangles have an index outside [0, {V})")
        out = _empty_mesh(Vo, To, col is not None, dev)
        if V:
            a.n_out_vertices, a.n_out_triangles = Vo, To
            a.d_out_vertices, a.d_out_normals = _ptr(out["vertices"]), _ptr(out["normals"])
            a.d_out_colors, a.d_out_triangles = _ptr(out.get("colors")), _ptr(out["triangles"])
            _lib.check(lib.nfl_mesh_simplify_emit(C.byref(a), stream), "nfl_mesh_simplify_emit")
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
    lib = _lib.lib()
    with torch.cuda.device(dev):
        a = _lib.MeshAdjacencyArgs()
        if V:
            stream = rendering._stream()
            scratch = _scratch(lib.nfl_mesh_adjacency_bytes(V, T), dev)
            totals = torch.empty(4, dtype=torch.int64, device=dev)
            a.d_triangles, a.n_vertices, a.n_triangles = _ptr(tri), V, T
            a.d_scratch, a.scratch_bytes, a.d_totals = _ptr(scratch), scratch.numel() * 8, _ptr(totals)
            _lib.check(lib.nfl_mesh_adjacency_count(C.byref(a), stream), "nfl_mesh_adjacency_count")
            I, N, outside, n_boundary = (int(v) for v in totals.tolist())  # the host synchronisation
        else:
            I, N, outside, n_boundary = 0, 0, T, 0
        if outside:
            raise ValueError(f"mesh: {outside} of {T} triangles have an index outside [0, {V})")
        new = lambda n, dtype: torch.empty(n, dtype=dtype, device=dev)
        out = {"offsets": new(V + 1, torch.int64), "neighbors": new(N, torch.int32), "boundary": new(V, torch.bool),
               "tri_offsets": new(V + 1, torch.int64), "incident": new(I, torch.int32), "n_boundary": n_boundary}
        if V:
            a.n_incident, a.n_neighbors = I, N
            a.d_tri_offsets, a.d_incident = _ptr(out["tri_offsets"]), _ptr(out["incident"])
            a.d_offsets, a.d_neighbors, a.d_boundary = _ptr(out["offsets"]), _ptr(out["neighbors"]), _ptr(out["boundary"])
            _lib.check(lib.nfl_mesh_adjacency_emit(C.byref(a), stream), "nfl_mesh_adjacency_emit")
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
            _lib.check(_lib.lib().nfl_mesh_normals(C.byref(a), rendering._stream()), "nfl_mesh_normals")
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
        lib = _lib.lib()
        scratch = _scratch(lib.nfl_mesh_smooth_bytes(V), dev)
        host = (C.c_double * max(len(factors), 1))(*factors)
        a = _lib.MeshSmoothArgs()
        a.d_vertices, a.d_offsets, a.d_neighbors = _ptr(ver), _ptr(adj["offsets"]), _ptr(adj["neighbors"])
        a.n_vertices, a.n_neighbors = V, adj["neighbors"].shape[0]
        a.d_boundary, a.d_pinned, a.fix_boundary = _ptr(adj["boundary"]), _ptr(pinned), int(fix)
        a.n_steps, a.factors = len(factors), host
        a.d_scratch, a.scratch_bytes, a.d_out_vertices = _ptr(scratch), scratch.numel() * 8, _ptr(out["vertices"])
        with torch.cuda.device(dev):
            _lib.check(lib.nfl_mesh_smooth(C.byref(a), rendering._stream()), "nfl_mesh_smooth")
    if weighting is not None:
        out["normals"] = vertex_normals(out, weighting=weighting, adjacency=adj, fallback=nrm)
    return out


def _run_raster(name, a, fields, lib, stream, ver, tri, table, n_images, first, count, words):
    """The raster `name` (its argument struct `a`) of images first .. first + count - 1 of `table` into `words`, one per
    pixel of the run; `fields` names the struct's pointer to them and their number."""
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(tri), ver.shape[0], tri.shape[0]
    a.d_table, a.n_images, a.first, a.count = _ptr(table), n_images, first, count
    setattr(a, fields[0], _ptr(words))
    setattr(a, fields[1], words.numel())
    _lib.check(getattr(lib, name)(C.byref(a), stream), name)


def _run_depth(lib, stream, ver, tri, table, n_images, first, count, depth):
    """nfl_mesh_depth of images first .. first + count - 1 of `table` into `depth` (the run's pixels, fp32)."""
    _run_raster("nfl_mesh_depth", _lib.MeshDepthArgs(), ("d_depth", "n_depth"), lib, stream, ver, tri, table, n_images,
                first, count, depth)


def _run_visibility(lib, stream, ver, tri, table, n_images, first, count, vis):
    """nfl_mesh_visibility of images first .. first + count - 1 of `table` into `vis` (the run's pixels, int64 words)."""
    _run_raster("nfl_mesh_visibility", _lib.MeshVisibilityArgs(), ("d_vis", "n_vis"), lib, stream, ver, tri, table, n_images,
                first, count, vis)


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
    lib = _lib.lib()
    table, n_images, image, H, W = _camera_record(what, dev, c2w, K, H, W, bank, image)
    words = torch.empty(H, W, dtype=dtype, device=dev)
    with torch.cuda.device(dev):
        run(lib, rendering._stream(), ver, tri, table, n_images, image, 1, words)
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
    try:
        background = [float(v) for v in background]
    except TypeError:
        raise ValueError("background: 3 numbers") from None
    if len(background) != 3:
        raise ValueError("background: 3 numbers")
    lib = _lib.lib()
    table, n_images, image, H, W = _camera_record("render_mesh", dev, c2w, K, H, W, bank, image)
    vis = torch.empty(H * W, dtype=torch.int64, device=dev)
    out = {"rgb": torch.empty(H, W, 3, dtype=torch.uint8, device=dev),
           "rgb_float": torch.empty(H * W, 3, dtype=torch.float32, device=dev),
           "depth": torch.empty(H, W, dtype=torch.float32, device=dev),
           "triangle": torch.empty(H, W, dtype=torch.int32, device=dev)}
    with torch.cuda.device(dev):
        stream = rendering._stream()
        _run_visibility(lib, stream, ver, tri, table, n_images, image, 1, vis)
        a = _lib.MeshShadeArgs() if atlas is None else _lib.MeshShadeAtlasArgs()
        a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(tri), V, tri.shape[0]
        a.d_table, a.n_images, a.first, a.count = _ptr(table), n_images, image, 1
        a.d_vis, a.n_vis = _ptr(vis), H * W
        a.background[:] = background
        a.d_rgb, a.d_rgb_u8, a.d_depth, a.d_triangle = (_ptr(out[k]) for k in ("rgb_float", "rgb", "depth", "triangle"))
        if atlas is None:
            a.mode, a.d_attr = _lib.SHADE_MODES[shade], _ptr(attr)
            _lib.check(lib.nfl_mesh_shade(C.byref(a), stream), "nfl_mesh_shade")
        else:
            a.d_atlas, a.d_atlas_u8, a.cell, a.cols, a.rows = _ptr(atlas[0]), _ptr(atlas[1]), *atlas[2:]
            _lib.check(lib.nfl_mesh_shade_atlas(C.byref(a), stream), "nfl_mesh_shade_atlas")
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
        self.lib, self.ver, self.tri, self.bank, self.runs = _lib.lib(), ver, tri, bank, runs
        self.weights, self.weighting, self.min_cos, self.depth_tol, self.reject = weights, weighting, min_cos, depth_tol, reject
        dev = ver.device
        self.keep = keep and sum(r[2] for r in runs) <= batch_pixels
        self.scratch = None if self.keep or not runs else torch.empty(max(r[2] for r in runs), dtype=torch.float32, device=dev)
        self.kept = {}

    def blend(self, points, normals, center, sums, views):
        """One pass over all runs: `sums` (n, 4) and `views` (n,) begin at zero; with `center` (n, 3) the samples further
        than `reject` from it are left out.  On the current device's stream."""
        lib, bank, dev, stream = self.lib, self.bank, self.ver.device, rendering._stream()
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
                _run_depth(lib, stream, self.ver, self.tri, bank.table, bank.n_images, first, count, depth)
                if self.keep:
                    self.kept[first] = depth
            else:
                depth = None
            a.first, a.count, a.start = first, count, int(k == 0)
            a.d_depth, a.n_depth = _ptr(depth), pixels
            _lib.check(lib.nfl_mesh_blend(C.byref(a), stream), "nfl_mesh_blend")


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
        try:
            flat = [float(v) for v in fallback]
        except TypeError:
            raise ValueError("fallback: 'colors' or 3 numbers") from None
        if len(flat) != 3:
            raise ValueError("fallback: 'colors' or 3 numbers")
    try:
        background = [float(v) for v in background]
    except TypeError:
        raise ValueError("background: 3 numbers") from None
    if len(background) != 3:
        raise ValueError("background: 3 numbers")
    N = W * H
    lib = _lib.lib()
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
        _lib.check(lib.nfl_atlas_resolve(C.byref(r), stream), "nfl_atlas_resolve")

    with torch.cuda.device(dev):
        stream = rendering._stream()
        for first in range(0, N, texel_batch):
            n = min(texel_batch, N - first)
            a = _lib.AtlasPointsArgs()
            a.d_vertices, a.d_vertex_normals, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(nrm), _ptr(tri), V, T
            a.cell, a.cols, a.rows, a.first_texel, a.n_texels = cell, cols, rows, first, n
            a.d_points, a.d_normals = _ptr(pts), _ptr(nor)
            _lib.check(lib.nfl_atlas_points(C.byref(a), stream), "nfl_atlas_points")
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


def write_obj(path, mesh, atlas):
    """Write `mesh` with its texture `atlas` (the dict bake_texture returns; tensors or arrays) as `stem`.obj,
    `stem`.mtl and `stem`.png beside each other, `path` being any of the three or the bare stem: per vertex `v` and
    `vn`, per CORNER a `vt` ((x + 0.5) / W, 1 - (y + 0.5) / H of atlas_uv: the PNG's row 0 is the top), faces
    `f v/vt/vn` 1-based, the material's `map_Kd` the PNG of `texture_u8`.  Needs Pillow."""
    import os
    from PIL import Image
    arr = lambda v: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
    ver, nrm, tri = arr(mesh["vertices"]), arr(mesh["normals"]), arr(mesh["triangles"])
    V, T = ver.shape[0], tri.shape[0]
    if ver.shape != (V, 3) or nrm.shape != (V, 3) or tri.shape != (T, 3):
        raise ValueError("mesh: vertices (V, 3), normals (V, 3), triangles (T, 3)")
    if T and (tri.min() < 0 or tri.max() >= V):
        raise ValueError("mesh: a triangle index lies outside the vertices")
    try:
        tex8, cell, cols = atlas.get("texture_u8"), int(atlas["cell"]), int(atlas["cols"])
    except (TypeError, KeyError, AttributeError):
        raise ValueError("atlas: a dict with `texture_u8` (H, W, 3) uint8, `cell` and `cols`") from None
    if tex8 is None:
        raise ValueError("atlas: a dict with `texture_u8` (H, W, 3) uint8, `cell` and `cols`")
    tex8 = arr(tex8)
    lay = atlas_layout(T, cell, cols)
    if tex8.dtype != np.uint8 or tex8.ndim != 3 or tex8.shape[2] != 3 or tex8.shape[1] != lay["width"] \
            or tex8.shape[0] % cell or tex8.shape[0] < lay["height"]:
        raise ValueError(f"atlas: texture_u8 {tex8.shape} is not an atlas of cell {cell} and {cols} columns for {T} triangles")
    H, W = tex8.shape[:2]
    stem = str(path)
    if stem.lower().endswith((".obj", ".mtl", ".png")):
        stem = stem[:-4]
    name = os.path.basename(stem)
    Image.fromarray(np.ascontiguousarray(tex8), "RGB").save(stem + ".png")
    with open(stem + ".mtl", "w") as f:
        f.write(f"# nerf_fl_amd.geometry\nnewmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {name}.png\n")
    uv = atlas_uv(lay, T).reshape(-1, 2)
    vt = np.stack([(uv[:, 0] + 0.5) / W, 1.0 - (uv[:, 1] + 0.5) / H], axis=1)
    lines = [f"# nerf_fl_amd.geometry\nmtllib {name}.mtl\nusemtl {name}\n"]
    lines += ["".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in ver.astype(np.float64).tolist())]
    lines += ["".join(f"vn {x!r} {y!r} {z!r}\n" for x, y, z in nrm.astype(np.float64).tolist())]
    lines += ["".join(f"vt {u!r} {v!r}\n" for u, v in vt.tolist())]
    lines += ["".join(f"f {a + 1}/{3 * t + 1}/{a + 1} {b + 1}/{3 * t + 2}/{b + 1} {c + 1}/{3 * t + 3}/{c + 1}\n"
                      for t, (a, b, c) in enumerate(tri.tolist()))]
    with open(stem + ".obj", "w") as f:
        f.write("".join(lines))


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


class OccupancyGrid:
    """One bit per cell of a lattice (the definition is written out in include/nerf_fl_amd.h, "occupancy").

        bits        (cz, cy, wx) int32 on the device: cell (i, j, k) is bit i & 31 of bits[k, j, i >> 5]
        lo, spacing 3 floats each, (x, y, z): lattice plane b of an axis lies at lo + b * spacing (fp32)
        cells       (cx, cy, cz)
        threshold, dilate   what the grid was built with"""

    def __init__(self, bits, lo, spacing, cells, threshold, dilate):
        self.bits, self.lo, self.spacing, self.cells = bits, tuple(lo), tuple(spacing), tuple(cells)
        self.threshold, self.dilate = float(threshold), int(dilate)

    def to_dense(self):
        """(cz, cy, cx) bool tensor on the device: the cells, unpacked with torch bit operations."""
        cx, cy, cz = self.cells
        shifts = torch.arange(32, dtype=torch.int32, device=self.bits.device)
        return ((self.bits[..., None] >> shifts) & 1).bool().reshape(cz, cy, -1)[..., :cx]

    def fraction(self):
        """Share of occupied cells.  ONE host read."""
        cx, cy, cz = self.cells
        return float(self.to_dense().sum().item()) / (cx * cy * cz)


def occupancy_grid(lattice, threshold, lo, hi, dilate=1):
    """The OccupancyGrid of `lattice` ((nz, ny, nx) fp32, contiguous, on the device; density_lattice returns one) over
    the box [lo, hi]: a cell is occupied when one of its 8 corner values is >= `threshold` (NaN never is), or when a
    cell within `dilate` (0 .. 8) cells of it, in the Chebyshev sense, is.  Built on the device in four launches, without
    atomics: two calls give the same bits.  Nothing here synchronises with the host.

    The default of ONE cell of dilation is the usual practice and not a measured choice: the density between lattice
    points is not bounded by the corner values, so a thin structure that passes between the points of a cell is missed
    at any threshold, and the dilation only makes that less likely.  Choose the lattice fine enough for the scene."""
    nx, ny, nz, lo, sp = _lattice(lattice, lo, hi)
    dilate = int(dilate)
    if not 0 <= dilate <= 8:
        raise ValueError("dilate: 0 .. 8 cells")
    dev = lattice.device
    lib = _lib.lib()
    nbytes, sbytes = lib.nfl_occ_bytes(nx, ny, nz), lib.nfl_occ_build_bytes(nx, ny, nz, dilate)
    if nbytes == 0 or sbytes == 0:
        raise ValueError(f"lattice {nx} x {ny} x {nz}: at most 2^30 points, and 65535 rows and planes")
    bits = torch.empty(nz - 1, ny - 1, (nx - 1 + 31) // 32, dtype=torch.int32, device=dev)
    scratch = _scratch(sbytes, dev)
    a = _lib.OccBuildArgs()
    a.d_lattice, a.nx, a.ny, a.nz, a.threshold, a.dilate = _ptr(lattice), nx, ny, nz, float(threshold), dilate
    a.d_scratch, a.scratch_bytes, a.d_bits = _ptr(scratch), scratch.numel() * 8, _ptr(bits)
    with torch.cuda.device(dev):
        _lib.check(lib.nfl_occ_build(C.byref(a), rendering._stream()), "nfl_occ_build")
    f32 = lambda v: float(np.float32(v))
    return OccupancyGrid(bits, [f32(v) for v in lo], [f32(v) for v in sp], (nx - 1, ny - 1, nz - 1), threshold, dilate)


def clip_rays(grid, rays):
    """Walk `rays` ((R, 8) fp32 rows [o, d, near, far] on the grid's device) through the OccupancyGrid `grid`.  Returns
    (rays', hit): rays' is a copy whose columns 6 and 7 hold, for a ray that meets an occupied cell inside [near, far],
    the depth at which it enters the first one and the depth at which it leaves the last one, and the ray's own near and
    far otherwise; hit (R,) bool tells the two apart.  The direction need not be normalised: the depths are in the
    ray's own parameter, as the renderer samples them.

    Space outside the grid's box is EMPTY: a ray that does not cross the box hits nothing, whatever the field holds
    there.  A ray with a NaN in it hits nothing.  No host synchronisation."""
    if not isinstance(grid, OccupancyGrid):
        raise ValueError("clip_rays: `grid` is what occupancy_grid returns")
    _on_device(rays)
    if not _is(rays, torch.float32, 2, (8,), contiguous=False):
        raise ValueError("rays: expected an fp32 (R, 8) tensor")
    dev = grid.bits.device
    if rays.device != dev:
        raise ValueError("rays and grid on different devices")
    out = rays.clone(memory_format=torch.contiguous_format)
    R = rays.shape[0]
    near_far = torch.empty(R, 2, dtype=torch.float32, device=dev)
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    cx, cy, cz = grid.cells
    a = _lib.OccClipArgs()
    a.d_rays, a.n_rays, a.d_bits, a.nx, a.ny, a.nz = _ptr(out), R, _ptr(grid.bits), cx + 1, cy + 1, cz + 1
    a.lo[:], a.spacing[:] = grid.lo, grid.spacing
    a.d_near_far, a.d_hit = _ptr(near_far), _ptr(hit)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().nfl_occ_clip_rays(C.byref(a), rendering._stream()), "nfl_occ_clip_rays")
    out[:, 6:8] = near_far
    return out, hit.view(torch.bool)
