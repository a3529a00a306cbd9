"""The field on a lattice and its iso-surface: lattice_points, density_lattice, extract_surface, surface_colors."""
import numpy as np
import torch

from .. import _lib, rendering
from ._call import _count, _empty_mesh, _is, _launch, _on_device, _ptr, _three

# Longest piece of an x-row handed to the render pass as one ray.  nfl_render_pass accepts any n_samples >= 1; the cut is
# a scheduling choice, not a limit of the ABI: the kernel gives whole rays to workgroups (contiguous ray ranges, one
# workgroup per CU), so a lattice of few, long rows would leave most CUs idle; 256 samples (8 segments of 32) keeps a ray
# near the lengths the renderer's own tests and benchmark exercise (64 + 64, 64 + 128).
_MAX_ROW_SAMPLES = 256


def _box(lo, hi, res):
    message = "lo, hi and res are 3 numbers each, in (x, y, z) order"
    lo, hi, res = _three(lo, message), _three(hi, message), _three(res, message, int)
    if min(res) < 2:
        raise ValueError(f"res {tuple(res)}: a lattice has at least 2 points along every axis")
    if not all(np.isfinite(lo + hi)) or not all(h > l for l, h in zip(lo, hi)):
        raise ValueError("lo and hi must be finite with hi > lo along every axis")
    return lo, [(h - l) / (n - 1) for l, h, n in zip(lo, hi, res)], res


def _row(v, n, what, dev):
    v = torch.as_tensor(v, dtype=torch.float32, device=dev).detach().reshape(1, -1)
    if v.shape[1] != n:
        raise ValueError(f"{what}: expected {n} numbers, got {v.shape[1]}")
    return v


def _lattice(lattice, lo, hi):
    """(nx, ny, nz, lo, spacing) of a lattice tensor over the box [lo, hi], checked."""
    _on_device(lattice)
    if not _is(lattice, torch.float32, 3):
        raise ValueError("lattice: expected a contiguous fp32 (nz, ny, nx) tensor")
    nz, ny, nx = lattice.shape
    lo, sp, _ = _box(lo, hi, (nx, ny, nz))
    return nx, ny, nz, lo, sp


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
            _launch("nfl_render_pass", a, field.h_plan, _ptr(field.d_plan), _ptr(field.packed))
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
    nbytes = _lib.lib().nfl_surface_bytes(nx, ny, nz)
    if nbytes == 0:
        raise ValueError(f"lattice {nx} x {ny} x {nz}: at most 2^30 points, and 65535 rows and planes")
    a = _lib.SurfaceArgs()
    a.d_lattice, a.nx, a.ny, a.nz, a.iso = _ptr(lattice), nx, ny, nz, float(iso)
    a.lo[:], a.spacing[:] = lo, sp
    with torch.cuda.device(dev):
        V, T = _count(a, "nfl_surface_count", nbytes, 2, dev)
        if V > 2 ** 31 - 1 or 3 * T > 2 ** 31 - 1:
            raise ValueError(f"the surface has {V} vertices and {T} triangles: more than int32 indices address")
        mesh = _empty_mesh(V, T, False, dev)
        a.n_vertices, a.n_triangles = V, T
        a.d_vertices, a.d_normals, a.d_triangles = _ptr(mesh["vertices"]), _ptr(mesh["normals"]), _ptr(mesh["triangles"])
        _launch("nfl_surface_emit", a)
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
