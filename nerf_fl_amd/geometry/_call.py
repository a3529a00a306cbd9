"""What every stage of the geometry package calls, and the modules that stand beside it (meshdist, registration, raycast):
the argument checks, the launch line in its two forms (_launch for a struct, _call for plain arguments), the counting half
of a sized call, and the small parsers.  Nothing else in the package calls into the library or reads a device tensor back."""
import ctypes as C

import numpy as np
import torch

from .. import _lib, rendering


def _ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)


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


def _f32(x):
    """`x` rounded to fp32, as a Python float: what a kernel is handed."""
    return float(np.float32(x))


def _positive(x, message):
    """`x` as a float, None meaning +inf; ValueError(`message`) unless it is positive and still positive in fp32."""
    x = float("inf") if x is None else float(x)
    if not x > 0.0 or not _f32(x) > 0.0:
        raise ValueError(message)
    return x


def _seed(seed, message):
    """`seed` as an int; ValueError(`message`) unless it lies in [0, 2^64)."""
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError(message)
    return seed


def _three(v, message, number=float):
    """`v` as a list of 3 numbers; ValueError(`message`) when it is not three things `number` takes."""
    try:
        v = [number(x) for x in v]
    except (TypeError, ValueError):
        raise ValueError(message) from None
    if len(v) != 3:
        raise ValueError(message)
    return v


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


def _empty_mesh(V, T, colors, dev):
    """A mesh dict of V vertices and T triangles to be written by a kernel, with a colour row when `colors`."""
    rows = lambda: torch.empty(V, 3, dtype=torch.float32, device=dev)
    mesh = {"vertices": rows(), "normals": rows(), "triangles": torch.empty(T, 3, dtype=torch.int32, device=dev)}
    return dict(mesh, colors=rows()) if colors else mesh


def _launch(name, a, *before):
    """Entry point `name` of the library with its filled struct `a`, on the current device's stream; RuntimeError when it
    fails.  `before` is what nfl_render_pass takes ahead of its struct (the plan pointers); every other entry point takes
    the struct and the stream alone."""
    _lib.check(getattr(_lib.lib(), name)(*before, C.byref(a), rendering._stream()), name)


def _call(name, *args):
    """Entry point `name` of the library with its plain arguments, on the current device's stream; RuntimeError when it
    fails.  (_launch is for the entry points that take a struct.)"""
    _lib.check(getattr(_lib.lib(), name)(*args, rendering._stream()), name)


def _count(a, name, nbytes, n_totals, dev):
    """The counting half of a sized call: scratch of `nbytes` and `n_totals` int64 totals go into `a`, entry point `name`
    fills them, and the totals come back as Python ints -- THE host synchronisation of the call."""
    scratch = _scratch(nbytes, dev)
    totals = torch.empty(n_totals, dtype=torch.int64, device=dev)
    a.held = scratch, totals                                          # the emitting half still reads the scratch
    a.d_scratch, a.scratch_bytes, a.d_totals = _ptr(scratch), scratch.numel() * 8, _ptr(totals)
    _launch(name, a)
    return [int(v) for v in totals.tolist()]


def _refuse_outside(outside, T, V):
    """ValueError when `outside` of the T triangles of a mesh of V vertices name a vertex it does not have."""
    if outside:
        raise ValueError(f"mesh: {outside} of {T} triangles have an index outside [0, {V})")


def _camera_run(a, ver, tri, table, n_images, first, count):
    """The prefix the four raster structs share: the mesh, and images first .. first + count - 1 of `table`."""
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = _ptr(ver), _ptr(tri), ver.shape[0], tri.shape[0]
    a.d_table, a.n_images, a.first, a.count = _ptr(table), n_images, first, count
    return a


def _host(v):
    """A tensor or anything array-like as a numpy array on the host."""
    return v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)


def _host_mesh(mesh):
    """(vertices, normals, triangles) of a mesh dict (tensors or arrays) as host arrays for the file writers, checked:
    shapes, and every index inside the vertices."""
    ver, nrm, tri = _host(mesh["vertices"]), _host(mesh["normals"]), _host(mesh["triangles"])
    V, T = ver.shape[0], tri.shape[0]
    if ver.shape != (V, 3) or nrm.shape != (V, 3) or tri.shape != (T, 3):
        raise ValueError("mesh: vertices (V, 3), normals (V, 3), triangles (T, 3)")
    if T and (tri.min() < 0 or tri.max() >= V):
        raise ValueError("mesh: a triangle index lies outside the vertices")
    return ver, nrm, tri
