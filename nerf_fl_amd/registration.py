"""Bring one mesh into the frame of another on the device: the similarity transform x' = s R x + t (rotation, translation
and, when asked for, scale) between a reconstruction and a ground-truth mesh, which mesh_distance assumes has been found.

    fit_transform        the closed form for given pairs of points (Horn's quaternion solution of Umeyama's problem)
    transform_points     nfl_register_apply on an (N, 3) tensor         transform_mesh   on a mesh's vertices and normals
    register_mesh        iterated closest point against a mesh: apply -> nfl_mesh_closest -> nfl_register_moments ->
                         nfl_register_solve per iteration, all on the stream, the transform itself in device memory
    registered_distance  register_mesh, then meshdist.mesh_distance of the moved mesh

The definitions are written out in include/nerf_fl_amd.h, "registration"; DESIGN.md section 34.  A TRANSFORM is a dict:
`scale` (float), `rotation` (3, 3), `translation` (3,), `matrix` (4, 4) as fp64 numpy arrays, and `device`, the 13 doubles
(s, R row-major, t) on the device, which is what the kernels read.  A dict without `device` (an inverse put together by
hand, say) is uploaded from `scale`, `rotation` and `translation`."""
import math

import numpy as np
import torch

from . import _lib
from .geometry._call import _call, _is, _mesh_tensors, _on_device, _positive, _ptr, _scratch
from .meshdist import _finite_box, _mesh_or_grid, closest_on_mesh, mesh_distance, sample_surface

__all__ = ["fit_transform", "transform_points", "transform_mesh", "register_mesh", "registered_distance"]

_STATUS = {v: k for k, v in _lib.REGISTER_STATUS.items()}


def _identity(dev):
    return torch.tensor([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=torch.float64, device=dev)


def _as_transform(device13, host13=None):
    """The dict of a transform from its 13 doubles on the device (`host13`: the same on the host, when already read)."""
    h = np.asarray(device13.cpu().numpy() if host13 is None else host13, dtype=np.float64)
    matrix = np.eye(4)
    matrix[:3, :3], matrix[:3, 3] = h[0] * h[1:10].reshape(3, 3), h[10:13]
    return {"scale": float(h[0]), "rotation": h[1:10].reshape(3, 3).copy(), "translation": h[10:13].copy(), "matrix": matrix,
            "device": device13}


def _device13(transform, dev):
    """The 13 doubles of `transform` on `dev`: its `device` entry when that is there, else uploaded from the host entries."""
    if transform is None:
        return _identity(dev)
    if not isinstance(transform, dict):
        raise ValueError("transform: a dict with scale, rotation (3, 3) and translation (3,)")
    d = transform.get("device")
    if d is not None:
        if not (torch.is_tensor(d) and _is(d, torch.float64, 1, (_lib.REGISTER_TRANSFORM,), dev)):
            raise ValueError("transform: `device` is 13 contiguous doubles on the points' device")
        return d
    try:
        s = float(transform["scale"])
        R = np.asarray(transform["rotation"], dtype=np.float64).reshape(3, 3)
        t = np.asarray(transform["translation"], dtype=np.float64).reshape(3)
    except (KeyError, TypeError, ValueError):
        raise ValueError("transform: a dict with scale, rotation (3, 3) and translation (3,)") from None
    host = np.concatenate([[s], R.reshape(9), t])
    if not np.isfinite(host).all():
        raise ValueError("transform: scale, rotation and translation are finite")
    return torch.from_numpy(host).to(dev)


def _points(points, what, dev=None):
    _on_device(points)
    if not _is(points, torch.float32, 2, (3,), dev):
        raise ValueError(f"{what}: expected a contiguous fp32 (N, 3) tensor" + (" on the same device" if dev is not None else ""))
    return points.detach()


def _apply(src, out, T13, vectors):
    _call("nfl_register_apply", _ptr(src), _ptr(out), src.shape[0], _ptr(T13), int(bool(vectors)))


def transform_points(points, transform, vectors=False):
    """`points` (N, 3) fp32 under `transform`: s R x + t, computed in fp64 and rounded once; with vectors=True R x alone
    (directions and normals).  A new tensor; no host synchronisation."""
    p = _points(points, "points")
    T13 = _device13(transform, p.device)
    out = torch.empty_like(p)
    with torch.cuda.device(p.device):
        _apply(p, out, T13, vectors)
    return out


def transform_mesh(mesh, transform):
    """A mesh dict under `transform`: vertices moved, normals rotated, triangles, colours and every other key carried over
    as they are (the same tensors).  No host synchronisation."""
    ver, nrm, _, _ = _mesh_tensors(mesh)
    return dict(mesh, vertices=transform_points(ver, transform), normals=transform_points(nrm, transform, vectors=True))


def _box_centre(p):
    """The middle of the box of the finite rows of p, as three Python floats: ONE host read."""
    if p.shape[0] == 0:
        return [0.0, 0.0, 0.0]
    box = torch.cat(_finite_box(p, rows=True)).double().cpu().numpy()
    if not np.isfinite(box).all():
        return [0.0, 0.0, 0.0]
    return [float(0.5 * (box[k] + box[3 + k])) for k in range(3)]


def _moments(p, q, triangle, distance, ver, tri, mode, max_distance, centre, scratch, row):
    V, T = (0, 0) if ver is None else (ver.shape[0], tri.shape[0])
    _call("nfl_register_moments", _ptr(p), _ptr(q), _ptr(triangle), _ptr(distance), _ptr(ver), _ptr(tri), p.shape[0], V, T,
          mode, max_distance, *centre, _ptr(scratch), scratch.numel() * 8, _ptr(row))


def _solve(row, mode, scale, min_pairs, centre, T13, history, iteration):
    _call("nfl_register_solve", _ptr(row), mode, int(bool(scale)), min_pairs, *centre, _ptr(T13), _ptr(history), iteration)


def _history(host):
    """The (iterations, 4) history as the dict register_mesh returns."""
    return {"count": [int(r[0]) for r in host], "rms": [float(r[1]) for r in host],
            "status": [_STATUS.get(int(r[2]), "unknown") for r in host], "scale": [float(r[3]) for r in host]}


def _refuse_failure(history, what):
    last = history["status"][-1]
    if last == "few":
        raise RuntimeError(f"{what}: the last step had {history['count'][-1]} pairs, fewer than min_pairs")
    if last != "ok":
        raise RuntimeError(f"{what}: the last step could not be solved (the pairs do not fix the transform: too few, "
                           "collinear, or a target that lets the source slide, such as a plane)")


def fit_transform(points, targets, scale=False):
    """The transform that brings `points` (N, 3) closest to `targets` (N, 3), row to row, in the least-squares sense: the
    closed form (Horn 1987; with scale=True Umeyama's problem, the scale fitted to the points' spread).  Rows with a
    non-finite coordinate do not take part.  The moments are summed on the device in fp64 about the middle of the points'
    box, in a fixed order: the same input gives the same bits.  RuntimeError when fewer than 3 pairs are left or they do not
    fix a rotation's scale.  TWO host reads: the box, and the transform."""
    p = _points(points, "points")
    q = _points(targets, "targets", p.device)
    if q.shape != p.shape:
        raise ValueError(f"targets: {tuple(q.shape)} for points {tuple(p.shape)}")
    dev, N = p.device, p.shape[0]
    mode = _lib.REGISTER_MODES["point"]
    with torch.cuda.device(dev):
        centre = _box_centre(p)
        T13 = _identity(dev)
        row = torch.empty(_lib.REGISTER_ROW["COLUMNS"], dtype=torch.float64, device=dev)
        history = torch.empty(_lib.REGISTER_HISTORY, dtype=torch.float64, device=dev)
        scratch = _scratch(_lib.lib().nfl_register_bytes(N), dev)
        _moments(p, q, None, None, None, None, mode, float("inf"), centre, scratch, row)
        _solve(row, mode, scale, 3, centre, T13, history, 0)
        host = torch.cat([T13, history]).cpu().numpy()
    h = _history(host[13:].reshape(1, 4))
    _refuse_failure(h, "fit_transform")
    return dict(_as_transform(T13, host[:13]), history=h)


def _schedule(max_distance, iterations):
    """One fp32-representable positive limit per iteration."""
    many = isinstance(max_distance, (list, tuple, np.ndarray)) or torch.is_tensor(max_distance)
    limits = [max_distance] * iterations if not many else list(max_distance)
    if len(limits) != iterations:
        raise ValueError(f"max_distance: a number, or one per iteration ({iterations}), got {len(limits)}")
    return [_positive(m, "max_distance: None, a positive number, or a positive number per iteration") for m in limits]


def register_mesh(source, target, initial=None, mode="plane", scale=False, iterations=30, n=50_000, points="samples",
                  max_distance=None, seed=0, min_pairs=6):
    """The transform that brings the surface of `source` onto `target`, by iterated closest point, from the start `initial`
    (a transform; None: the identity).  Returns the transform dict plus `history`: `count` (pairs that took part), `rms` (of
    their distances BEFORE that iteration's step), `status` ("ok", "few", "singular") and `scale`, a list entry per iteration.

    target        a mesh dict, or a meshdist.TriangleGrid over it (the grid is built once either way);
    points        "samples": about `n` random points of the source's surface (sample_surface with `seed`); "vertices": its vertices;
    mode          "plane" (the default) minimises the distances to the tangent planes of the closest points, linearised:
                  a smooth surface lets points slide along it, and point-to-plane does not resist that slide -- on the test
                  height field it reaches the fp32 floor in 5 or 6 iterations where "point" (Horn's closed form per
                  iteration) is still degrees off after 40.  The target must not be a plane or
                  another surface that leaves a motion free: that is refused ("singular"), not guessed;
    scale         fit the scale as well (a reconstruction from a structure-from-motion model has an arbitrary one);
    max_distance  pairs farther apart do not take part: a number, or one per iteration (a trimming schedule);
    min_pairs     a step with fewer pairs is refused ("few") and leaves the transform as it was.

    There is NO coarse alignment: ICP converges from a start within its basin (30 degrees on the test surface), and the
    caller passes `initial`; and no early stop on a tolerance, which would cost a host read per iteration.  The loop runs
    on the stream without one; before it come the synchronisations of triangle_grid and sample_surface and one read of the
    points' box (the moments are taken about its middle), after it ONE read: the transform and the history.
    RuntimeError when the last iteration failed."""
    if mode not in _lib.REGISTER_MODES:
        raise ValueError(f"mode: 'plane' or 'point', got {mode!r}")
    if points not in ("samples", "vertices"):
        raise ValueError(f"points: 'samples' or 'vertices', got {points!r}")
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= iterations <= 10_000:
        raise ValueError("iterations: an integer in [1, 10000]")
    if isinstance(min_pairs, bool) or int(min_pairs) != min_pairs or min_pairs < 1:
        raise ValueError("min_pairs: a positive integer")
    iterations, min_pairs = int(iterations), int(min_pairs)
    limits = _schedule(max_distance, iterations)
    grid = _mesh_or_grid(target, "grid")[2]
    dev = grid.vertices.device
    src = sample_surface(source, n=n, seed=seed)["points"] if points == "samples" else _mesh_tensors(source)[0]
    if src.device != dev:
        raise ValueError("source and target are on different devices")
    N, code = src.shape[0], _lib.REGISTER_MODES[mode]
    with torch.cuda.device(dev):
        T13 = _device13(initial, dev).clone()
        moved = torch.empty_like(src)
        _apply(src, moved, T13, False)
        centre = _box_centre(moved)
        row = torch.empty(_lib.REGISTER_ROW["COLUMNS"], dtype=torch.float64, device=dev)
        history = torch.empty(iterations * _lib.REGISTER_HISTORY, dtype=torch.float64, device=dev)
        scratch = _scratch(_lib.lib().nfl_register_bytes(N), dev)
        for it, limit in enumerate(limits):
            if it:
                _apply(src, moved, T13, False)
            got = closest_on_mesh(moved, grid, max_distance=None if math.isinf(limit) else limit)
            _moments(moved, got["point"], got["triangle"], got["distance"], grid.vertices, grid.triangles, code, limit, centre,
                     scratch, row)
            _solve(row, code, scale, min_pairs, centre, T13, history, it)
        host = torch.cat([T13, history]).cpu().numpy()
    h = _history(host[13:].reshape(iterations, 4))
    _refuse_failure(h, "register_mesh")
    return dict(_as_transform(T13, host[:13]), history=h)


def registered_distance(a, b, register=None, **distance):
    """mesh_distance between `a`, first brought onto `b` by register_mesh, and `b`: what the evaluation protocols that report
    Chamfer distance and F-score do before they measure.  `register` is a dict of register_mesh's arguments (initial, mode,
    scale, iterations, ...), the remaining keywords are mesh_distance's.  Returns mesh_distance's dict with `transform` (the
    transform dict) and `history` added."""
    T = register_mesh(a, b, **(register or {}))
    out = mesh_distance(transform_mesh(a, T), b, **distance)
    history = T.pop("history")
    return dict(out, transform=T, history=history)
