"""numpy restatement of the occupancy kernels (csrc/nfl_occupancy.hip; the definitions are in include/nerf_fl_amd.h,
"occupancy"): the build as boolean arrays and their packing into words, the ray clip in fp32 operation for operation
(vectorised over the rays, one walk step per loop turn), and a brute-force dilation written separately from the
separable one.  Conventions as in nerf_fl_amd.geometry: a lattice is (nz, ny, nx), cells are (cz, cy, cx), lo and
spacing are (x, y, z)."""
import numpy as np

F = np.float32


def inside(lat, threshold):
    with np.errstate(invalid="ignore"):
        return np.asarray(lat, dtype=F) >= F(threshold)             # NaN compares false


def build_dense(lat, threshold, dilate):
    """(cz, cy, cx) bool, the separable way: along every axis cell i is the OR of the POINTS max(i - d, 0) ..
    min(i + d + 1, n - 1) (its two corners and the dilation in one window)."""
    p = inside(lat, threshold)
    d = int(dilate)
    for axis in (2, 1, 0):
        n = p.shape[axis]
        p = np.stack([p.take(range(max(i - d, 0), min(i + d + 1, n - 1) + 1), axis=axis).any(axis=axis)
                      for i in range(n - 1)], axis=axis)
    return p


def build_dense_brute(lat, threshold, dilate):
    """The definition read literally: a cell is occupied at dilation 0 when one of its 8 corners is inside; at
    dilation d when some EXISTING cell within Chebyshev distance d is."""
    p = inside(lat, threshold)
    nz, ny, nx = p.shape
    occ0 = np.zeros((nz - 1, ny - 1, nx - 1), dtype=bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                occ0 |= p[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
    d = int(dilate)
    out = np.zeros_like(occ0)
    cz, cy, cx = occ0.shape
    for k in range(cz):
        for j in range(cy):
            for i in range(cx):
                out[k, j, i] = occ0[max(k - d, 0):k + d + 1, max(j - d, 0):j + d + 1, max(i - d, 0):i + d + 1].any()
    return out


def pack(dense):
    """(cz, cy, cx) bool -> (cz, cy, wx) uint32: cell i is bit i & 31 of word i >> 5; tail bits zero."""
    cz, cy, cx = dense.shape
    wx = (cx + 31) // 32
    padded = np.zeros((cz, cy, wx * 32), dtype=np.uint64)
    padded[..., :cx] = dense
    words = (padded.reshape(cz, cy, wx, 32) << np.arange(32, dtype=np.uint64)).sum(axis=-1)
    return words.astype(np.uint32)


def unpack(bits, cx):
    bits = np.asarray(bits).view(np.uint32) if np.asarray(bits).dtype == np.int32 else np.asarray(bits, dtype=np.uint32)
    cz, cy, wx = bits.shape
    return ((bits[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(cz, cy, wx * 32)[..., :cx]


def build_bits(lat, threshold, dilate):
    return pack(build_dense(lat, threshold, dilate))


def planes(lo, spacing, n):
    """fp32 positions of the n lattice planes of one axis: fl(lo + fl(b * spacing))."""
    return (F(lo) + np.arange(n, dtype=F) * F(spacing)).astype(F)


def clip(rays, dense, lo, spacing):
    """(near_far (R, 2) fp32, hit (R,) bool) of rays (R, 8) through the cells `dense` (cz, cy, cx) bool."""
    rays = np.ascontiguousarray(rays, dtype=F)
    lo, sp = np.asarray(lo, dtype=F), np.asarray(spacing, dtype=F)
    cz, cy, cx = dense.shape
    c = np.array([cx, cy, cz])
    R = rays.shape[0]
    o, d, near, far = rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7]
    with np.errstate(all="ignore"):
        miss = np.isnan(rays).any(axis=1)
        t0, t1 = near.copy(), far.copy()
        inv = np.zeros((R, 3), dtype=F)
        for k in range(3):
            hi = F(lo[k] + F(F(c[k]) * sp[k]))
            moving = d[:, k] != 0
            invk = (F(1) / d[:, k]).astype(F)
            ta, tb = (lo[k] - o[:, k]) * invk, (hi - o[:, k]) * invk
            t0 = np.where(moving, np.fmax(t0, np.fmin(ta, tb)), t0).astype(F)
            t1 = np.where(moving, np.fmin(t1, np.fmax(ta, tb)), t1).astype(F)
            miss |= ~moving & ~((o[:, k] >= lo[k]) & (o[:, k] <= hi))
            inv[:, k] = np.where(moving, invk, F(0))
        alive = ~miss & (t0 < t1)
        idx = np.zeros((R, 3), dtype=np.int64)
        for k in range(3):
            f = np.floor(((o[:, k] + t0 * d[:, k]) - lo[k]) / sp[k])
            f = np.fmin(np.fmax(f, F(0)), F(c[k] - 1))
            idx[:, k] = np.where(alive, f, 0).astype(np.int64)
        step = np.where(d > 0, 1, -1).astype(np.int64)
        b = idx + (d > 0)
        tn = np.where(d != 0, ((lo[None, :] + b.astype(F) * sp[None, :]) - o) * inv, F(np.inf)).astype(F)
        t_in = t0.copy()
        t_first, t_last = np.zeros(R, dtype=F), np.zeros(R, dtype=F)
        found = np.zeros(R, dtype=bool)
        for _ in range(cx + cy + cz + 1):
            if not alive.any():
                break
            occ = dense[idx[:, 2], idx[:, 1], idx[:, 0]] & alive
            axis = np.zeros(R, dtype=np.int64)
            t_out = tn[:, 0].copy()
            for k in (1, 2):                                        # ties stay with the lowest axis
                m = tn[:, k] < t_out
                axis[m], t_out[m] = k, tn[m, k]
            new = occ & ~found
            t_first[new] = t_in[new]
            found |= occ
            t_last[occ] = np.fmin(t_out, t1)[occ]
            alive &= t_out < t1
            r = np.nonzero(alive)[0]
            ax = axis[r]
            idx[r, ax] += step[r, ax]
            b[r, ax] += step[r, ax]
            gone = (idx[r, ax] < 0) | (idx[r, ax] >= c[ax])
            idx[r[gone], ax[gone]] -= step[r[gone], ax[gone]]       # stays addressable; the ray is finished
            alive[r[gone]] = False
            r, ax = r[~gone], ax[~gone]
            tn[r, ax] = ((lo[ax] + b[r, ax].astype(F) * sp[ax]) - o[r, ax]) * inv[r, ax]
            t_in[r] = t_out[r]
        hit = found & (t_last > t_first)
    out = np.stack([np.where(hit, t_first, near), np.where(hit, t_last, far)], axis=1).astype(F)
    return out, hit


def ball_lattice(cells, radius, half):
    """(cells + 1)^3 lattice of radius - |p| over [-half, half]^3: inside (>= 0) the ball.  Returns (lattice, lo, hi)."""
    n = cells + 1
    ax = planes(-half, (2.0 * half) / cells, n).astype(np.float64)
    zz, yy, xx = np.meshgrid(ax, ax, ax, indexing="ij")
    return (radius - np.sqrt(xx * xx + yy * yy + zz * zz)).astype(F), (-half,) * 3, (half,) * 3


def spacing_of(lo, hi, shape):
    """fp32 spacing of a (nz, ny, nx) lattice over [lo, hi], as geometry.lattice._box computes it (in double, rounded once)."""
    nz, ny, nx = shape
    return np.array([F((h - l) / (n - 1)) for l, h, n in zip(lo, hi, (nx, ny, nz))], dtype=F)


def pinhole_rays(H, W, cam_z, near, far):
    """(H W, 8) rays of the fov-60 test camera at (0, 0, cam_z) with identity rotation (it looks down -z): directions
    [(i - W / 2) / f, -(j - H / 2) / f, -1] normalised, as nfl_gen_rays forms them.  Computed in double and rounded:
    for estimates on the CPU (a hit share), not for bit comparisons with the device's generator."""
    f = W / 2 / np.tan(np.pi / 6)
    j, i = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    d = np.stack([(i - W / 2) / f, -(j - H / 2) / f, -np.ones_like(i)], axis=-1).reshape(-1, 3)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    rays = np.zeros((H * W, 8), dtype=F)
    rays[:, 2], rays[:, 3:6], rays[:, 6], rays[:, 7] = cam_z, d, near, far
    return rays


def random_rays(rng, R, lo, hi):
    """Origins inside and outside the box, aimed at points of the box, unnormalised; [near, far] partly outside it."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    size = hi - lo
    o = lo - size + rng.random((R, 3)) * 3 * size
    inside = rng.random(R) < 0.25
    o[inside] = (lo + rng.random((R, 3)) * size)[inside]
    target = lo + rng.random((R, 3)) * size
    d = (target - o) * rng.uniform(0.3, 2.0, (R, 1))
    axis = rng.random(R) < 0.1                                       # some axis-aligned ones
    keep = rng.integers(0, 3, R)
    for k in range(3):
        d[axis & (keep != k), k] = 0.0
    d[np.abs(d).sum(axis=1) == 0] = (1.0, 0.5, 0.25)
    rays = np.zeros((R, 8), dtype=F)
    rays[:, :3], rays[:, 3:6] = o, d
    rays[:, 6] = rng.uniform(0.0, 0.8, R)
    rays[:, 7] = rays[:, 6] + rng.uniform(0.2, 4.0, R)
    return rays
