"""CPU-side checks of the occupancy feature (nerf_fl_amd.geometry.occupancy_grid / clip_rays, csrc/nfl_occupancy.hip):
the C entry points size their buffers and refuse bad arguments before any launch (their structs and signatures are held to
the header in tests/test_abi_cpu.py); the numpy restatement
(tests/occupancy_ref.py), which the GPU tests hold the kernels to, is itself checked on hand cases whose expected values
are plane distances written out, against a brute-force dilation, and -- independent of the walk -- for conservativeness
and tightness against points sampled densely along random rays.  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest

import occupancy_ref as oref
from abi_probe import L  # noqa: F401  (a fixture)
from nerf_fl_amd import _lib

F = np.float32
EINVAL, ESMALL = -1, -4


# ---- sizes and validation ------------------------------------------------------------------------------------------------

def test_size_queries(L):
    for nx, ny, nz in [(2, 2, 2), (33, 3, 2), (34, 5, 4), (66, 9, 7), (300, 6, 5)]:
        wx = (nx - 1 + 31) // 32
        assert L.nfl_occ_bytes(nx, ny, nz) == 4 * (nz - 1) * (ny - 1) * wx
        for d in (0, 8):
            # at least the two word arrays of the build: point flags and x-dilated rows, one bit per lattice point each
            assert L.nfl_occ_build_bytes(nx, ny, nz, d) >= 4 * nz * ny * ((nx + 31) // 32 + wx)
    assert L.nfl_occ_bytes(1, 5, 5) == 0 and L.nfl_occ_bytes(5, 5, 1) == 0
    assert L.nfl_occ_bytes(1024, 1024, 1025) == 0                      # more than 2^30 points
    assert L.nfl_occ_bytes(1024, 1024, 1024) == 4 * 1023 * 1023 * 32
    assert L.nfl_occ_build_bytes(5, 5, 5, -1) == 0 and L.nfl_occ_build_bytes(5, 5, 5, 9) == 0


def _build_args(L, nx=5, ny=4, nz=3, dilate=1):
    a = _lib.OccBuildArgs()
    a.d_lattice, a.nx, a.ny, a.nz, a.threshold, a.dilate = 0x1000, nx, ny, nz, 0.0, dilate
    a.d_scratch, a.scratch_bytes, a.d_bits = 0x2000, L.nfl_occ_build_bytes(nx, ny, nz, max(0, min(dilate, 8))), 0x3000
    return a


def test_build_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    assert L.nfl_occ_build(None, None) == EINVAL
    for field in ("d_lattice", "d_scratch", "d_bits"):
        a = _build_args(L)
        setattr(a, field, None)
        assert L.nfl_occ_build(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_lattice", 0x1002), ("d_bits", 0x3001), ("d_scratch", 0x2004)):
        a = _build_args(L)
        setattr(a, field, addr)
        assert L.nfl_occ_build(C.byref(a), None) == EINVAL, field
    for dims in ((1, 4, 3), (5, 1, 3), (5, 4, 1), (0, 4, 3), (-5, 4, 3), (5, 65536, 3), (1024, 1024, 1025)):
        a = _build_args(L)
        a.nx, a.ny, a.nz = dims
        a.scratch_bytes = 1 << 40
        assert L.nfl_occ_build(C.byref(a), None) == EINVAL, dims
    for d in (-1, 9, 100):
        a = _build_args(L, dilate=d)
        assert L.nfl_occ_build(C.byref(a), None) == EINVAL, d
    a = _build_args(L)
    a.scratch_bytes -= 1
    assert L.nfl_occ_build(C.byref(a), None) == ESMALL
    a.scratch_bytes = 0
    assert L.nfl_occ_build(C.byref(a), None) == ESMALL


def _clip_args(n_rays=4):
    a = _lib.OccClipArgs()
    a.d_rays, a.n_rays, a.d_bits, a.nx, a.ny, a.nz = 0x1000, n_rays, 0x2000, 5, 4, 3
    for k in range(3):
        a.lo[k], a.spacing[k] = -1.0, 0.5
    a.d_near_far, a.d_hit = 0x3000, 0x4000
    return a


def test_clip_refuses_before_any_launch(L):
    assert L.nfl_occ_clip_rays(None, None) == EINVAL
    for field in ("d_rays", "d_bits", "d_near_far", "d_hit"):
        a = _clip_args()
        setattr(a, field, None)
        assert L.nfl_occ_clip_rays(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_rays", 0x1008), ("d_bits", 0x2002), ("d_near_far", 0x3004)):
        a = _clip_args()
        setattr(a, field, addr)
        assert L.nfl_occ_clip_rays(C.byref(a), None) == EINVAL, field
    for dims in ((1, 4, 3), (5, 1, 3), (5, 4, 1)):
        a = _clip_args()
        a.nx, a.ny, a.nz = dims
        assert L.nfl_occ_clip_rays(C.byref(a), None) == EINVAL, dims
    for n in (-1, 1 << 31):
        assert L.nfl_occ_clip_rays(C.byref(_clip_args(n)), None) == EINVAL, n
    for bad in (0.0, -0.5, float("nan"), float("inf")):
        a = _clip_args()
        a.spacing[1] = bad
        assert L.nfl_occ_clip_rays(C.byref(a), None) == EINVAL, bad
    a = _clip_args()
    a.lo[2] = float("nan")
    assert L.nfl_occ_clip_rays(C.byref(a), None) == EINVAL
    # no rays: NFL_OK without a launch, whatever the pointers
    a = _clip_args(0)
    a.d_rays = a.d_bits = a.d_near_far = a.d_hit = None
    assert L.nfl_occ_clip_rays(C.byref(a), None) == 0


# ---- the restatement on hand cases: 4 x 4 x 4 cells with planes at the integers 0 .. 4, cell (1, 2, 1) occupied ---------

LO, SP = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _one_cell():
    dense = np.zeros((4, 4, 4), dtype=bool)
    dense[1, 2, 1] = True                                            # [k, j, i]: x in [1, 2], y in [2, 3], z in [1, 2]
    return dense


def _clip1(o, d, near, far, dense=None):
    nf, hit = oref.clip(np.array([list(o) + list(d) + [near, far]], dtype=F), _one_cell() if dense is None else dense, LO, SP)
    return float(nf[0, 0]), float(nf[0, 1]), bool(hit[0])


def test_axis_aligned_ray_through_the_cell():
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 0.0, 10.0) == (2.0, 3.0, True)      # planes x = 1 and x = 2, 1 away from o = -1
    assert _clip1((5, 2.5, 1.5), (-1, 0, 0), 0.0, 10.0) == (3.0, 4.0, True)      # the same planes from the other side
    assert _clip1((1.5, 2.5, 6), (0, 0, -2), 0.0, 10.0) == (2.0, 2.5, True)      # |d| = 2: z = 2 at (2 - 6) / -2, z = 1 at 2.5
    # a diagonal in the plane z = 1.5: p(t) = (t, 1.25 + t): x in [1, 2] for t in [1, 2], y in [2, 3] for t in [0.75, 1.75]
    assert _clip1((0, 1.25, 1.5), (1, 1, 0), 0.0, 10.0) == (1.0, 1.75, True)


def test_ray_that_misses():
    assert _clip1((-1, 0.5, 0.5), (1, 0, 0), 0.0, 10.0) == (0.0, 10.0, False)    # through the box, not through the cell
    assert _clip1((-1, 7.0, 0.5), (1, 0, 0), 0.25, 10.0) == (0.25, 10.0, False)  # past the box
    assert _clip1((-1, 2.5, 1.5), (-1, 0, 0), 0.0, 10.0) == (0.0, 10.0, False)   # away from it


def test_origin_inside_the_occupied_cell():
    assert _clip1((1.5, 2.5, 1.5), (1, 0, 0), 0.25, 10.0) == (0.25, 0.5, True)   # near' == near; leaves through x = 2
    assert _clip1((1.5, 2.5, 1.5), (0, 0, 0), 0.25, 10.0) == (0.25, 10.0, True)  # going nowhere: all of [near, far]


def test_zero_direction_component_on_and_off_the_slab():
    assert _clip1((1.5, -1, 1.5), (0, 1, 0), 0.0, 10.0) == (3.0, 4.0, True)      # y = 2 and y = 3 from y = -1
    assert _clip1((5.0, -1, 1.5), (0, 1, 0), 0.0, 10.0) == (0.0, 10.0, False)    # x = 5 is off the slab [0, 4]
    assert _clip1((1.5, -1, -0.5), (0, 1, 0), 0.0, 10.0) == (0.0, 10.0, False)
    assert _clip1((4.0, -1, 1.5), (0, 1, 0), 0.0, 10.0, np.ones((4, 4, 4), dtype=bool)) == (1.0, 5.0, True)   # ON the slab's end


def test_near_not_below_far():
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 5.0, 5.0) == (5.0, 5.0, False)
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 6.0, 2.0) == (6.0, 2.0, False)
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 2.5, 2.5) == (2.5, 2.5, False)      # inside the cell, but an empty interval


def test_nan_ray_is_a_miss_and_passes_through():
    base = [-1, 2.5, 1.5, 1, 0, 0, 0.0, 10.0]
    for col in range(8):
        ray = np.array([base], dtype=F)
        ray[0, col] = np.nan
        nf, hit = oref.clip(ray, np.ones((4, 4, 4), dtype=bool), LO, SP)
        assert not hit[0], col
        assert np.array_equal(nf[0], ray[0, 6:8], equal_nan=True), col


def test_far_ending_inside_the_cell():
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 0.0, 2.5) == (2.0, 2.5, True)
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 2.25, 2.5) == (2.25, 2.5, True)     # and near inside it too
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 0.0, 2.0) == (0.0, 2.0, False)      # far ON its first plane: nothing of it seen


def test_two_cells_give_first_entry_and_last_exit():
    dense = _one_cell()
    dense[1, 2, 3] = True                                            # x in [3, 4], a gap at [2, 3]
    assert _clip1((-1, 2.5, 1.5), (1, 0, 0), 0.0, 10.0, dense) == (2.0, 5.0, True)


@pytest.mark.parametrize("cx", [31, 32, 33, 65])
def test_packing_and_tail_bits(cx):
    rng = np.random.default_rng(cx)
    dense = rng.random((3, 2, cx)) < 0.5
    dense[:, :, cx - 1] = True                                       # the last cell of every row is set ...
    bits = oref.pack(dense)
    wx = (cx + 31) // 32
    assert bits.shape == (3, 2, wx) and bits.dtype == np.uint32
    for k, j, i in [(0, 0, 0), (2, 1, cx - 1), (1, 0, cx // 2), (1, 1, 31 if cx > 31 else 30)]:
        assert bool((int(bits[k, j, i >> 5]) >> (i & 31)) & 1) == bool(dense[k, j, i])
    if cx & 31:                                                      # ... and nothing above it in the last word
        assert (bits[:, :, -1] >> np.uint32(cx & 31) == 0).all()
    assert int(sum(bin(int(w)).count("1") for w in bits.ravel())) == int(dense.sum())
    assert np.array_equal(oref.unpack(bits, cx), dense)
    # a full lattice through the build: every cell set, the tail still zero
    full = oref.build_bits(np.ones((3, 3, cx + 1), dtype=F), 0.5, 8)
    last = (1 << (cx & 31)) - 1 if cx & 31 else 0xFFFFFFFF
    assert (full[:, :, :-1] == 0xFFFFFFFF).all() and (full[:, :, -1] == last).all()


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_separable_dilation_is_the_brute_force_one(d):
    rng = np.random.default_rng(40 + d)
    for shape, share in (((6, 7, 9), 0.03), ((4, 9, 40), 0.01), ((2, 2, 2), 0.3), ((9, 3, 5), 0.1)):
        lat = (rng.random(shape) < share).astype(F)
        a, b = oref.build_dense(lat, 0.5, d), oref.build_dense_brute(lat, 0.5, d)
        assert a.shape == tuple(n - 1 for n in shape) and np.array_equal(a, b), (shape, d)
    one = np.zeros((12, 12, 12), dtype=F)
    one[6, 5, 4] = 1.0                                               # one point: the 2^3 cells around it, grown by d each way
    exp = np.zeros((11, 11, 11), dtype=bool)
    exp[5 - d:7 + d, 4 - d:6 + d, 3 - d:5 + d] = True
    assert np.array_equal(oref.build_dense(one, 0.5, d), exp)


def test_nan_and_infinite_lattice_values():
    lat = np.zeros((2, 2, 4), dtype=F)
    lat[0, 0, :] = [np.nan, -np.inf, np.inf, 0.0]
    assert oref.inside(lat, 0.5)[0, 0].tolist() == [False, False, True, False]
    assert oref.inside(lat, np.inf)[0, 0].tolist() == [False, False, True, False]      # inf >= inf
    assert oref.inside(lat, -np.inf)[0, 0].tolist() == [False, True, True, True]       # all but the NaN
    assert oref.inside(lat, np.nan).sum() == 0
    lat[:] = -1.0
    lat[0, 0, :] = [np.nan, -np.inf, np.inf, -1.0]
    assert oref.build_dense(lat, 0.0, 0)[0, 0].tolist() == [False, True, True]         # only the cells touching +inf


# ---- conservativeness and tightness of the definition, independent of the walk -----------------------------------------

def test_clip_is_conservative_and_tight():
    """Judged in fp64 on the cells themselves (their faces are the fp32 planes, taken as exact), not by another walk.

    eps: near' and far' are ((plane - o) * inv) with inv = 1 / d: a subtraction, a division and a product, each within
    half an ulp, so at most 1.5 ulp of the parameter itself, which is at most far: 4 ulp of far covers it."""
    rng = np.random.default_rng(2024)
    cx, cy, cz = 37, 21, 13
    dense = rng.random((cz, cy, cx)) < 0.3
    lo = np.array([-1.3, -0.7, -0.4], dtype=F)
    sp = np.array([0.07, 0.1, 0.09], dtype=F)
    pl = [oref.planes(lo[k], sp[k], n + 1).astype(np.float64) for k, n in enumerate((cx, cy, cz))]
    hi = [p[-1] for p in pl]
    rays = oref.random_rays(rng, 2000, lo.astype(np.float64), hi)
    nf, hit = oref.clip(rays, dense, lo, sp)
    assert 0.2 < hit.mean() < 0.98                                   # the sample has both kinds
    r64 = rays.astype(np.float64)
    o, d, near, far = r64[:, :3], r64[:, 3:6], r64[:, 6], r64[:, 7]
    eps = 4 * np.spacing(np.abs(rays[:, 7])).astype(np.float64)

    def cells_of(p, margin):
        """(index (..., 3), ok (...)): the cell of every point; ok when it lies in the grid, `margin` cells off every face."""
        idx, ok = np.zeros(p.shape, dtype=np.int64), np.ones(p.shape[:-1], dtype=bool)
        for k, n in enumerate((cx, cy, cz)):
            i = np.searchsorted(pl[k], p[..., k], side="right") - 1
            inside = (i >= 0) & (i < n)
            i = np.clip(i, 0, n - 1)
            m = margin * (pl[k][i + 1] - pl[k][i])
            ok &= inside & (p[..., k] - pl[k][i] >= m) & (pl[k][i + 1] - p[..., k] >= m)
            idx[..., k] = i
        return idx, ok

    steps = np.linspace(0.0, 1.0, 4000)
    worst = 0.0
    for r0 in range(0, len(rays), 250):
        s = slice(r0, r0 + 250)
        t = near[s, None] + (far[s] - near[s])[:, None] * steps[None, :]
        p = o[s, None, :] + t[..., None] * d[s, None, :]
        idx, ok = cells_of(p, 1e-4)
        occ = ok & dense[idx[..., 2], idx[..., 1], idx[..., 0]]
        assert not (occ & ~hit[s, None]).any()                       # a ray that sees an occupied cell is a hit
        lo_gap = np.where(occ, nf[s, 0:1].astype(np.float64) - t, -np.inf).max()
        hi_gap = np.where(occ, t - nf[s, 1:2].astype(np.float64), -np.inf).max()
        over = np.where(occ, np.maximum(nf[s, 0:1] - t, t - nf[s, 1:2]) - eps[s, None], -np.inf).max()
        worst = max(worst, lo_gap, hi_gap)
        assert over <= 0.0, (r0, over)
    print(f"conservativeness: worst t outside [near', far'] over 8e6 points: {worst:.3e} (eps up to {eps.max():.3e})")

    # tightness: the ends that moved sit ON an occupied cell: within 1e-4 of a cell size of one (the parameter is rounded)
    def touches_occupied(p):
        got = np.zeros(len(p), dtype=bool)
        for corner in range(8):
            q = p.copy()
            for k in range(3):
                q[:, k] += (1 if (corner >> k) & 1 else -1) * 1e-4 * float(sp[k])
            idx, ok = cells_of(q, 0.0)
            got |= ok & dense[idx[..., 2], idx[..., 1], idx[..., 0]]
        return got

    h = np.nonzero(hit)[0]
    assert (nf[h, 0] >= rays[h, 6]).all() and (nf[h, 1] <= rays[h, 7]).all() and (nf[h, 0] < nf[h, 1]).all()
    moved_near = h[nf[h, 0] > rays[h, 6]]
    moved_far = h[nf[h, 1] < rays[h, 7]]
    assert len(moved_near) > 100 and len(moved_far) > 100
    assert touches_occupied(o[moved_near] + nf[moved_near, 0:1].astype(np.float64) * d[moved_near]).all()
    assert touches_occupied(o[moved_far] + nf[moved_far, 1:2].astype(np.float64) * d[moved_far]).all()
    miss = ~hit
    assert np.array_equal(nf[miss], rays[miss, 6:8])


def test_ball_frame_hit_share():
    """The end-to-end GPU test's scene, on the CPU first: a ball of radius 1.2 at 32^3 cells over [-1.5, 1.5]^3 with one
    cell of dilation, seen by the fov-60 camera from (0, 0, 4) on 48 x 48 pixels.  The ball itself covers
    pi tan^2(asin 0.3) / (2 tan 30 deg)^2 = 23 % of the frame; voxelisation and dilation add to that."""
    lat, lo, hi = oref.ball_lattice(32, 1.2, 1.5)
    dense = oref.build_dense(lat, 0.0, 1)
    assert 4 / 3 * np.pi * 1.2 ** 3 / 27 < dense.mean() < 0.6         # at least the ball's own share of the box
    rays = oref.pinhole_rays(48, 48, 4.0, 2.0, 6.0)
    nf, hit = oref.clip(rays, dense, lo, oref.spacing_of(lo, hi, lat.shape))
    analytic = np.pi * np.tan(np.arcsin(0.3)) ** 2 / (2 * np.tan(np.pi / 6)) ** 2
    print(f"ball frame: hit share {hit.mean():.4f}, the ball alone {analytic:.4f}")
    assert analytic <= hit.mean() and 0.15 < hit.mean() < 0.45
    assert hit.reshape(48, 48)[24, 24] and not hit.reshape(48, 48)[0, 0]
    centre = nf.reshape(48, 48, 2)[24, 24]                           # straight down the axis: the dilated ball's two ends
    assert 4 - 1.5 <= centre[0] <= 4 - 1.2 and 4 + 1.2 <= centre[1] <= 4 + 1.5
