"""GPU checks of the occupancy feature: the build and clip kernels (csrc/nfl_occupancy.hip) against the numpy restatement
of tests/occupancy_ref.py, and the evaluation path on top of them (eval.clipped_inference, render_frame(occupancy=...)).

The bit grid is integer work: every word must be equal.  The hit flags must be equal too: a differing flag is a finding
to explain, never a tolerance to widen.  near' / far' follow the convention of the geometry tests: both sides evaluate
the same fp32 formulae with every operation rounded on its own (the library is built with -ffp-contract=off; division
is correctly rounded on both), so they can differ only where a compiler contracts or reorders.  MEASURED worst deviation
over all the cases below on an MI355X: 0.0 (bit-identical).  Allowed: 4 x the measured value, but at least 1 ulp of the
largest far of the rays.

The shapes are the smallest that cross the boundaries of the code: 32 cells of a word (cx = 32, 33, 65), the 64 lanes of
the flag pass's ballot, its 256-point workgroup (nx = 300), and 1 / 63 / 64 / 65 / 257 / 5000 rays for the clip's waves
and workgroups."""
import ctypes as C

import numpy as np
import pytest
import torch

import occupancy_ref as oref
from gpu_util import DEV
from nerf_fl_amd import NeRF, PosEmbedding, _lib, eval as nfl_eval, geometry, render_rays, rendering, synth

pytestmark = pytest.mark.gpu

F = np.float32
MEASURED = 0.0                  # see the module docstring
FWD_TOL = 1e-4                  # the project's forward bar


def _ulp(x):
    return float(np.spacing(F(x)))


def _bits(grid):
    return grid.bits.cpu().numpy().view(np.uint32)


def _build(lat, threshold, dilate, lo=(-1.0, 0.5, 2.0), hi=(2.0, 1.5, 2.75)):
    lat = np.ascontiguousarray(lat, dtype=F)
    grid = geometry.occupancy_grid(torch.from_numpy(lat).to(DEV), threshold, lo, hi, dilate=dilate)
    nz, ny, nx = lat.shape
    assert grid.cells == (nx - 1, ny - 1, nz - 1) and grid.bits.dtype == torch.int32
    assert tuple(grid.bits.shape) == (nz - 1, ny - 1, (nx - 1 + 31) // 32)
    return grid


def _check_build(lat, threshold, dilate, what):
    grid = _build(lat, threshold, dilate)
    got, exp = _bits(grid), oref.build_bits(lat, threshold, dilate)
    assert np.array_equal(got, exp), (what, int((got != exp).sum()), "words differ")
    cx = grid.cells[0]
    if cx & 31:
        assert (got[:, :, -1] >> np.uint32(cx & 31) == 0).all(), what           # tail bits zero
    return grid


# ---- build ---------------------------------------------------------------------------------------------------------------

def test_all_corner_patterns():
    """2 x 2 x 2: the one cell is occupied exactly when a corner is inside, at any dilation."""
    for pattern in range(256):
        lat = np.array([1.0 if (pattern >> c) & 1 else -1.0 for c in range(8)], dtype=F).reshape(2, 2, 2)
        for d in (0, 8):
            got = _bits(_check_build(lat, 0.0, d, f"pattern {pattern} dilate {d}"))
            assert got.shape == (1, 1, 1) and int(got[0, 0, 0]) == (1 if pattern else 0)


@pytest.mark.parametrize("shape", [(33, 3, 2), (34, 5, 4), (66, 9, 7), (300, 6, 5)])
def test_random_lattices(shape):
    """(nx, ny, nz).  33: 32 cells, one full word, and a second word of point flags that holds one point; 34: a tail of
    one cell; 66: three words; 300: two workgroups of the flag pass and a wave that ends inside the row."""
    nx, ny, nz = shape
    rng = np.random.default_rng(sum(shape))
    for d in (0, 1, 2, 3, 8):
        lat = np.where(rng.random((nz, ny, nx)) < 0.04, 1.0, -1.0).astype(F) * rng.uniform(0.5, 2.0, (nz, ny, nx)).astype(F)
        grid = _check_build(lat, 0.25, d, f"random {shape} dilate {d}")
        assert torch.equal(grid.to_dense().cpu(), torch.from_numpy(oref.build_dense(lat, 0.25, d)))
        assert grid.fraction() == pytest.approx(oref.build_dense(lat, 0.25, d).mean(), abs=1e-12)
    # the x pass's carries: one point at every place of the words around a boundary, nothing else
    for x in sorted({0, 1, 30, 31, 32, min(33, nx - 1), nx - 2, nx - 1}):
        lat = -np.ones((nz, ny, nx), dtype=F)
        lat[nz // 2, ny // 2, x] = 1.0
        for d in (0, 3, 8):
            _check_build(lat, 0.0, d, f"one point x={x} {shape} dilate {d}")


def test_nan_and_infinite_values():
    rng = np.random.default_rng(3)
    lat = rng.standard_normal((4, 5, 40)).astype(F)
    kind = rng.integers(0, 8, lat.shape)
    lat[kind == 0], lat[kind == 1], lat[kind == 2] = np.nan, np.inf, -np.inf
    for thr in (0.5, np.inf, -np.inf, np.nan):
        for d in (0, 1):
            _check_build(lat, thr, d, f"non-finite threshold {thr} dilate {d}")
    only_nan = np.full((3, 3, 35), np.nan, dtype=F)
    assert not _bits(_check_build(only_nan, -np.inf, 2, "all NaN")).any()


def test_empty_and_full_lattices():
    for shape in ((2, 2, 2), (3, 4, 33), (5, 3, 70)):
        nz, ny, nx = shape
        cx = nx - 1
        last = (1 << (cx & 31)) - 1 if cx & 31 else 0xFFFFFFFF
        for d in (0, 1, 8):
            assert not _bits(_check_build(-np.ones(shape, dtype=F), 0.0, d, f"empty {shape}")).any()
            full = _bits(_check_build(np.ones(shape, dtype=F), 0.0, d, f"full {shape}"))
            assert (full[:, :, :-1] == 0xFFFFFFFF).all() and (full[:, :, -1] == last).all()


def test_two_runs_give_the_same_bits():
    rng = np.random.default_rng(11)
    lat = rng.standard_normal((9, 17, 131)).astype(F)
    a, b = _bits(_build(lat, 1.0, 2)), _bits(_build(lat, 1.0, 2))
    assert np.array_equal(a, b) and np.array_equal(a, oref.build_bits(lat, 1.0, 2))


def test_python_refuses_bad_arguments():
    lat = torch.zeros(3, 3, 3, device=DEV)
    with pytest.raises(ValueError):
        geometry.occupancy_grid(lat, 0.0, (0, 0, 0), (1, 1, 1), dilate=9)
    with pytest.raises(ValueError):
        geometry.occupancy_grid(lat.double(), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError):
        geometry.occupancy_grid(lat.cpu(), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(TypeError):
        geometry.occupancy_grid(lat, lo=(0, 0, 0), hi=(1, 1, 1))                 # threshold has no default
    grid = geometry.occupancy_grid(lat, 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        geometry.clip_rays(grid, torch.zeros(4, 7, device=DEV))
    with pytest.raises(ValueError):
        geometry.clip_rays(None, torch.zeros(4, 8, device=DEV))


# ---- clip ----------------------------------------------------------------------------------------------------------------

N_RAYS = 5000
SIZES = (1, 63, 64, 65, 257, N_RAYS)


def _grid_of(dense, lo, sp):
    """An OccupancyGrid around the restatement's packed words (any cell pattern, not only what a lattice can give)."""
    cz, cy, cx = dense.shape
    bits = torch.from_numpy(oref.pack(dense).view(np.int32)).to(DEV)
    return geometry.OccupancyGrid(bits, [float(v) for v in lo], [float(v) for v in sp], (cx, cy, cz), 0.0, 0)


def _special_rays(rays, lo, sp, cells):
    """Overwrite the first rows with the cases random rays do not produce."""
    pl = [oref.planes(lo[k], sp[k], cells[k] + 1) for k in range(3)]
    mid = [float(p[len(p) // 2 - 1]) + 0.37 * float(sp[k]) for k, p in enumerate(pl)]
    far = 40.0
    rows = [
        [np.nan, mid[1], mid[2], 1, 0, 0, 0, far], [mid[0], mid[1], mid[2], 0, np.nan, 1, 0, far],
        [mid[0], mid[1], mid[2], 0, 0, 1, np.nan, far], [mid[0], mid[1], mid[2], 0, 0, 1, 0, np.nan],
        [float(pl[0][0]) - 1, mid[1], mid[2], 1, 0, 0, 3.0, 3.0],                                  # near == far
        [float(pl[0][0]) - 1, mid[1], mid[2], 1, 0, 0, 5.0, 2.0],                                  # near > far
        [float(pl[0][0]) - 1, mid[1], mid[2], 1, 0, 0, 0, far], [float(pl[0][-1]) + 1, mid[1], mid[2], -3, 0, 0, 0, far],
        [mid[0], float(pl[1][0]) - 1, mid[2], 0, 0.5, 0, 0, far], [mid[0], mid[1], float(pl[2][-1]) + 2, 0, 0, -1, 0, far],
        [float(pl[0][0]) - 1, float(pl[1][0]) - 0.5, mid[2], 1, 0, 0, 0, far],                     # off the y slab, d_y = 0
        [float(pl[0][-1]), float(pl[1][0]) - 1, mid[2], 0, 1, 0, 0, far],                          # ON the last x plane
        [float(pl[0][3]), float(pl[1][0]) - 1, mid[2], 0, 1, 0, 0, far],                           # along an inner plane
        [mid[0], mid[1], mid[2], 0, 0, 0, 0.5, 2.0],                                               # going nowhere, inside
        [mid[0], mid[1], float(pl[2][0]) - 1, 0, 0, 0, 0.5, 2.0],                                  # going nowhere, outside
        # through cell corners: all three planes tie at every step
        [float(pl[0][0]) - float(sp[0]), float(pl[1][0]) - float(sp[1]), float(pl[2][0]) - float(sp[2]),
         float(sp[0]), float(sp[1]), float(sp[2]), 0, far],
        [float(pl[0][2]), float(pl[1][2]), float(pl[2][2]), -float(sp[0]), float(sp[1]), float(sp[2]), -1.0, far],
        [mid[0], mid[1], mid[2], 1e-30, 1, -1e-30, 0, far],                                        # a huge 1 / d
        [mid[0], mid[1], mid[2], 1, 2, 3, -50.0, 50.0],                                            # near behind the origin
        [mid[0], mid[1], mid[2], 1, 2, 3, 0.0, np.inf],                                            # far = inf: the box ends it
    ]
    rays[:len(rows)] = np.array(rows, dtype=F)
    return rays


def _case(name):
    rng = np.random.default_rng({"empty": 1, "full": 2, "random": 3, "shell": 4}[name])
    if name == "shell":
        cells = (64, 64, 64)
        lo, sp = np.array([-1, -1, -1], dtype=F), oref.spacing_of((-1,) * 3, (1,) * 3, (65, 65, 65))
        ax = [oref.planes(lo[k], sp[k], 65).astype(np.float64) for k in range(3)]
        zz, yy, xx = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
        dense = oref.build_dense(0.04 - np.abs(np.sqrt(xx * xx + yy * yy + zz * zz) - 0.7), 0.0, 0)
    else:
        cells = (37, 21, 13)
        lo, sp = np.array([-1.3, -0.7, -0.4], dtype=F), np.array([0.07, 0.1, 0.09], dtype=F)
        shape = cells[::-1]
        dense = {"empty": np.zeros(shape, dtype=bool), "full": np.ones(shape, dtype=bool),
                 "random": rng.random(shape) < 0.3}[name]
    hi = [float(oref.planes(lo[k], sp[k], cells[k] + 1)[-1]) for k in range(3)]
    rays = _special_rays(oref.random_rays(rng, N_RAYS, lo.astype(np.float64), hi), lo, sp, cells)
    return dense, lo, sp, rays


def _clip_framed(grid, rays):
    """nfl_occ_clip_rays through the C ABI with the outputs inside larger, sentinel-filled buffers."""
    R = rays.shape[0]
    d_rays = torch.from_numpy(rays).to(DEV)
    nf = torch.full((R + 4, 2), -777.0, dtype=torch.float32, device=DEV)
    hit = torch.full((R + 32,), 0xAB, dtype=torch.uint8, device=DEV)
    a = _lib.OccClipArgs()
    a.d_rays, a.n_rays, a.d_bits = d_rays.data_ptr(), R, grid.bits.data_ptr()
    a.nx, a.ny, a.nz = (c + 1 for c in grid.cells)
    for k in range(3):
        a.lo[k], a.spacing[k] = grid.lo[k], grid.spacing[k]
    a.d_near_far, a.d_hit = nf[2:].data_ptr(), hit[16:].data_ptr()
    _lib.check(_lib.lib().nfl_occ_clip_rays(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "clip")
    nf, hit = nf.cpu().numpy(), hit.cpu().numpy()
    assert (nf[:2] == -777.0).all() and (nf[R + 2:] == -777.0).all(), "near_far written outside its R rows"
    assert (hit[:16] == 0xAB).all() and (hit[R + 16:] == 0xAB).all(), "hit written outside its R entries"
    return nf[2:R + 2], hit[16:R + 16]


def _deviation(got, exp):
    same = (got == exp) | (np.isnan(got) & np.isnan(exp))
    with np.errstate(invalid="ignore"):
        d = np.where(same, 0.0, np.abs(got.astype(np.float64) - exp.astype(np.float64)))
    return float(np.nan_to_num(d, nan=np.inf).max()) if d.size else 0.0


@pytest.mark.parametrize("name", ["empty", "full", "random", "shell"])
def test_clip_against_the_restatement(name):
    dense, lo, sp, rays = _case(name)
    grid = _grid_of(dense, lo, sp)
    exp_nf, exp_hit = oref.clip(rays, dense, lo, sp)                 # once, for all sizes: rays are independent
    if name == "empty":
        assert not exp_hit.any()
    else:
        assert 0.1 < exp_hit.mean() < 0.99
    finite_far = rays[:, 7][np.isfinite(rays[:, 7])]
    tol = max(4 * MEASURED, _ulp(np.abs(finite_far).max()))
    worst = 0.0
    for R in SIZES:
        got_nf, got_hit = _clip_framed(grid, rays[:R])
        assert set(np.unique(got_hit)) <= {0, 1}
        differ = np.nonzero(got_hit.astype(bool) != exp_hit[:R])[0]
        assert len(differ) == 0, (name, R, "hit flags differ at rays", differ[:10].tolist(), rays[differ[:3]].tolist())
        dev = _deviation(got_nf, exp_nf[:R])
        worst = max(worst, dev)
        assert dev <= tol, (name, R, dev, tol)
        miss = ~exp_hit[:R]
        assert np.array_equal(got_nf[miss], rays[:R][miss, 6:8], equal_nan=True)        # passed through bit for bit
    print(f"clip {name}: hit share {exp_hit.mean():.3f}, worst near'/far' deviation {worst:.3e} (allowed {tol:.3e})")


def test_clip_rays_returns_a_copy_and_a_bool_flag():
    dense, lo, sp, rays = _case("random")
    grid = _grid_of(dense, lo, sp)
    exp_nf, exp_hit = oref.clip(rays[:300], dense, lo, sp)
    wide = torch.zeros(300, 9, device=DEV)
    wide[:, 1:] = torch.from_numpy(rays[:300]).to(DEV)
    view = wide[:, 1:]                                               # neither contiguous nor 16-byte aligned
    before = view.clone()
    out, hit = geometry.clip_rays(grid, view)
    assert hit.dtype == torch.bool and hit.shape == (300,) and out.shape == (300, 8) and out.is_contiguous()
    assert np.array_equal(view.cpu().numpy(), before.cpu().numpy(), equal_nan=True)     # the input is left alone
    assert np.array_equal(out[:, :6].cpu().numpy(), rays[:300, :6], equal_nan=True)
    assert np.array_equal(hit.cpu().numpy(), exp_hit)
    assert _deviation(out[:, 6:].cpu().numpy(), exp_nf) <= _ulp(40.0)
    out0, hit0 = geometry.clip_rays(grid, torch.zeros(0, 8, device=DEV))
    assert out0.shape == (0, 8) and hit0.shape == (0,)


# ---- identity --------------------------------------------------------------------------------------------------------------

def _models(nerfw):
    kw = dict(encode_appearance=True, encode_transient=True) if nerfw else {}
    coarse, fine = NeRF("coarse"), NeRF("fine", **kw)
    coarse.load_state_dict(synth.make_field_params(21, "sharp", typ="coarse"))
    fine.load_state_dict(synth.make_field_params(22, "sharp", typ="fine", **kw))
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    if nerfw:
        torch.manual_seed(5)
        emb["a"], emb["t"] = torch.nn.Embedding(64, 48).to(DEV), torch.nn.Embedding(64, 16).to(DEV)
    return {"coarse": coarse.to(DEV), "fine": fine.to(DEV)}, emb


def _worst(a, b):
    assert set(a) == set(b), set(a) ^ set(b)
    return max((a[k] - b[k]).abs().max().item() if a[k].numel() else 0.0 for k in a)


def test_full_grid_around_the_rays_changes_nothing():
    rays = synth.make_rays(700, 8).to(DEV)                           # origins near (0, 0, 4), depths 2 .. 6
    grid = geometry.occupancy_grid(torch.ones(9, 9, 9, device=DEV), 0.5, (-8, -8, -8), (8, 8, 8), dilate=0)
    assert grid.fraction() == 1.0
    out, hit = geometry.clip_rays(grid, rays)
    assert bool(hit.all()) and torch.equal(out, rays)                # near' == near and far' == far bit for bit
    models, emb = _models(False)
    with torch.no_grad():
        a = nfl_eval.clipped_inference(models, emb, rays, None, grid, 16, 16, chunk=256)
        b = nfl_eval.batched_inference(models, emb, rays, None, 16, 16, chunk=256)
    worst = _worst(a, b)
    print(f"identity: worst |clipped - batched| = {worst:.3e}")
    assert worst <= FWD_TOL
    rendering.check_status(torch.device(DEV))


# ---- end to end on a hand-made grid ----------------------------------------------------------------------------------------

H = W = 48
NEAR, FAR = 2.0, 6.0


@pytest.fixture(scope="module")
def ball():
    lat, lo, hi = oref.ball_lattice(32, 1.2, 1.5)
    grid = geometry.occupancy_grid(torch.from_numpy(lat).to(DEV), 0.0, lo, hi, dilate=1)
    assert np.array_equal(_bits(grid), oref.build_bits(lat, 0.0, 1))
    c2w = torch.eye(4)[:3].clone()
    c2w[2, 3] = 4.0                                                  # at (0, 0, 4), looking down -z at the origin
    K = nfl_eval.fov60_intrinsics(W, H)
    rays = nfl_eval.frame_rays(c2w, K, H, W, NEAR, FAR, DEV)
    models, emb = _models(True)
    g = torch.Generator().manual_seed(9)
    ts = (torch.arange(H * W) * 7 % 64).to(DEV)                      # a different id and code on every neighbouring ray
    a_emb = torch.randn(H * W, 48, generator=g).to(DEV)
    return dict(grid=grid, c2w=c2w, K=K, rays=rays, models=models, emb=emb, ts=ts, a_emb=a_emb, lat=lat, lo=lo, hi=hi)


@pytest.mark.parametrize("white_back", [False, True])
def test_clipped_frame_end_to_end(ball, white_back):
    s = ball
    B = H * W
    rays2, hit = geometry.clip_rays(s["grid"], s["rays"])
    share = hit.float().mean().item()
    analytic = np.pi * np.tan(np.arcsin(0.3)) ** 2 / (2 * np.tan(np.pi / 6)) ** 2
    print(f"ball frame: hit share {share:.4f} (the ball alone covers {analytic:.4f})")
    assert 0.15 < share < 0.45
    with torch.no_grad():
        out = nfl_eval.clipped_inference(s["models"], s["emb"], s["rays"], s["ts"], s["grid"], 16, 16, chunk=512,
                                         white_back=white_back, a_embedded=s["a_emb"])
        direct = render_rays(s["models"], s["emb"], rays2[hit].contiguous(), s["ts"][hit], 16, False, 0, 0, 16, 4096,
                             white_back, True, a_embedded=s["a_emb"][hit])
    assert not any(k.startswith("_") for k in out)
    assert set(out) == {k for k in direct if not k.startswith("_")}
    assert {"rgb_fine", "depth_fine", "beta", "weights_fine", "transient_sigmas"} <= set(out)
    worst = max((out[k][hit] - direct[k]).abs().max().item() for k in out)
    print(f"hit rows vs render_rays on the clipped rays: worst {worst:.3e}")
    assert worst <= FWD_TOL
    beta_min = s["models"]["fine"].beta_min
    for k, v in out.items():
        assert v.shape[0] == B and v.shape[1:] == direct[k].shape[1:], k
        fill = (1.0 if white_back else 0.0) if "rgb" in k else beta_min if k == "beta" else 0.0
        assert bool((v[~hit] == fill).all()), k                      # exactly the fill values
    rendering.check_status(torch.device(DEV))

    # the same through render_frame
    with torch.no_grad():
        img, res = nfl_eval.render_frame(s["models"], s["emb"], s["c2w"], s["K"], H, W, NEAR, FAR, 16, 16, ts=s["ts"],
                                         chunk=512, white_back=white_back, device=DEV, occupancy=s["grid"],
                                         a_embedded=s["a_emb"])
    assert img.shape == (H, W, 3) and img.dtype == torch.uint8
    assert set(res) == set(out) and all(torch.equal(res[k], out[k]) for k in out)
    assert torch.equal(img, nfl_eval.to_uint8(out["rgb_fine"]).view(H, W, 3))


def test_empty_grid_renders_nothing(ball):
    s = ball
    B = H * W
    empty = geometry.occupancy_grid(torch.from_numpy(-np.ones_like(s["lat"])).to(DEV), 0.0, s["lo"], s["hi"], dilate=1)
    assert empty.fraction() == 0.0
    with torch.no_grad():
        ref = nfl_eval.clipped_inference(s["models"], s["emb"], s["rays"], s["ts"], s["grid"], 16, 16, chunk=512,
                                         a_embedded=s["a_emb"])
        for wb in (False, True):
            out = nfl_eval.clipped_inference(s["models"], s["emb"], s["rays"], s["ts"], empty, 16, 16, chunk=512,
                                             white_back=wb, a_embedded=s["a_emb"])
            assert set(out) == set(ref)
            for k, v in out.items():
                assert v.shape == ref[k].shape and v.dtype == ref[k].dtype, k
                fill = (1.0 if wb else 0.0) if "rgb" in k else s["models"]["fine"].beta_min if k == "beta" else 0.0
                assert bool((v == fill).all()), k
        # a broadcast (1, C) code stays broadcast, with and without hits
        one = s["a_emb"][:1]
        for g in (empty, s["grid"]):
            out = nfl_eval.clipped_inference(s["models"], s["emb"], s["rays"], s["ts"], g, 16, 16, chunk=512, a_embedded=one)
            assert out["rgb_fine"].shape == (B, 3)


# ---- plumbing from a field -------------------------------------------------------------------------------------------------

def test_grid_from_a_field():
    models, emb = _models(False)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (24, 24, 24)
    with torch.no_grad():
        lat = geometry.density_lattice(models["fine"], emb, lo, hi, res)
    thr = lat.median().item()
    grid = geometry.occupancy_grid(lat, thr, lo, hi)                 # dilate defaults to 1
    assert grid.dilate == 1 and grid.threshold == thr and grid.cells == (23, 23, 23)
    exp = oref.build_dense(lat.cpu().numpy(), thr, 1)
    assert torch.equal(grid.to_dense().cpu(), torch.from_numpy(exp))
    assert grid.fraction() == pytest.approx(exp.mean(), abs=1e-12) and exp.any()
    sp = oref.spacing_of(lo, hi, (24, 24, 24))
    assert np.array_equal(np.array(grid.spacing, dtype=F), sp) and grid.lo == lo
