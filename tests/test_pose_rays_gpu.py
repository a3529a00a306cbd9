"""HIP pose -> ray kernels (nfl_pose_rays / nfl_pose_rays_backward through nerf_fl_amd.poses.posed_rays) against the
reference's own pose path (tests/golden/g20_pose_rays.npz, written by tests/golden/make_pose_golden.py)."""
import pytest
import torch

import golden_util as gu
from nerf_fl_amd import check_status
from nerf_fl_amd.parallel import GradArena
from nerf_fl_amd.poses import LearnPose, get_rays, posed_rays

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# backward vs the fp64 reference, relative to max|g| of the tensor: the fp32 reference's own (1 - cos n)/n^2 cancellation
# sets the floor for 0 < |r| < 1e-2
TOL = {"zero": 1e-4, "1e-3": 1e-3, "1e-2": 1e-4, "large": 1e-4}


def _setup(tag, learn_R=True, learn_t=True):
    cfg, a = gu.load("g20_pose_rays")
    pose = LearnPose(cfg["n_cams"], learn_R, learn_t, a["init_c2w"].clone() if tag == "init" else None).to(DEV)
    with torch.no_grad():
        pose.r.copy_(a["r"])
        pose.t.copy_(a["t"])
    return cfg, a, pose, a["row_of_id"].to(DEV)


def _grads(pose, a, tab, arena=None, n=None):
    n = a["ts"].shape[0] if n is None else n
    out = posed_rays(pose, a["rays_cam"][:n].to(DEV), a["ts"][:n].to(DEV), tab, grad_arena=arena)
    (out * a["g_rays"][:n].to(DEV)).sum().backward()
    return out


@pytest.mark.parametrize("tag", ["init", "noinit"])
def test_forward_matches_reference(tag):
    _, a, pose, tab = _setup(tag)
    with torch.no_grad():
        got = posed_rays(pose, a["rays_cam"].to(DEV), a["ts"].to(DEV), tab).cpu()
    exp = a[f"rays_{tag}"]
    assert got.shape == exp.shape
    err = (got[:, :6] - exp[:, :6]).abs().max().item()
    print(f"forward ({tag}): max abs err {err:.2e}")
    assert err <= 2e-6, err
    assert torch.equal(got[:, 6:], exp[:, 6:])                     # near / far copied bit-exactly
    check_status(DEV)


@pytest.mark.parametrize("tag", ["init", "noinit"])
def test_backward_matches_reference_fp64(tag):
    cfg, a, pose, tab = _setup(tag)
    _grads(pose, a, tab)
    for name in ("r", "t"):
        got, exp = getattr(pose, name).grad.cpu().double(), a[f"g_{name}64_{tag}"]
        scale = exp.abs().max().item()
        for cls, (lo, hi) in cfg["classes"].items():
            err = (got[lo:hi] - exp[lo:hi]).abs().max().item() / scale
            print(f"backward ({tag}) d{name}, |r| class {cls}: max err / max|g| = {err:.2e}")
            assert err <= TOL[cls], (name, cls, err)


def test_backward_is_bit_reproducible_and_overwrites_the_arena():
    cfg, a, pose, tab = _setup("init")
    _grads(pose, a, tab)
    g1 = (pose.r.grad.clone(), pose.t.grad.clone())
    pose.r.grad = pose.t.grad = None
    _grads(pose, a, tab)
    assert torch.equal(pose.r.grad, g1[0]) and torch.equal(pose.t.grad, g1[1])
    # an arena view pre-filled with NaN is overwritten: every camera written, the absent one with exact zeros
    pose.r.grad = pose.t.grad = None
    arena = GradArena([pose.r, pose.t])
    arena.flat.fill_(float("nan"))
    for _ in range(2):                                              # twice: overwrite, never accumulate
        _grads(pose, a, tab, arena)
    assert pose.r.grad is arena.view(pose.r) and pose.t.grad is arena.view(pose.t)
    assert torch.equal(pose.r.grad, g1[0]) and torch.equal(pose.t.grad, g1[1])
    k = cfg["absent_row"]
    assert torch.equal(pose.r.grad[k].cpu(), torch.zeros(3)) and torch.equal(pose.t.grad[k].cpu(), torch.zeros(3))


def test_learn_R_or_t_off():
    _, a, full, tab = _setup("init")
    _grads(full, a, tab)
    for learn_R, learn_t in ((False, True), (True, False)):
        _, _, pose, _ = _setup("init", learn_R, learn_t)
        _grads(pose, a, tab)
        assert (pose.r.grad is None) != learn_R and (pose.t.grad is None) != learn_t
        if learn_R:
            assert torch.equal(pose.r.grad, full.r.grad)
        if learn_t:
            assert torch.equal(pose.t.grad, full.t.grad)


def test_empty_batch_writes_zeros():
    cfg, a, pose, tab = _setup("init")
    arena = GradArena([pose.r, pose.t])
    arena.flat.fill_(float("nan"))
    out = _grads(pose, a, tab, arena, n=0)
    assert out.shape == (0, 8)
    assert torch.equal(arena.flat.cpu(), torch.zeros_like(arena.flat.cpu()))


@pytest.mark.parametrize("n", [1, 63, 333])
def test_ragged_batches_match_torch(n):
    """Batches that fill no whole wavefront / block: the kernels against LearnPose + get_rays (fp64 autograd)."""
    _, a, pose, tab = _setup("init")
    out = _grads(pose, a, tab, n=n)
    ref = LearnPose(pose.num_cams, True, True, a["init_c2w"].clone()).double()
    with torch.no_grad():
        ref.r.copy_(a["r"].double())
        ref.t.copy_(a["t"].double())
    rows = tab.cpu()[a["ts"][:n]]
    o, d = get_rays(a["rays_cam"][:n, :3].double(), ref(rows))
    exp = torch.cat([o, d, a["rays_cam"][:n, 3:5].double()], 1)
    (exp * a["g_rays"][:n].double()).sum().backward()
    assert (out.detach().cpu().double() - exp.detach()).abs().max().item() <= 2e-6
    for name in ("r", "t"):
        g, e = getattr(pose, name).grad.cpu().double(), getattr(ref, name).grad
        assert (g - e).abs().max().item() <= 1e-3 * e.abs().max().item(), name


def test_bad_ids_give_nan_and_a_status_bit():
    cfg, a, pose, tab = _setup("init")
    check_status(DEV)
    ts = a["ts"][:64].clone()
    ts[3] = 0                                   # an id inside the table without a pose (row -1)
    ts[17] = tab.shape[0] + 1000                # an id beyond the table
    ts[40] = -5
    with torch.no_grad():
        out = posed_rays(pose, a["rays_cam"][:64].to(DEV), ts.to(DEV), tab).cpu()
    bad = torch.zeros(64, dtype=torch.bool)
    bad[[3, 17, 40]] = True
    assert torch.isnan(out[bad]).all() and torch.isfinite(out[~bad]).all()
    with pytest.raises(FloatingPointError, match="no pose"):
        check_status(DEV)
    check_status(DEV)                           # cleared; the device is healthy
    with torch.no_grad():
        assert torch.isfinite(posed_rays(pose, a["rays_cam"][:64].to(DEV), a["ts"][:64].to(DEV), tab)).all()
