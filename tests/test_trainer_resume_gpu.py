"""RayTrainer.save / resume: a run interrupted and resumed by a fresh trainer (another seed) continues bit-exactly --
eager, with a HIP graph captured BEFORE the resume, and with learnable poses across the BARF epoch boundary -- and a
checkpoint in the reference's Lightning layout continues like torch.optim.Adam would."""
import pytest
import torch
from torch import nn

from oracle import nerfw_oracle as orc

pytestmark = pytest.mark.gpu

KW = dict(N_samples=32, N_importance=32, batch_size=512, perturb=0.0, noise_std=0.0, optimizer="adam", lr=5e-4,
          lr_scheduler="cosine", warmup_epochs=1, warmup_multiplier=2.0, num_epochs=4)


def _scene(n=2048):
    """test_optim_train_gpu's scene: coarse + fine fields without latent tables (whose gradients are the only ones
    accumulated with atomics), so that a run is reproducible bit for bit."""
    import gpu_util
    dev = gpu_util.DEV
    spec = orc.FieldSpec("coarse")
    teacher = orc.make_field_params(spec, 21, "sharp")
    rays = orc.make_rays(n, 31)
    with torch.no_grad():
        rgb = orc.render_rays(spec, teacher, None, None, rays, n_samples=48, white_back=True, noise_std=0.0)["rgb_coarse"]
    ts = torch.zeros(n, dtype=torch.long, device=dev)
    return dev, rays.to(dev), rgb.to(dev), ts


def _epochs(tr, k, data, lrs):
    for _ in range(k):
        lrs.append(tr.opt.param_groups[0]["lr"])
        loss, _ = tr.fit_epoch(*data)
        assert loss == loss


def _state(tr):
    out = [p.detach().clone() for p in tr.params]
    for p in tr.params:
        st = tr.opt.state[p]
        out += [st["exp_avg"].clone(), st["exp_avg_sq"].clone()]
    return out, [int(tr.opt.state[p]["step"]) for p in tr.params]


def _check_resumed_run(make, epochs_before, data, tmp_path, capture_before=False):
    from nerf_fl_amd.train import RayTrainer
    full, lrs_full = make(3), []
    _epochs(full, epochs_before + 1, data, lrs_full)

    first, lrs = make(3), []
    _epochs(first, epochs_before, data, lrs)
    path = str(tmp_path / "ckpt" / "last.ckpt")
    first.save(path, epoch=epochs_before - 1)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["epoch"] == epochs_before - 1 and set(ck["state_dict"]) == set(first.state_dict())
    assert ck["global_step"] == first.global_step > 0 and len(ck["optimizer_states"]) == 1 and len(ck["lr_schedulers"]) == 1
    assert ck["nerf_fl_amd"]["current_epoch"] == epochs_before and ck["nerf_fl_amd"]["world_size"] == 1

    second = make(11)
    assert isinstance(second, RayTrainer)
    graphed = None
    if capture_before:                       # the fresh trainer trains an epoch of its own: its step gets captured
        second.fit_epoch(*data)
        graphed = second._graphed
        assert graphed is not None
    second.resume(path)
    assert second.current_epoch == epochs_before and second.global_step == first.global_step
    _epochs(second, 1, data, lrs)
    if capture_before:
        assert second._graphed is graphed    # the step captured before resume() is the one that replayed
    assert lrs == lrs_full, (lrs, lrs_full)
    (a, sa), (b, sb) = _state(full), _state(second)
    assert sa == sb
    bad = [i for i, (x, y) in enumerate(zip(a, b)) if not torch.equal(x, y)]
    assert not bad, f"{len(bad)} of {len(a)} tensors differ (first: {bad[0]})"


def test_resume_is_bit_exact(tmp_path):
    """3 uninterrupted epochs == 2 epochs, save, a fresh trainer with another seed resumes, 1 epoch: weights, Adam's
    moments and steps bitwise, and the per-epoch rates of the warm-up + cosine schedule."""
    from nerf_fl_amd.train import RayTrainer
    dev, rays, rgb, ts = _scene()
    _check_resumed_run(lambda seed: RayTrainer(dev, seed=seed, **KW), 2, (rays, rgb, ts), tmp_path)


def test_resume_keeps_a_step_captured_before_it_valid(tmp_path):
    """The same with use_graph=True, the fresh trainer's step captured (and replayed for an epoch) BEFORE resume():
    restoring in place leaves it replaying on live memory.  The backward runs in f16x3 here: the rounding seed of the
    default f16 backward is a by-value argument of the captured dgrad launch, so a graph captured by a trainer of another
    seed keeps its own draws (RayTrainer.resume documents it)."""
    import nerf_fl_amd
    from nerf_fl_amd.train import RayTrainer
    dev, rays, rgb, ts = _scene()
    fwd, bwd = nerf_fl_amd.get_precision(), nerf_fl_amd.rendering.get_backward_precision()
    nerf_fl_amd.set_precision(backward="f16x3")
    try:
        _check_resumed_run(lambda seed: RayTrainer(dev, seed=seed, use_graph=True, **KW), 2, (rays, rgb, ts), tmp_path,
                           capture_before=True)
    finally:
        nerf_fl_amd.set_precision(fwd, backward=bwd)


def _pose_scene():
    from nerf_fl_amd.poses import get_ray_directions
    import gpu_util
    dev = gpu_util.DEV
    n_cam, w = 3, 8
    K = torch.tensor([[8.0, 0, 4.0], [0, 8.0, 4.0], [0, 0, 1]])
    dirs = get_ray_directions(w, w, K).reshape(-1, 3)
    init = torch.eye(4)[None].repeat(n_cam, 1, 1)
    init[:, :3, 3] = torch.tensor([[0.1, -0.1, 4.0], [0.3, 0.2, 4.2], [-0.2, 0.1, 3.9]])
    n = n_cam * dirs.shape[0]
    rays = torch.cat([dirs.repeat(n_cam, 1), torch.tensor([2.0, 6.0]).expand(n, 2)], 1)
    ids = [5, 2, 9]
    ts = torch.tensor(ids).repeat_interleave(dirs.shape[0])
    rgb = torch.rand(n, 3, generator=torch.Generator().manual_seed(3))
    return dev, init, ids, (rays.to(dev), rgb.to(dev), ts.to(dev))


def test_resume_with_poses_across_the_barf_boundary(tmp_path):
    """refine_pose=True: 6 uninterrupted epochs == 5 epochs, save, resume, epoch 5 -- the BARF weights (embeddings
    (N-1, N, 4, 8): fractional from epoch 4) follow the resumed current_epoch; poses and their moments bitwise too."""
    from nerf_fl_amd.train import RayTrainer
    dev, init, ids, data = _pose_scene()
    kw = dict(KW, batch_size=64, num_epochs=8)

    def make(seed):
        return RayTrainer(dev, seed=seed, refine_pose=True, init_c2w=init, image_ids=ids, N_vocab=16, **kw)

    _check_resumed_run(make, 5, data, tmp_path)


@pytest.mark.parametrize("refine_pose", [False, True])
def test_resume_from_a_lightning_layout_checkpoint(refine_pose, tmp_path):
    """A checkpoint in the reference's layout: `state_dict` under every prefix including learn_poses.*, the optimiser
    state of torch.optim.Adam over get_parameters' list (learn_poses last, r / t frozen unless --refine_pose), a
    MultiStepLR's state.  After resume() one step equals torch.optim.Adam continuing from the same state."""
    import gpu_util
    from nerf_fl_amd.poses import LearnPose
    from nerf_fl_amd.train import RayTrainer
    dev = gpu_util.DEV
    n_cam = 4
    init = torch.eye(4)[None].repeat(n_cam, 1, 1)
    init[:, 2, 3] = torch.arange(n_cam, dtype=torch.float32)
    kw = dict(N_samples=32, N_importance=32, encode_a=True, encode_t=True, N_vocab=8, lr=5e-4, lr_scheduler="steplr",
              decay_step=(2,), decay_gamma=0.5)
    if refine_pose:
        kw.update(refine_pose=True, init_c2w=init)
    src = RayTrainer(dev, seed=1, **kw)
    modules = dict(src.modules)
    if not refine_pose:
        modules["learn_poses"] = LearnPose(n_cam, False, False, init).to(dev)
    ref = [nn.Parameter(p.detach().clone(), requires_grad=p.requires_grad) for m in modules.values() for p in m.parameters()]
    adam = torch.optim.Adam(ref, lr=5e-4, eps=1e-8)
    sched = torch.optim.lr_scheduler.MultiStepLR(adam, milestones=[2], gamma=0.5)
    g = torch.Generator().manual_seed(5)

    def grads():
        return [torch.randn(*p.shape, generator=g).to(dev) * 1e-2 for p in ref if p.requires_grad]

    for _epoch in range(3):
        for _step in range(2):
            for p, gr in zip([p for p in ref if p.requires_grad], grads()):
                p.grad = gr
            adam.step()
        sched.step()
    names = [f"{prefix}.{n}" for prefix, m in modules.items() for n, _ in m.named_parameters()]
    sd = {n: p.detach().cpu() for n, p in zip(names, ref)}
    path = str(tmp_path / "epoch=2.ckpt")
    torch.save({"epoch": 3, "global_step": 6, "state_dict": sd, "optimizer_states": [adam.state_dict()],
                "lr_schedulers": [sched.state_dict()]}, path)

    tr = RayTrainer(dev, seed=9, **kw)
    tr.resume(path)
    assert tr.current_epoch == 3 and tr.global_step == 6
    assert tr.opt.param_groups[0]["lr"] == adam.param_groups[0]["lr"] == 2.5e-4
    trainable = [p for p in ref if p.requires_grad]
    assert len(trainable) == len(tr.params) and tr.param_names() == [n for n, p in zip(names, ref) if p.requires_grad]
    for a, b in zip(trainable, tr.params):
        assert torch.equal(a.detach(), b.detach())
    tr.arena.attach()
    for a, b, gr in zip(trainable, tr.params, grads()):
        a.grad = gr
        b.grad.copy_(gr)
    adam.step()
    tr.opt.step()
    for a, b in zip(trainable, tr.params):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, a.abs().max().item())
    # the schedule continues from epoch 3 as the reference's would
    tr.sched.step()
    sched.step()
    assert tr.opt.param_groups[0]["lr"] == adam.param_groups[0]["lr"]
