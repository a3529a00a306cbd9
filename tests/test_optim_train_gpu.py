"""RayTrainer with the reference's other optimiser settings (opt.py --optimizer / --weight_decay / --lr_scheduler /
--warmup_epochs), eager and graphed, on the small synthetic scene of test_train_gpu.py.  Coarse + fine fields without
appearance / transient embeddings: their gradients are the only ones the backward accumulates with atomics, so without
them a run is reproducible and its PSNR margin means the same on every run."""
import pytest
import torch

from oracle import nerfw_oracle as orc

pytestmark = pytest.mark.gpu


def _scene():
    import gpu_util
    dev = gpu_util.DEV
    spec = orc.FieldSpec("coarse")
    teacher = orc.make_field_params(spec, 21, "sharp")
    rays, val = orc.make_rays(4096, 31), orc.make_rays(512, 32)
    with torch.no_grad():
        kw = dict(n_samples=48, white_back=True, noise_std=0.0)
        rgb = orc.render_rays(spec, teacher, None, None, rays, **kw)["rgb_coarse"]
        vrgb = orc.render_rays(spec, teacher, None, None, val, **kw)["rgb_coarse"]
    ts = torch.randint(0, 8, (4096,), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    vts = torch.zeros(512, dtype=torch.long, device=dev)
    return dev, rays.to(dev), rgb.to(dev), ts, val.to(dev), vrgb.to(dev), vts


# RAdam / Ranger move little in their first, un-rectified steps (and the rectification term is ~0.1 .. 0.3 over the 24
# steps here): a larger base rate than Adam's
CASES = [dict(optimizer="sgd", lr=0.5, momentum=0.9), dict(optimizer="radam", lr=5e-3), dict(optimizer="ranger", lr=5e-3),
    dict(optimizer="adam", lr=5e-4, weight_decay=1e-4, warmup_epochs=2, lr_scheduler="steplr", decay_step=(2,))]


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["optimizer"])
def test_trainer_fits_with_the_reference_optimizers(case, graph, tmp_path):
    from nerf_fl_amd import train
    from nerf_fl_amd.train import RayTrainer
    dev, rays, rgb, ts, val, vrgb, vts = _scene()
    tr = RayTrainer(dev, N_samples=32, N_importance=32, batch_size=512,
                    num_epochs=3, use_graph=graph, **case)
    assert type(tr.opt) is {"sgd": train.SGD, "adam": train.Adam, "radam": train.RAdam, "ranger": train.Ranger}[
        case["optimizer"]] and tr.opt.capturable == graph
    p0 = tr.validate(val, vrgb, vts)
    lrs = []
    for _ in range(3):
        lrs.append(tr.opt.param_groups[0]["lr"])
        loss, _psnr = tr.fit_epoch(rays, rgb, ts)
        assert loss == loss
    p1 = tr.validate(val, vrgb, vts)
    print(f"{case} graph={graph}: PSNR {p0:.2f} -> {p1:.2f}, lr per epoch {lrs}")
    assert p1 > p0 + 6.0, (p0, p1)          # every case gained 9.6 .. 12.3 dB on the MI355X
    if case.get("warmup_epochs"):
        assert isinstance(tr.sched, train.GradualWarmupLR) and lrs == [5e-4] * 3     # multiplier 1: flat warm-up
    path = str(tmp_path / "ckpt" / "last.ckpt")
    tr.save(path, epoch=3)
    tr2 = RayTrainer(dev, N_samples=32, N_importance=32, batch_size=512,
                     seed=5, **case)
    tr2.load(path)
    assert abs(tr2.validate(val, vrgb, vts) - p1) < 1e-4


def test_default_trainer_is_the_adam_trainer():
    """RayTrainer() with the new arguments at their defaults: bit-identical parameters after one epoch to a trainer whose
    optimiser is replaced by a hand-built Adam(lr=5e-4, eps=1e-8)."""
    from nerf_fl_amd.train import Adam, RayTrainer
    dev, rays, rgb, ts, _, _, _ = _scene()
    out = []
    for by_hand in (False, True):
        tr = RayTrainer(dev, N_samples=32, N_importance=32, batch_size=512)
        assert tr.sched is None and type(tr.opt) is Adam and tr.opt.defaults["weight_decay"] == 0.0
        if by_hand:
            tr.opt = Adam(tr.params, lr=5e-4, eps=1e-8)
        tr.fit_epoch(rays, rgb, ts)
        out.append([p.detach().clone() for p in tr.params])
    assert all(torch.equal(a, b) for a, b in zip(*out))
