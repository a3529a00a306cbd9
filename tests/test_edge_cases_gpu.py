"""Edge cases: empty and tiny batches, minimal and odd sample counts, against the CPU oracle."""
import pytest
import torch

from oracle import nerfw_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R,S,I", [(0, 8, 4), (1, 3, 1), (5, 8, 0), (3, 33, 31), (2, 1, 0), (7, 40, 5)])
def test_small_and_empty(R, S, I):
    import gpu_util
    from nerf_fl_amd import PosEmbedding, render_rays
    dev = gpu_util.DEV
    spec_c = orc.FieldSpec("coarse")
    spec_f = orc.FieldSpec("fine", encode_appearance=True, encode_transient=True, beta_min=0.1)
    P_c, P_f = orc.make_field_params(spec_c, 61, "sharp"), orc.make_field_params(spec_f, 62, "sharp")
    models = {"coarse": gpu_util.module_from(spec_c, P_c), "fine": gpu_util.module_from(spec_f, P_f)}
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    g = torch.Generator().manual_seed(R * 100 + S)
    rays = orc.make_rays(max(R, 1), 63)[:R]
    a_emb, t_emb = torch.randn(R, 48, generator=g), torch.randn(R, 16, generator=g)
    with torch.no_grad():
        got = render_rays(models, emb, rays.to(dev), torch.zeros(R, dtype=torch.long, device=dev), S, False, 0, 0.0, I,
                          32768, True, False, a_embedded=a_emb.to(dev), t_embedded=t_emb.to(dev))
        exp = orc.render_rays(spec_c, P_c, spec_f if I > 0 else None, P_f if I > 0 else None, rays, n_samples=S,
                              n_importance=I, noise_std=0.0, white_back=True, a_emb=a_emb, t_emb=t_emb)
    assert list(got.keys()) == list(exp.keys())
    for k in exp:
        assert tuple(got[k].shape) == tuple(exp[k].shape), k
        if R:
            assert (got[k].cpu() - exp[k]).abs().max().item() <= 1e-4, k


def small_case(R, S, I):
    """Fields, rays, target, latent codes and density noise of a tiny NeRF-W call (seeded)."""
    spec_c = orc.FieldSpec("coarse")
    spec_f = orc.FieldSpec("fine", encode_appearance=True, encode_transient=True, beta_min=0.1) if I > 0 else None
    P_c = orc.make_field_params(spec_c, 61, "sharp")
    P_f = orc.make_field_params(spec_f, 62, "sharp") if I > 0 else None
    g = torch.Generator().manual_seed(R * 100 + S)
    rays = orc.make_rays(R, 63)
    target = torch.rand(R, 3, generator=g)
    a_emb, t_emb = torch.randn(R, 48, generator=g), torch.randn(R, 16, generator=g)
    noise_coarse = torch.randn(R, S, generator=g)
    return spec_c, P_c, spec_f, P_f, rays, target, a_emb, t_emb, noise_coarse


def _small_backward_errors(R, S, I):
    """name -> (max abs error, max |oracle gradient|) of every parameter and latent gradient, at the oracle's fine depths."""
    import gpu_util
    from nerf_fl_amd import PosEmbedding, render_rays
    dev = gpu_util.DEV
    spec_c, P_c, spec_f, P_f, rays, target, a_emb, t_emb, noise_coarse = small_case(R, S, I)
    leaves = {}
    for tag, P in (("coarse", P_c), ("fine", P_f)):
        if P is not None:
            for n, p in P.items():
                leaves[f"{tag}.{n}"] = p.requires_grad_(True)
    a_o, t_o = a_emb.clone().requires_grad_(True), t_emb.clone().requires_grad_(True)
    res = orc.render_rays(spec_c, P_c, spec_f, P_f, rays, n_samples=S, n_importance=I, noise_std=1.0, white_back=True,
                          a_emb=a_o, t_emb=t_o, noise_coarse=noise_coarse, return_z=True)
    z_o = res.pop("_z_fine", None)
    loss_o = sum(orc.nerfw_loss(res, target).values())
    loss_o.backward()

    models = {"coarse": gpu_util.module_from(spec_c, {k: v.detach() for k, v in P_c.items()})}
    if I > 0:
        models["fine"] = gpu_util.module_from(spec_f, {k: v.detach() for k, v in P_f.items()})
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    a_h, t_h = a_emb.to(dev).requires_grad_(True), t_emb.to(dev).requires_grad_(True)
    extra = {"z_fine": z_o.to(dev)} if z_o is not None else {}
    out = render_rays(models, emb, rays.to(dev), torch.zeros(R, dtype=torch.long, device=dev), S, False, 0, 1.0, I, 32768,
                      True, False, a_embedded=a_h, t_embedded=t_h, noise_coarse=noise_coarse.to(dev), **extra)
    assert list(out.keys()) == list(res.keys())
    loss_h = sum(orc.nerfw_loss(out, target.to(dev)).values())
    loss_h.backward()
    assert abs(float(loss_h.detach()) - float(loss_o.detach())) <= 1e-4 * max(1.0, abs(float(loss_o.detach())))

    worst = {}
    for tag, m in models.items():
        for n, p in m.named_parameters():
            exp = leaves[f"{tag}.{n}"].grad
            worst[f"{tag}.{n}"] = ((p.grad.cpu() - exp).abs().max().item(), exp.abs().max().item())
    if I > 0:
        for key, got, exp in (("a_emb", a_h.grad, a_o.grad), ("t_emb", t_h.grad, t_o.grad)):
            worst[key] = ((got.cpu() - exp).abs().max().item(), exp.abs().max().item())
    return worst


@pytest.mark.parametrize("backward", ["f16", "f16w", "f16x3"])
@pytest.mark.parametrize("R,S,I", [(1, 3, 1), (2, 1, 0), (3, 33, 31), (7, 40, 5)])
def test_small_backward(R, S, I, backward):
    """The same tiny shapes with a loss and .backward(): fewer segments than a weight-gradient job has workgroups, rays
    whose last segment is mostly padding.  Gradients against the CPU oracle's autograd, as test_grad_variants_gpu.py
    compares them (every backward arithmetic; max error within GTOL of each tensor's largest gradient), with one
    difference: the oracle's fine depths are injected (`z_fine`), as test_parity_gpu.py::test_render_at_reference_depths
    does.  With so few rays the importance sampler's conditioning would decide the comparison otherwise: perturb = 0 draws
    u = 1, which flips between the last bin and the clamp when a coarse weight moves by 1e-7, and three moved depths among
    the 192 of (3, 33, 31) change the oracle's own fine-field gradients by 3e-2 of max|g|, three times GTOL
    (tests/test_sampler_conditioning_cpu.py measures this on the oracle alone)."""
    import nerf_fl_amd
    from test_grad_variants_gpu import GTOL
    nerf_fl_amd.set_precision("f16x3", backward=backward)
    try:
        worst = _small_backward_errors(R, S, I)
    finally:
        nerf_fl_amd.set_precision("f16x3", backward="f16")
    print(f"small backward R={R} S={S} I={I} {backward}: largest error / max|g| = "
          f"{max(e / r for e, r in worst.values() if r > 0):.3e}")
    bad = {k: v for k, v in worst.items() if not v[0] <= GTOL * v[1] + 1e-7}
    assert not bad, bad


def test_argument_errors():
    import gpu_util
    from nerf_fl_amd import NeRF, PosEmbedding, render_rays
    dev = gpu_util.DEV
    models = {"coarse": NeRF("coarse").to(dev)}
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    rays = orc.make_rays(4, 1).to(dev)
    ts = torch.zeros(4, dtype=torch.long, device=dev)
    with torch.no_grad():
        with pytest.raises(KeyError):                      # fine model missing, as in the reference
            render_rays(models, emb, rays, ts, 8, False, 0, 0, 4)
        with pytest.raises(TypeError):
            render_rays(models, emb, rays.double(), ts, 8)
        with pytest.raises(ValueError):
            render_rays(models, emb, rays[:, :6], ts, 8)
        with pytest.raises(ValueError):                    # embedding width does not match the model
            render_rays(models, {"xyz": PosEmbedding(14, 15), "dir": PosEmbedding(3, 4)}, rays, ts, 8)


def test_parameters_modified_between_forward_and_backward():
    """The hand-written backward reads the weights again (dgrad stream; the gradients around xyz_encoding_final are
    composed from the fp32 weights): like autograd's saved-tensor version check it refuses weights that changed."""
    import gpu_util
    from nerf_fl_amd import NeRF, PosEmbedding, render_rays
    dev = gpu_util.DEV
    models = {"coarse": NeRF("coarse").to(dev), "fine": NeRF("fine").to(dev)}
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    rays = orc.make_rays(8, 1).to(dev)
    ts = torch.zeros(8, dtype=torch.long, device=dev)
    res = render_rays(models, emb, rays, ts, 8, False, 0, 0, 8)
    loss = res["rgb_fine"].sum() + res["rgb_coarse"].sum()
    with torch.no_grad():
        models["fine"].xyz_encoding_final.weight.mul_(1.5)
    with pytest.raises(RuntimeError, match="modified in place"):
        loss.backward()
    res = render_rays(models, emb, rays, ts, 8, False, 0, 0, 8)         # an untouched pair of passes still works
    (res["rgb_fine"].sum() + res["rgb_coarse"].sum()).backward()
    assert models["fine"].xyz_encoding_final.weight.grad is not None
