"""Why tests/test_edge_cases_gpu.py::test_small_backward compares gradients at injected fine depths: on the oracle alone, a
change of the coarse weights far inside the forward's 1e-4 parity bar moves a fine depth, and with a handful of rays one
moved depth changes the fine field's gradients by more than the gradient tolerance."""
import torch

from oracle import nerfw_oracle as orc
from test_edge_cases_gpu import small_case

GTOL = 1e-2      # tests/test_grad_variants_gpu.py


def test_small_shape_gradients_move_with_1e7_of_the_coarse_weights():
    R, S, I = 3, 33, 31
    spec_c, _, spec_f, _, rays, target, a_emb, t_emb, noise_coarse = small_case(R, S, I)

    def fine_grads(z_fine=None):
        _, P_c, _, P_f, *_ = small_case(R, S, I)
        for p in P_f.values():
            p.requires_grad_(True)
        res = orc.render_rays(spec_c, P_c, spec_f, P_f, rays, n_samples=S, n_importance=I, noise_std=1.0, white_back=True,
                              a_emb=a_emb, t_emb=t_emb, noise_coarse=noise_coarse, return_z=True, z_fine=z_fine)
        z = res.pop("_z_fine")
        sum(orc.nerfw_loss(res, target).values()).backward()
        return z.detach(), res["weights_coarse"].detach(), {k: p.grad for k, p in P_f.items()}

    z0, w, g0 = fine_grads()
    # the oracle's own sampler (perturb = 0: u = linspace(0, 1, I), which ends at u = 1) on weights 1e-7 larger
    zc = orc.coarse_depths(rays[:, 6:7], rays[:, 7:8], S, False, 0.0, None)
    zs = orc.sample_pdf(0.5 * (zc[:, :-1] + zc[:, 1:]), w[:, 1:-1] + 1e-7, torch.linspace(0, 1, I).expand(R, I))
    z1 = torch.sort(torch.cat([zc, zs], 1), 1)[0]
    _, _, g1 = fine_grads(z1)
    moved = int(((z1 - z0).abs() > 1e-5).sum())
    change = max(((g1[k] - g0[k]).abs().max() / g0[k].abs().max()).item() for k in g0)
    print(f"{moved} of {z0.numel()} fine depths moved (max {(z1 - z0).abs().max().item():.2e}); "
          f"largest gradient change / max|g| = {change:.2e}")
    assert 1 <= moved <= 3
    assert change > GTOL
