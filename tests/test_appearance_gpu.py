"""AppearanceFit (nerf_fl_amd.appearance): NeRF-W appearance codes fitted to images the fields were not trained on, on the
cache-building render pass + the fused fit iteration (C ABI nfl_appearance_cache / nfl_appearance_fit)."""
import ctypes as C
import os

import pytest
import torch

import golden_util as gu
import gpu_util
import nerf_fl_amd
from nerf_fl_amd import render_rays
from nerf_fl_amd.appearance import AppearanceFit
from nerf_fl_amd.eval import batched_inference, fit_and_evaluate_halves
from nerf_fl_amd.train import Adam
from oracle import nerfw_oracle as orc

pytestmark = pytest.mark.gpu
DEV = gpu_util.DEV


def _setup(name, regime=None):
    cfg, a = gu.load(name)
    if regime is not None:
        cfg = dict(cfg, regime=regime)
    specs, kw = gu.oracle_kwargs(cfg, a)
    spec_c, P_c, spec_f, P_f = specs
    barf = kw.get("pe_w_xyz") is not None
    models = {"coarse": gpu_util.module_from(spec_c, P_c, barf), "fine": gpu_util.module_from(spec_f, P_f, barf)}
    emb = gpu_util.make_embeddings(spec_c.n_emb_xyz, barf, spec_c.n_emb_dir)
    extra = {"current_epoch": kw["barf_epoch"]} if barf else {}
    return cfg, a, specs, kw, models, emb, extra


def _ragged_images(R, sizes, seed):
    """image_index (R,) with len(sizes) images of the given ray counts, shuffled"""
    assert sum(sizes) == R
    idx = torch.cat([torch.full((n,), i, dtype=torch.int64) for i, n in enumerate(sizes)])
    return idx[torch.randperm(R, generator=torch.Generator().manual_seed(seed))]


def _oracle(specs, rays, kw, a_emb, z_fine, white_back, test_time=True, dtype=torch.float32):
    spec_c, P_c, spec_f, P_f = specs
    cast = lambda P: {k: v.to(dtype) for k, v in P.items()}
    R = rays.shape[0]
    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        return orc.render_rays(spec_c, cast(P_c), spec_f, cast(P_f), rays.to(dtype), n_samples=kw["n_samples"],
                               use_disp=kw["use_disp"], perturb=0.0, noise_std=0.0, n_importance=kw["n_importance"],
                               white_back=white_back, test_time=test_time, a_emb=a_emb,
                               t_emb=torch.zeros(R, spec_f.n_tau, dtype=dtype), output_transient=False,
                               z_fine=z_fine.to(dtype),
                               pe_w_xyz=None if kw.get("pe_w_xyz") is None else kw["pe_w_xyz"].to(dtype),
                               pe_w_dir=None if kw.get("pe_w_dir") is None else kw["pe_w_dir"].to(dtype))
    finally:
        torch.set_default_dtype(old)


# ---- 1. forward ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,white_back", [("g7_test_nerfw_noT", False), ("g7_test_nerfw_noT", True),
                                             ("g18_na40_tau5_emb", False)])
def test_render_matches_the_reference(name, white_back):
    """image_index = the fixture's ts renumbered, codes = those rows of its table, its fine depths injected: the stored
    reference rgb_fine (g7, the fixture's own white_back) or the oracle's (other settings) within 1e-4 on every ray"""
    cfg, a, specs, kw, models, emb, extra = _setup(name)
    uniq, idx = torch.unique(a["ts"], return_inverse=True)
    table = gu.embedding_table(cfg, "a")
    R = a["rays"].shape[0]
    fit = AppearanceFit(models, emb, a["rays"].to(DEV), torch.zeros(R, 3, device=DEV), idx.to(DEV), cfg["S"], cfg["I"],
                        use_disp=cfg["use_disp"], white_back=white_back, init=table[uniq].to(DEV),
                        z_fine=a["z_fine"].to(DEV), **extra)
    got = fit.render().cpu()
    if name == "g7_test_nerfw_noT" and white_back == cfg["white_back"]:
        exp = a["out.rgb_fine"]
    else:
        with torch.no_grad():
            exp = _oracle(specs, a["rays"], kw, table[a["ts"]], a["z_fine"], white_back)["rgb_fine"]
    err = (got - exp).abs().max().item()
    print(f"{name} white_back={white_back}: max |rgb - reference| = {err:.3e}")
    assert err <= 1e-4
    assert torch.equal(fit.z_fine.cpu(), a["z_fine"])


def test_render_matches_render_rays_on_photo_rays():
    """g15_photo_test weights: per-ray near/far, use_disp, 128+128 samples, N_vocab 1500; the fit's own coarse pass and
    sampler: within 1e-5 of render_rays(test_time=True, output_transient=False, a_embedded=...)"""
    cfg, a, specs, kw, models, emb, extra = _setup("g15_photo_test")
    uniq, idx = torch.unique(a["ts"], return_inverse=True)
    table = gu.embedding_table(cfg, "a")
    rays = a["rays"].to(DEV)
    R = rays.shape[0]
    fit = AppearanceFit(models, emb, rays, torch.zeros(R, 3, device=DEV), idx.to(DEV), cfg["S"], cfg["I"],
                        use_disp=cfg["use_disp"], init=table[uniq].to(DEV))
    got = fit.render()
    with torch.no_grad():
        exp = render_rays(models, emb, rays, None, cfg["S"], cfg["use_disp"], 0, 0, cfg["I"], 32768, False, True,
                          output_transient=False, a_embedded=table[a["ts"]].to(DEV))
    err = (got - exp["rgb_fine"]).abs().max().item()
    print(f"g15_photo_test: max |rgb - render_rays| = {err:.3e}")
    assert err <= 1e-5


@pytest.mark.parametrize("inject", [False, True])
def test_cache_is_the_same_whatever_the_chunk(inject):
    """150 rays of 3 images with a per-ray view_dir: built in chunks of 64 + 64 + 22 rays, the cache, the weights, the
    opacity and the fine depths are bit-identical to the ones built in one pass; with injected fine depths as well."""
    cfg, a, specs, kw, models, emb, extra = _setup("g17_trained_cfg3", "trained")
    R, S, I = 150, 32, 32
    rays = orc.make_rays(R, 23).to(DEV)
    gen = torch.Generator().manual_seed(29)
    more = dict(view_dir=torch.nn.functional.normalize(torch.randn(R, 3, generator=gen), dim=1).to(DEV))
    if inject:
        more["z_fine"] = torch.sort(2.0 + 4.0 * torch.rand(R, S + I, generator=gen), dim=1)[0].to(DEV)
    idx = _ragged_images(R, [70, 13, 67], 4).to(DEV)
    rgb = torch.zeros(R, 3, device=DEV)
    init = gu.embedding_table(cfg, "a")[[2, 3, 9]].to(DEV)
    fits = [AppearanceFit(models, emb, rays, rgb, idx, S, I, white_back=True, init=init, chunk=chunk, **more)
            for chunk in (64, 1024)]
    for name in ("zcache", "weights", "opacity", "z_fine"):
        assert torch.equal(getattr(fits[0], name), getattr(fits[1], name)), name
    assert fits[0].zcache.shape[0] == R and float(fits[0].weights.abs().sum()) > 0
    if inject:
        assert torch.equal(fits[0].z_fine, more["z_fine"])


# ---- 2. gradient ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,regime", [("g17_trained_cfg3", "trained"), ("g14_barf_e9", None)])
def test_gradient_matches_fp64_autograd(name, regime):
    cfg, a, specs, kw, models, emb, extra = _setup(name, regime)
    rays = a["rays"]
    R = rays.shape[0]
    sizes = [R // 8, R // 2 - 3, R - R // 8 - (R // 2 - 3)]
    idx = _ragged_images(R, sizes, 5)
    table = gu.embedding_table(cfg, "a")
    init = table[[3, 7, 11]].clone()
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(9))
    fit = AppearanceFit(models, emb, rays.to(DEV), target.to(DEV), idx.to(DEV), cfg["S"], cfg["I"],
                        white_back=cfg["white_back"], init=init.to(DEV), lr=0.0, **extra)
    loss = fit.step()
    g_hip = fit.codes.grad.cpu()
    codes = init.double().requires_grad_()
    out = _oracle(specs, rays, kw, codes[idx], fit.z_fine.cpu(), cfg["white_back"], test_time=False, dtype=torch.float64)
    ref_loss = ((out["rgb_fine"] - target.double()) ** 2).mean()
    ref_loss.backward()
    g_ref = codes.grad
    print(f"{name}: loss {loss.item():.6e} vs {ref_loss.item():.6e}")
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * ref_loss.item() + 1e-7
    for i in range(3):
        gmax = g_ref[i].abs().max().item()
        err = (g_hip[i].double() - g_ref[i]).abs().max().item()
        print(f"  image {i} ({sizes[i]} rays): max|g| {gmax:.3e}, max|dg| {err:.3e} ({err / gmax:.2e})")
        assert gmax > 0 and err <= 2e-4 * gmax


@pytest.mark.parametrize("R,I", [(4500, 64), (6000, 96)])
def test_many_rays_per_wavefront_match_render_rays_and_autograd(R, I):
    """More than 2048 rays: every work item of the fit kernel carries its accumulators and squared error across several
    rays.  Synthetic rays through the trained fields, five images of ragged sizes (one without rays), shuffled;
    64 + 96 samples pads to 192 (three 64-sample chunks per ray).  render() against render_rays, the loss and the code
    gradient against render_rays + autograd with the fp32-class backward."""
    cfg, a, specs, kw, models, emb, extra = _setup("g17_trained_cfg3", "trained")
    for p in list(models["coarse"].parameters()) + list(models["fine"].parameters()):
        p.requires_grad_(False)
    S = 64
    rays = orc.make_rays(R, 31).to(DEV)
    sizes = [R // 10, 0, R // 3 + 7, R // 4 - 5]
    sizes.append(R - sum(sizes))
    idx = _ragged_images(R, sizes, 13).to(DEV)
    table = gu.embedding_table(cfg, "a")
    init = table[[2, 4, 6, 8, 10]].to(DEV)
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(17)).to(DEV)
    fit = AppearanceFit(models, emb, rays, target, idx, S, I, white_back=True, init=init, lr=0.0)
    assert fit.n_items < R // 2                          # several rays per wavefront
    got = fit.render()
    loss = fit.step()
    g_fit = fit.codes.grad.clone()
    with torch.no_grad():
        exp = render_rays(models, emb, rays, None, S, False, 0, 0, I, 32768, True, True, output_transient=False,
                          a_embedded=init[idx], z_fine=fit.z_fine)["rgb_fine"]
    err = (got - exp).abs().max().item()
    nerf_fl_amd.set_precision("f16x3", backward="f16x3")
    try:
        codes = init.clone().requires_grad_()
        res = render_rays(models, emb, rays, None, S, False, 0, 0, I, 32768, True, False, output_transient=False,
                          a_embedded=codes[idx], z_fine=fit.z_fine)
        ref_loss = ((res["rgb_fine"] - target) ** 2).mean()
        ref_loss.backward()
    finally:
        nerf_fl_amd.set_precision("f16x3", backward="f16")
    print(f"R={R}, {S}+{I} samples, {fit.n_items} work items: max |rgb - render_rays| {err:.3e}, "
          f"loss {loss.item():.6e} vs {ref_loss.item():.6e}")
    assert err <= 1e-5
    assert abs(loss.item() - ref_loss.item()) <= 1e-5 * ref_loss.item()
    assert torch.equal(g_fit[1], torch.zeros_like(g_fit[1]))          # the image without rays
    for i in (0, 2, 3, 4):
        gmax = codes.grad[i].abs().max().item()
        gerr = (g_fit[i] - codes.grad[i]).abs().max().item()
        print(f"  image {i} ({sizes[i]} rays): max|g| {gmax:.3e}, max|dg| {gerr:.3e} ({gerr / gmax:.2e})")
        assert gmax > 0 and gerr <= 2e-4 * gmax


# ---- 3. trajectory --------------------------------------------------------------------------------------------------
def test_same_trajectory_as_render_rays_autograd_and_adam():
    cfg, a, specs, kw, models, emb, extra = _setup("g17_trained_cfg3", "trained")
    for p in list(models["coarse"].parameters()) + list(models["fine"].parameters()):
        p.requires_grad_(False)
    rays = a["rays"].to(DEV)
    R = rays.shape[0]
    idx = _ragged_images(R, [10, 30, 24], 3).to(DEV)
    table = gu.embedding_table(cfg, "a")
    init = table[[1, 4, 6]].to(DEV)
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(4)).to(DEV)
    lr = 0.02
    fit = AppearanceFit(models, emb, rays, target, idx, cfg["S"], cfg["I"], white_back=True, init=init, lr=lr)
    fast = fit.fit(20).clone()
    nerf_fl_amd.set_precision("f16x3", backward="f16x3")
    try:
        codes = torch.nn.Parameter(init.clone())
        opt = Adam([codes], lr=lr)
        for _ in range(20):
            opt.zero_grad()
            res = render_rays(models, emb, rays, None, cfg["S"], False, 0, 0, cfg["I"], 32768, True, False,
                              output_transient=False, a_embedded=codes[idx], z_fine=fit.z_fine)
            ((res["rgb_fine"] - target) ** 2).mean().backward()
            opt.step()
    finally:
        nerf_fl_amd.set_precision("f16x3", backward="f16")
    err = (fast - codes.detach()).abs().max().item()
    scale = codes.detach().abs().max().item()
    moved = (codes.detach() - init).abs().max().item()
    print(f"20 iterations: max |codes fast - slow| = {err:.3e} (max |code| {scale:.3f}, moved {moved:.3e})")
    assert moved > 10 * err
    assert err <= 1e-3 * scale


# ---- 4. convergence -------------------------------------------------------------------------------------------------
def _look_at(c):
    f = -c / c.norm()
    up = torch.tensor([0.0, 1.0, 0.0])
    r = torch.linalg.cross(up, -f)
    r = r / r.norm()
    u = torch.linalg.cross(-f, r)
    m = torch.eye(4)
    m[:3, 0], m[:3, 1], m[:3, 2], m[:3, 3] = r, u, -f, c
    return m


def test_fit_recovers_the_appearance_of_a_held_out_image():
    cfg, a, specs, kw, models, emb, extra = _setup("g17_trained_cfg3", "trained")
    table = gu.embedding_table(cfg, "a").to(DEV)
    emb["a"] = torch.nn.Embedding.from_pretrained(table.clone(), freeze=True)
    H = W = 24
    K = torch.tensor([[W / 0.7, 0, W / 2], [0, W / 0.7, H / 2], [0, 0, 1]])
    c2w = _look_at(torch.tensor([0.4, 0.3, 3.9]))
    S = I = 64
    from nerf_fl_amd.eval import frame_rays
    rays = frame_rays(c2w, K, H, W, 2.0, 6.0, DEV)
    with torch.no_grad():
        target = batched_inference(models, emb, rays, None, S, I, white_back=True, output_transient=False,
                                   a_embedded=table[5][None])["rgb_fine"].clone()
    params = [p.detach().clone() for m in models.values() for p in m.parameters()]
    code0 = table[12].clone()
    _, psnr0 = fit_and_evaluate_halves(models, emb, c2w, K, H, W, 2.0, 6.0, target, S, I, n_iters=0, init=code0,
                                       white_back=True, device=DEV)
    # 300 iterations reach 35.2 dB on this scene; 1000 leave a margin of about 3 dB over the bar
    code, psnr = fit_and_evaluate_halves(models, emb, c2w, K, H, W, 2.0, 6.0, target, S, I, n_iters=1000, lr=0.25,
                                         init=code0, white_back=True, device=DEV, use_graph=True)
    print(f"right-half PSNR: {psnr0:.2f} dB at the start code, {psnr:.2f} dB after 1000 iterations; "
          f"|code - truth| {(code - table[5]).norm().item():.3f} (start {(code0 - table[5]).norm().item():.3f})")
    assert psnr >= 35.0 and psnr >= psnr0 + 5.0
    assert all(torch.equal(p, q) for p, q in zip(params, [p for m in models.values() for p in m.parameters()]))
    assert torch.equal(emb["a"].weight, table)


def test_halves_protocol_on_barf_fields():
    """refine_pose fields: current_epoch reaches both the fit and the right-half render"""
    cfg, a, specs, kw, models, emb, extra = _setup("g14_barf_e9")
    table = gu.embedding_table(cfg, "a").to(DEV)
    H = W = 16
    K = torch.tensor([[W / 0.7, 0, W / 2], [0, W / 0.7, H / 2], [0, 0, 1]])
    c2w = _look_at(torch.tensor([0.4, 0.3, 3.9]))
    from nerf_fl_amd.eval import frame_rays
    rays = frame_rays(c2w, K, H, W, 2.0, 6.0, DEV)
    with torch.no_grad():
        target = batched_inference(models, emb, rays, None, 64, 64, output_transient=False, a_embedded=table[5][None],
                                   **extra)["rgb_fine"].clone()
    _, psnr0 = fit_and_evaluate_halves(models, emb, c2w, K, H, W, 2.0, 6.0, target, 64, 64, n_iters=0, init=table[12],
                                       device=DEV, **extra)
    _, psnr = fit_and_evaluate_halves(models, emb, c2w, K, H, W, 2.0, 6.0, target, 64, 64, n_iters=100, lr=0.1,
                                      init=table[12], device=DEV, **extra)
    print(f"BARF fields, epoch {extra['current_epoch']}: right-half PSNR {psnr0:.2f} -> {psnr:.2f} dB")
    assert psnr > psnr0 + 1.0


# ---- 5. bit-exact and frozen ----------------------------------------------------------------------------------------
def _graph_nodes(graph_ptr):
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    hip.hipGraphGetNodes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    hip.hipGraphNodeGetType.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    n = C.c_size_t(0)
    assert hip.hipGraphGetNodes(C.c_void_p(graph_ptr), None, C.byref(n)) == 0
    nodes = (C.c_void_p * n.value)()
    assert hip.hipGraphGetNodes(C.c_void_p(graph_ptr), nodes, C.byref(n)) == 0
    types = []
    for node in nodes:
        ty = C.c_int(-1)
        assert hip.hipGraphNodeGetType(C.c_void_p(node), C.byref(ty)) == 0
        types.append(ty.value)
    return types


def test_bit_exact_graph_replay_frozen_fields_and_rayless_images():
    cfg, a, specs, kw, models, emb, extra = _setup("g17_trained_cfg3", "trained")
    table = gu.embedding_table(cfg, "a").to(DEV)
    emb["a"] = torch.nn.Embedding.from_pretrained(table.clone(), freeze=False)
    rays = a["rays"].to(DEV)
    R = rays.shape[0]
    idx = _ragged_images(R, [20, 0, 44], 8).to(DEV)       # image 1 has no rays
    idx = torch.where(idx == 2, torch.full_like(idx, 3), idx)   # and image 2 neither: ids 0 and 3
    init = table[[2, 3, 9, 13]].clone()
    target = torch.rand(R, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    params = {n: p.detach().clone() for k, m in models.items() for n, p in m.named_parameters(prefix=k)}

    def run(use_graph):
        fit = AppearanceFit(models, emb, rays, target, idx, cfg["S"], cfg["I"], white_back=True, init=init, lr=0.05)
        out = fit.fit(12, use_graph=use_graph).clone()
        return fit, out

    _, eager1 = run(False)
    _, eager2 = run(False)
    fit_g, graphed = run(True)
    assert torch.equal(eager1, eager2)
    assert torch.equal(eager1, graphed)
    assert not torch.equal(eager1[0], init[0]) and not torch.equal(eager1[3], init[3])
    assert torch.equal(eager1[1], init[1]) and torch.equal(eager1[2], init[2])      # images without rays: exact
    types = _graph_nodes(fit_g._graph.raw_cuda_graph())
    print(f"captured iteration: {len(types)} nodes, types {sorted(set(types))}")
    assert types and all(t == 0 for t in types)           # kernel nodes only: no memset / memcpy node
    for k, m in models.items():
        for n, p in m.named_parameters(prefix=k):
            assert p.grad is None and torch.equal(p.detach(), params[n]), n
    assert emb["a"].weight.grad is None and torch.equal(emb["a"].weight.detach(), table)


# ---- 6. errors ------------------------------------------------------------------------------------------------------
def test_errors():
    cfg, a, specs, kw, models, emb, extra = _setup("g17_trained_cfg3", "trained")
    rays = a["rays"].to(DEV)
    R = rays.shape[0]
    z = torch.zeros(R, dtype=torch.int64, device=DEV)
    rgb = torch.zeros(R, 3, device=DEV)
    init = torch.zeros(1, 48, device=DEV)
    spec_c, P_c, spec_f, P_f = specs
    base = orc.FieldSpec("fine", encode_appearance=False, encode_transient=False)
    base_models = {"coarse": models["coarse"], "fine": gpu_util.module_from(base, orc.make_field_params(base, 3, "sharp"))}
    with pytest.raises(ValueError):
        AppearanceFit(base_models, emb, rays, rgb, z, 64, 64, init=init)
    with pytest.raises(ValueError):
        AppearanceFit(models, emb, rays, rgb, z, 64, 0, init=init)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError):
        AppearanceFit(models, emb, rays, rgb, z, 64, 64, init=init, max_cache_bytes=R * 128 * 128 * 4 - 1)
    assert torch.cuda.memory_allocated(DEV) == before
    fit = AppearanceFit(models, emb, rays, rgb, z, 64, 64, init=init, max_cache_bytes=R * 128 * 128 * 4)
    assert fit.zcache.numel() * 4 == R * 128 * 128 * 4
