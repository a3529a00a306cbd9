"""nerf_fl_amd.metrics / eval.evaluate_bank / RayTrainer.validate_bank on the device: nfl_image_metrics and
nfl_depth_image against the restatements of tests/metrics_util.py (fp64 truth; the tolerance of the SSIM map is measured
at run time from the reference's own fp32 arithmetic), and the bank evaluation against the routes the package had
before (bank.frame + batched_inference + a torch expression, fit_and_evaluate_halves)."""
import math

import numpy as np
import pytest
import torch

import data_util as du
import metrics_util as mu

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
PSNR_TOL = 1e-4       # dB: fp32 colours, differences and sums in fp64 (relative error of the sums far below 1e-5 = 4e-5 dB)
COLS = {k: j for j, k in enumerate(("sse", "count", "sse_valid", "count_valid", "ssim_sum", "psnr", "psnr_valid", "ssim"))}


def _banks():
    from nerf_fl_amd import data
    kinds = dict(big=lambda dev: data.ImageBank.from_blender(du.SCENE, "train", (800, 800), (), device=dev),
                 small=lambda dev: data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), ("color",), device=dev),
                 photo=lambda dev: data.ImageBank(**du.photo_inputs()[1], device=dev))
    return kinds


_cache = {}


def _bank(kind):
    if kind not in _cache:
        make = _banks()[kind]
        _cache[kind] = (make(DEV), make(None))
    return _cache[kind]


def _close_db(a, b, tol=PSNR_TOL):
    return (math.isinf(a) and math.isinf(b) and a == b) or abs(a - b) <= tol


def _check(row, smap, ref32, ref64, tag):
    """row: the 8 columns (host), smap: the kernel's map (host, fp32)."""
    for k in ("count", "count_valid"):
        assert row[COLS[k]] == ref64[k], (tag, k, row[COLS[k]], ref64[k])
    for k in ("sse", "sse_valid"):
        assert abs(row[COLS[k]] - ref64[k]) <= 1e-9 * ref64[k], (tag, k, row[COLS[k]], ref64[k])
    d_ref = (ref32["map"].double() - ref64["map"]).abs().max().item()
    d_kernel = (smap.double() - ref64["map"]).abs().max().item()
    m_ref, m_kernel = abs(ref32["ssim"] - ref64["ssim"]), abs(row[COLS["ssim"]] - ref64["ssim"])
    print(f"{tag}: psnr {row[COLS['psnr']]:.6f} (truth {ref64['psnr']:.6f}) valid {row[COLS['psnr_valid']]:.6f} "
          f"({ref64['psnr_valid']:.6f}); ssim {row[COLS['ssim']]:.8f} (truth {ref64['ssim']:.8f}); map d_ref {d_ref:.3e} "
          f"kernel {d_kernel:.3e}; mean fp32 {m_ref:.2e} kernel {m_kernel:.2e}")
    assert _close_db(row[COLS["psnr"]], ref64["psnr"]), tag
    if ref64["count_valid"]:
        assert _close_db(row[COLS["psnr_valid"]], ref64["psnr_valid"]), tag
    else:
        assert math.isnan(row[COLS["psnr_valid"]])
    assert smap.shape == ref64["map"].shape
    assert d_kernel <= 4 * d_ref, (tag, d_kernel, d_ref)
    assert m_kernel <= 2 * m_ref + 1e-6, (tag, m_kernel, m_ref)
    assert abs(row[COLS["ssim_sum"]] / row[COLS["count"]] - row[COLS["ssim"]]) <= 1e-15
    return d_ref, d_kernel


# (bank, image, region): 800 x 800 RGBA whole / right half / a 701 x 333 window off the tile grid; 24 x 24 whole, 2 wide,
# 23 x 19; the unequal RGB photos whole (17 x 23, 30 x 12, 8 x 41: no multiple of a tile) and 2 high
CASES = [("big", 0, None), ("big", 1, (400, 800, 0, 800)), ("big", 2, (3, 704, 5, 338)),
         ("small", 1, None), ("small", 0, (11, 13, 0, 24)), ("small", 2, (1, 24, 2, 21)),
         ("photo", 0, None), ("photo", 1, None), ("photo", 2, None), ("photo", 1, (0, 12, 7, 9))]


@pytest.mark.parametrize("kind,image,region", CASES)
def test_bank_form_against_the_restatement(kind, image, region):
    from nerf_fl_amd import eval as ev, metrics
    bank, host = _bank(kind)
    target, valid = mu.host_image(host, image)
    H, W = target.shape[:2]
    assert torch.equal(bank.frame(image)[1].cpu().reshape(H, W, 3), target)       # the colours the old route scores
    for n, (name, sigma) in enumerate(mu.NOISE):
        for clip in ((True, False) if name == "wild" else (True,)):
            pred = mu.noisy(target, sigma, 100 * image + n)
            if name == "wild":
                assert (pred < 0).any() and (pred > 1).any()
            table, u8, smap = metrics.image_metrics(pred.reshape(-1, 3).to(DEV), H, W, bank=bank, image=image,
                                                    region=region, clip=clip, want_uint8=True, want_map=True)
            ref32, ref64 = (mu.reference(pred, target, valid, clip, region, d) for d in (torch.float32, torch.float64))
            _check(table[0].cpu().tolist(), smap.cpu(), ref32, ref64, f"{kind}[{image}] {region} {name} clip={clip}")
            exp_u8 = ev.to_uint8(pred.to(DEV)).cpu()
            assert torch.equal(u8.cpu(), exp_u8 if region is None else mu.crop(exp_u8, region))
    if kind != "photo":
        assert 0 < valid.sum() < valid.numel()            # the masked PSNR is a different number on these images


def test_ground_truth_is_converted_as_the_gather_converts_it():
    from nerf_fl_amd import metrics
    for kind, image in (("big", 1), ("small", 2), ("photo", 2)):
        bank, host = _bank(kind)
        rgb = bank.frame(image)[1]
        rec = host.host_table[image]
        H, W = int(rec["height"]), int(rec["width"])
        table = metrics.image_metrics(torch.zeros(H * W, 3, device=DEV), H, W, bank=bank, image=image, clip=False)
        exp = (rgb.double() ** 2).sum().item()
        got = table[0, 0].item()
        print(kind, image, "sse", got, "sum of squares of the frame", exp, "rel", abs(got - exp) / exp)
        assert abs(got - exp) <= 1e-12 * exp
        assert table[0, 1].item() == 3 * H * W


def test_real_render_of_the_small_scene():
    from nerf_fl_amd import eval as ev, metrics
    bank, host = _bank("small")
    models, emb = _fields(False)
    rays, rgbs, ts = bank.frame(1)
    res = ev.batched_inference(models, emb, rays, ts, 32, 32, white_back=True)
    pred = res["rgb_fine"].contiguous()
    target, valid = mu.host_image(host, 1)
    table, smap = metrics.image_metrics(pred, 24, 24, bank=bank, image=1, want_map=True)
    p = pred.cpu().reshape(24, 24, 3)
    ref32, ref64 = (mu.reference(p, target, valid, True, None, d) for d in (torch.float32, torch.float64))
    _check(table[0].cpu().tolist(), smap.cpu(), ref32, ref64, "render of small[1]")


def test_tensor_form_mask_and_reference_style_wrappers():
    from nerf_fl_amd import metrics
    bank, host = _bank("photo")
    target, _ = mu.host_image(host, 1)
    H, W = target.shape[:2]
    pred = mu.noisy(target, 0.1, 7)
    valid = torch.rand(H, W, generator=torch.Generator().manual_seed(2)) < 0.6
    p, t = pred.reshape(-1, 3).to(DEV), target.reshape(-1, 3).to(DEV)
    table, smap = metrics.image_metrics(p, H, W, target=t, mask=valid.reshape(-1).to(DEV), clip=False, want_map=True)
    ref32, ref64 = (mu.reference(pred, target, valid, False, None, d) for d in (torch.float32, torch.float64))
    _check(table[0].cpu().tolist(), smap.cpu(), ref32, ref64, "tensor form")
    # metrics.psnr(pred, target[, valid_mask]) and metrics.ssim in both layouts
    got = metrics.psnr(p, t)
    assert got.dim() == 0 and got.is_cuda and _close_db(got.item(), ref64["psnr"])
    assert _close_db(metrics.psnr(p, t, valid.reshape(-1).to(DEV)).item(), ref64["psnr_valid"])
    odd = ((pred.reshape(-1, 3)[:-1].double() - target.reshape(-1, 3)[:-1].double()) ** 2).mean().item()
    assert _close_db(metrics.psnr(p[:-1], t[:-1]).item(), -10 * math.log10(odd))           # an odd number of pixels
    tol = 2 * abs(ref32["ssim"] - ref64["ssim"]) + 1e-6
    nchw = lambda x: x.reshape(H, W, 3).permute(2, 0, 1)[None].to(DEV)
    for s in (metrics.ssim(nchw(pred), nchw(target)), metrics.ssim(p, t, H, W)):
        assert s.dim() == 0 and s.is_cuda and abs(s.item() - ref64["ssim"]) <= tol
    assert metrics.psnr(t, t).item() == math.inf and metrics.ssim(t, t, H, W).item() == 1.0


def test_table_slots_and_errors():
    from nerf_fl_amd import metrics
    bank, host = _bank("small")
    pred = torch.rand(576, 3, device=DEV)
    table = torch.zeros(3, 8, dtype=torch.float64, device=DEV)
    out = metrics.image_metrics(pred, 24, 24, bank=bank, image=0, table=table, slot=2)
    assert out is table and (table[:2] == 0).all() and table[2, 1].item() == 1728
    metrics.image_metrics(pred, 24, 24, bank=bank, image=0, table=table, slot=1, region=(5, 5, 0, 24))     # empty: untouched
    assert (table[:2] == 0).all()
    for kw in (dict(bank=bank, image=3), dict(bank=bank, image=0, region=(0, 1, 0, 24)), dict(),
               dict(bank=bank, image=0, target=pred), dict(bank=bank, image=0, table=table, slot=3)):
        with pytest.raises(ValueError):
            metrics.image_metrics(pred, 24, 24, **kw)
    with pytest.raises(ValueError):
        metrics.image_metrics(pred[:100], 24, 24, bank=bank, image=0)
    with pytest.raises(ValueError):
        metrics.image_metrics(torch.rand(17 * 23, 3, device=DEV), 17, 23, bank=bank, image=0)     # not the image's size


def test_depth_image():
    from nerf_fl_amd import metrics
    rng = np.random.default_rng(3)
    H, W = 37, 150
    depth = rng.uniform(2.0, 6.0, (H, W)).astype(np.float32)
    depth[rng.random((H, W)) < 0.05] = np.nan
    lut = rng.integers(0, 256, (256, 3), dtype=np.uint8)
    d = torch.from_numpy(depth).to(DEV)
    for region in (None, (10, 141, 3, 30), (0, 1, 0, 1)):
        for table in (None, lut):
            got = metrics.depth_image(d.reshape(-1), H, W, region=region, lut=None if table is None else
                                      torch.from_numpy(table).to(DEV))
            assert torch.equal(got.cpu(), torch.from_numpy(mu.depth_reference(depth, region, table))), (region, table is None)
    clean = np.nan_to_num(depth, nan=3.0)                      # no NaN: the minimum is not 0
    assert torch.equal(metrics.depth_image(torch.from_numpy(clean).to(DEV).reshape(-1), H, W).cpu(),
                       torch.from_numpy(mu.depth_reference(clean)))
    const = np.full((H, W), 4.25, np.float32)                  # ma == mi
    got = metrics.depth_image(torch.from_numpy(const).to(DEV).reshape(-1), H, W)
    assert torch.equal(got.cpu(), torch.from_numpy(mu.depth_reference(const))) and (got == 0).all()
    big = rng.uniform(0.0, 9.0, (800, 800)).astype(np.float32)   # more pixels than the first pass has workgroups
    assert torch.equal(metrics.depth_image(torch.from_numpy(big).to(DEV).reshape(-1), 800, 800).cpu(),
                       torch.from_numpy(mu.depth_reference(big)))
    assert metrics.depth_image(d.reshape(-1), H, W, region=(4, 4, 0, H)).shape == (H, 0, 3)


def test_two_calls_are_bit_identical_and_a_graph_replay_equals_the_eager_call():
    from nerf_fl_amd import metrics
    bank, host = _bank("big")
    target, _ = mu.host_image(host, 0)
    pred = mu.noisy(target, 0.1, 5).reshape(-1, 3).to(DEV)
    a = metrics.image_metrics(pred, 800, 800, bank=bank, image=0, want_map=True)
    b = metrics.image_metrics(pred, 800, 800, bank=bank, image=0, want_map=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    static = pred.clone()
    table = torch.zeros(2, 8, dtype=torch.float64, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        metrics.image_metrics(static, 800, 800, bank=bank, image=0, table=table, slot=1)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                              # a linear chain of two kernel launches
        metrics.image_metrics(static, 800, 800, bank=bank, image=0, table=table, slot=1)
    table.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(table[1], a[0][0]) and (table[0] == 0).all()
    other = mu.noisy(target, 0.3, 6).reshape(-1, 3).to(DEV)
    static.copy_(other)
    graph.replay()
    assert torch.equal(table[1], metrics.image_metrics(other, 800, 800, bank=bank, image=0)[0])


# ---- evaluate_bank -----------------------------------------------------------------------------------------------------
def _fields(encode_a, n_a=48, n_vocab=8):
    from nerf_fl_amd import NeRF, PosEmbedding, synth

    def module(typ, seed, **kw):
        m = NeRF(typ, in_channels_xyz=63, in_channels_dir=27, encode_appearance=kw.get("encode_appearance", False),
                 in_channels_a=n_a)
        m.load_state_dict(synth.make_field_params(seed, "sharp", typ=typ, **kw), strict=True)
        return m.to(DEV)

    models = {"coarse": module("coarse", 21), "fine": module("fine", 22, encode_appearance=encode_a, n_a=n_a)}
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    if encode_a:
        g = torch.Generator().manual_seed(23)
        emb["a"] = torch.nn.Embedding.from_pretrained(torch.randn(n_vocab, n_a, generator=g), freeze=True).to(DEV)
    return models, emb


def _old_route_psnr(models, emb, bank, i, S, I):
    from nerf_fl_amd import eval as ev
    rays, rgbs, ts = bank.frame(i)
    pred = ev.batched_inference(models, emb, rays, ts, S, I, white_back=bank.white_back)["rgb_fine"]
    return -10.0 * math.log10(((pred.clamp(0, 1).double() - rgbs.double()) ** 2).mean().item())


@pytest.mark.parametrize("encode_a", [False, True])
def test_evaluate_bank_equals_the_old_route_and_shards_add_up(encode_a):
    from nerf_fl_amd import eval as ev
    bank, host = _bank("small")
    models, emb = _fields(encode_a)
    S = I = 32
    full = ev.evaluate_bank(models, emb, bank, S, I, return_images=True, return_depth=True)
    assert full["table"].shape == (3, 8) and full["table"].dtype == torch.float64 and len(full["frames"]) == 3
    for i in range(3):
        old = _old_route_psnr(models, emb, bank, i, S, I)
        print(f"NeRF{'-A' if encode_a else ''} image {i}: evaluate_bank {full['psnr'][i].item():.6f} dB, old route {old:.6f} dB, "
              f"ssim {full['ssim'][i].item():.6f}, valid psnr {full['psnr_valid'][i].item():.6f}")
        assert abs(full["psnr"][i].item() - old) <= PSNR_TOL
        assert full["frames"][i].shape == (24, 24, 3) and full["depths"][i].shape == (24, 24, 3)
    assert abs(full["mean_psnr"] - full["psnr"].mean().item()) <= 1e-12
    assert abs(full["mean_ssim"] - full["ssim"].mean().item()) <= 1e-12
    # ranks without a process group: disjoint rows that add up bit for bit
    parts = [ev.evaluate_bank(models, emb, bank, S, I, rank=r, world=2)["table"] for r in (0, 1)]
    assert ((parts[0] != 0).any(1) & (parts[1] != 0).any(1)).sum() == 0
    assert (parts[0] != 0).any(1).tolist() == [True, True, False]
    assert torch.equal(parts[0] + parts[1], full["table"])
    # a subset, ids overridden (the reference's t = 0 for val / test images), right halves
    sub = ev.evaluate_bank(models, emb, bank, S, I, images=[2, 0], ts=0, halves=True)
    assert sub["table"].shape == (2, 8) and sub["table"][0, 1].item() == 3 * 24 * 12
    if not encode_a:                                            # no latent input: the id does not matter
        rays, rgbs, ts = bank.frame(2)
        pred = ev.batched_inference(models, emb, rays, ts, S, I, white_back=True)["rgb_fine"].reshape(24, 24, 3)
        mse = ((pred[:, 12:].clamp(0, 1).double() - rgbs.reshape(24, 24, 3)[:, 12:].double()) ** 2).mean().item()
        assert abs(sub["psnr"][0].item() + 10.0 * math.log10(mse)) <= PSNR_TOL


def test_halves_with_a_fit_equals_fit_and_evaluate_halves():
    from nerf_fl_amd import eval as ev
    bank, host = _bank("small")
    models, emb = _fields(True)
    S = I = 32
    init = emb["a"].weight[3].detach().clone()
    out = ev.evaluate_bank(models, emb, bank, S, I, images=[1], halves=True, clip=False,
                           fit=dict(n_iters=30, lr=0.1, init=init))
    rec = host.host_table[1]
    K = torch.tensor([[float(rec["fx"]), 0, float(rec["cx"])], [0, float(rec["fy"]), float(rec["cy"])], [0, 0, 1.0]])
    code, psnr = ev.fit_and_evaluate_halves(models, emb, torch.from_numpy(rec["c2w"].reshape(3, 4).copy()), K, 24, 24,
                                            float(rec["near"]), float(rec["far"]), bank.frame(1)[1], S, I, n_iters=30, lr=0.1,
                                            init=init, white_back=True, device=DEV)
    err, scale = (out["codes"][0] - code).abs().max().item(), code.abs().max().item()
    moved = (code - init).abs().max().item()
    print(f"fit: max |code difference| {err:.3e} (scale {scale:.3f}, moved {moved:.3e}); right-half PSNR "
          f"{out['psnr'][0].item():.6f} vs {psnr:.6f} dB")
    assert moved > 0
    assert err <= 1e-3 * scale                 # tests/test_appearance_gpu.py's bound between its two routes
    assert abs(out["psnr"][0].item() - psnr) <= PSNR_TOL


def test_peak_memory_does_not_grow_with_the_number_of_images():
    from nerf_fl_amd import data, eval as ev
    rng = np.random.default_rng(5)

    def bank_of(n_img):
        imgs = [rng.integers(0, 256, (32, 32, 4), dtype=np.uint8) for _ in range(n_img)]
        c2w = np.tile(np.eye(4)[None, :3], (n_img, 1, 1))
        c2w[:, :, 3] = np.array([0.0, 0.0, 4.0]) + 0.1 * rng.standard_normal((n_img, 3))
        K = np.array([[40.0, 0, 16], [0, 40.0, 16], [0, 0, 1]])
        return data.ImageBank(imgs, c2w, K, 2.0, 6.0, device=DEV)

    models, emb = _fields(False)
    small, large = bank_of(4), bank_of(16)
    ev.evaluate_bank(models, emb, small, 32, 32)           # weight streams, kernel attributes: once
    peaks = []
    for b in (small, large):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = ev.evaluate_bank(models, emb, b, 32, 32)
        torch.cuda.synchronize()
        peaks.append(torch.cuda.max_memory_allocated() - base)
        del res
    print("peak above the resident state for 4 and 16 images:", peaks)
    assert 0 <= peaks[1] - peaks[0] <= 1024                # 12 more rows of 64 B = 768 B, in the allocator's 512 B blocks


def test_validate_bank():
    from nerf_fl_amd import eval as ev
    from nerf_fl_amd.train import RayTrainer
    bank, host = _bank("small")
    tr = RayTrainer(DEV, N_samples=32, N_importance=32, batch_size=256, lr=1e-3, seed=3)
    psnr, ssim = tr.validate_bank(bank)
    res = ev.evaluate_bank(tr.models, tr.embeddings, bank, 32, 32, clip=False, chunk=32768)
    assert psnr == res["mean_psnr"] and ssim == res["mean_ssim"] and np.isfinite(psnr) and 0 < ssim <= 1
    per_image = [tr.validate(*bank.frame(i)) for i in range(3)]
    print("validate_bank", psnr, ssim, "validate per image", per_image)
    assert abs(psnr - float(np.mean(per_image))) <= PSNR_TOL
    assert tr.validate_bank(bank, images=[1])[0] == res["psnr"][1].item()
    # refine_pose with untouched poses: the learned pose of every id is its initial pose, which is the bank's, so the
    # render through the learned poses is the render validate() gives for the training (camera) layout.  The two routes
    # build the same rays with different arithmetic (nfl_pose_rays against the render prologue): directions agree to
    # data_util.RAY_TOL = 2e-7, positions along a ray of length <= 6 to about 1e-6, and the untrained field's colours
    # change by the same order (its first layers have gains of order 1): a relative change of the squared error of about
    # 1e-5, well inside 1e-3 dB.
    init = torch.from_numpy(host.host_table["c2w"].reshape(-1, 3, 4).copy())
    rp = RayTrainer(DEV, N_samples=32, N_importance=32, batch_size=256, lr=1e-3, seed=3, refine_pose=True, init_c2w=init,
                    image_ids=host.host_table["id"].tolist())
    got = rp.validate_bank(bank)[0]
    exp = float(np.mean([rp.validate(*bank.frame(i, "camera")) for i in range(3)]))
    print("refine_pose: validate_bank", got, "validate on the camera layout", exp)
    assert abs(got - exp) <= 1e-3
