"""nfl_depth_bounds / data.depth_bounds / ImageBank.from_phototourism on the device, against the fixtures the REAL
reference's PhototourismDataset wrote (tests/golden/make_photo_golden.py) and against the reference's own statement of the
bounds in numpy (datasets/phototourism.py:127-131).

The bound on a depth bound, BOUND_REL * max|depth| of the scene: a depth is three fp64 products and three sums, so its
error is a few 2^-53 (1.1e-16) of its largest term, whatever the order of the sums (numpy's matmul may fuse or reorder
them); an order statistic of such depths carries the error of one depth, and the interpolation between two neighbouring
ones adds two more roundings of the same size.  1e-12 leaves four decimal digits above that."""
import dataclasses
import os

import numpy as np
import pytest
import torch

import data_util as du

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "data_photo")
DEV = "cuda:0"
BOUND_REL = 1e-12
pytestmark = pytest.mark.gpu


def _data():
    from nerf_fl_amd import data
    return data


def _golden():
    return du.golden("g24_photo.npz")


def _ulp_apart(a, b):
    """Largest distance in fp32 units in the last place between two fp32 arrays of one sign."""
    a = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


def _scene_depths(sc):
    xyz_h = np.concatenate([sc.xyz_world, np.ones((len(sc.xyz_world), 1))], -1)
    return xyz_h @ sc.w2c[:, 2, :].T                       # (P, N)


def test_fixture_bounds_equal_the_reference():
    from nerf_fl_amd import colmap
    g = _golden()
    sc = colmap.read_phototourism(SCENE)
    z = _scene_depths(sc)
    near, far, count = _data().depth_bounds(sc.xyz_world, sc.w2c, q=(0.1 / 100, 99.9 / 100), device=DEV)
    assert near.dtype == far.dtype == torch.float64 and near.is_cuda and count.dtype == torch.int32
    assert count.cpu().tolist() == (z > 0).sum(0).tolist()
    scale = float(g["scale_s1"])
    tol = BOUND_REL * np.abs(z).max()
    e_near = np.abs(near.cpu().numpy() - g["nears_s1"] * scale).max()
    e_far = np.abs(far.cpu().numpy() - g["fars_s1"] * scale).max()
    print(f"fixture: near err {e_near:.3e}, far err {e_far:.3e}, tol {tol:.3e}, counts {count.cpu().tolist()}")
    assert e_near <= tol and e_far <= tol
    n2, f2 = _data().scene_bounds(sc, DEV)
    assert np.array_equal(n2, near.cpu().numpy()) and np.array_equal(f2, far.cpu().numpy())


@pytest.mark.parametrize("s", [1, 2])
@pytest.mark.parametrize("split", ["train", "test"])
def test_bank_table_holds_the_golden_bounds(split, s):
    g = _golden()
    bank = _data().ImageBank.from_phototourism(SCENE, split, s, device=DEV)
    ids = g[f"img_ids_{split}_s{s}"]
    assert bank.img_ids == ids.tolist() and bank.host_table["id"].tolist() == ids.tolist()
    assert bank.n_images == (4 if split == "train" else 2)
    rows = [g[f"img_ids_s{s}"].tolist().index(i) for i in ids]
    assert _ulp_apart(bank.host_table["near"], g[f"nears_s{s}"][rows].astype(np.float32)) <= 1
    assert _ulp_apart(bank.host_table["far"], g[f"fars_s{s}"][rows].astype(np.float32)) <= 1
    assert bank.max_id == int(g[f"img_ids_s{s}"].max()) == 1203
    assert isinstance(bank.scale_factor, np.float32) and bank.scale_factor == g[f"scale_s{s}"]
    assert bank.xyz_world.dtype == np.float64
    assert np.abs(bank.xyz_world - g[f"xyz_world_s{s}"]).max() <= 1e-12 * np.abs(g[f"xyz_world_s{s}"]).max()
    assert not bank.white_back and bank.channels == 3
    if split == "test":                                    # the image that sets the scale is a held-out one
        assert _ulp_apart(bank.host_table["far"].max(), np.float32(5)) <= 1


def test_synthetic_scene_equals_numpy_percentile_and_allocates_no_n_by_p_buffer():
    """64 cameras x 200 000 points against np.percentile(z[z > 0], [0.1, 99.9]) in fp64, image by image."""
    n_img, n_pts = 64, 200_000
    rng = np.random.default_rng(1724)
    xyz = rng.standard_normal((n_pts, 3)) * np.array([30.0, 10.0, 30.0])
    w2c = np.tile(np.eye(4), (n_img, 1, 1))
    for i in range(n_img):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        w2c[i, :3, :3] = q * np.sign(np.linalg.det(q))
        w2c[i, :3, 3] = 10.0 * rng.standard_normal(3)      # inside the cloud: every camera has points in front
    xyz_h = np.concatenate([xyz, np.ones((n_pts, 1))], -1)
    z_all = [(xyz_h @ w2c[i].T)[:, 2] for i in range(n_img)]                      # phototourism.py:128
    assert min(np.abs(z).min() for z in z_all) >= 1e-9                            # no depth on the z > 0 edge: must hold
    m = [int((z > 0).sum()) for z in z_all]
    assert min(m) >= 1000 and max(m) <= n_pts - 1000
    exp = np.array([np.percentile(z[z > 0], [0.1, 99.9]) for z in z_all])         # phototourism.py:129-131
    tol = BOUND_REL * max(np.abs(z).max() for z in z_all)

    d_xyz = torch.from_numpy(xyz).to(DEV)
    d_w2c = torch.from_numpy(w2c).to(DEV)
    _data().depth_bounds(d_xyz[:1000], d_w2c[:2])                                 # library load, kernel attributes: once
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    near, far, count = _data().depth_bounds(d_xyz, d_w2c, q=(0.1 / 100, 99.9 / 100))
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - base
    e_near = np.abs(near.cpu().numpy() - exp[:, 0]).max()
    e_far = np.abs(far.cpu().numpy() - exp[:, 1]).max()
    print(f"synthetic: near err {e_near:.3e}, far err {e_far:.3e}, tol {tol:.3e}, memory grown {grown} B, "
          f"m {min(m)} .. {max(m)}")
    assert count.cpu().tolist() == m
    assert e_near <= tol and e_far <= tol
    assert grown < 1_000_000, grown                                               # an (N, P) fp64 buffer is 102 MB


def test_other_quantiles_and_duplicate_depths():
    """Quantiles 0, 0.5 and 1 (integer virtual indexes, the ends) and a cloud where many depths are exactly equal."""
    rng = np.random.default_rng(9)
    xyz = np.round(rng.standard_normal((5001, 3)) * 4) / 4                        # a coarse lattice: ties in depth
    w2c = np.tile(np.eye(4), (3, 1, 1))
    w2c[1, 2, :] = [0.0, 1.0, 0.0, 0.5]
    w2c[2, 2, :] = [1.0, 0.0, 0.0, -0.25]
    for q in ((0.0, 1.0), (0.5, 0.5), (0.25, 0.9)):
        near, far, count = _data().depth_bounds(xyz, w2c, q=q, device=DEV)
        for i in range(3):
            z = xyz @ w2c[i, 2, :3] + w2c[i, 2, 3]
            exp = np.quantile(z[z > 0], q)
            assert count[i].item() == (z > 0).sum()
            assert abs(near[i].item() - exp[0]) <= 1e-12 * np.abs(z).max(), (q, i)
            assert abs(far[i].item() - exp[1]) <= 1e-12 * np.abs(z).max(), (q, i)


def test_degenerate_images():
    from nerf_fl_amd import colmap
    xyz = np.array([[0.0, 0.0, -1.0], [0.5, 0.0, -2.0], [0.0, 0.0, 3.25], [1.0, 1.0, -4.0]])
    w2c = np.tile(np.eye(4), (3, 1, 1))
    w2c[1, 2, 3] = -10.0                                   # everything behind the second camera
    w2c[2, 2, 2] = -1.0                                    # the third looks the other way: three points in front
    near, far, count = _data().depth_bounds(xyz, w2c, device=DEV)
    assert count.cpu().tolist() == [1, 0, 3]
    assert near[0].item() == far[0].item() == 3.25
    assert torch.isnan(near[1]).item() and torch.isnan(far[1]).item()
    exp = np.percentile([1.0, 2.0, 4.0], [0.1, 99.9])
    assert abs(near[2].item() - exp[0]) <= 1e-15 and abs(far[2].item() - exp[1]) <= 4e-15
    sc = colmap.read_phototourism(SCENE)
    z = _scene_depths(sc)
    behind = z[:, 3] < 0                                                          # the points behind the fourth image
    first = int(np.argmax((z[behind] > 0).sum(0) == 0))                           # the first image that sees none of them
    assert behind.sum() >= 20 and first <= 3
    behind = sc.xyz_world[behind]
    with pytest.raises(ValueError, match=sc.filenames[first]):
        _data().scene_bounds(dataclasses.replace(sc, xyz_world=behind), DEV)


@pytest.mark.parametrize("s", [1, 2])
def test_train_split_rows_equal_the_reference(s):
    g = _golden()
    bank = _data().ImageBank.from_phototourism(SCENE, "train", s, device=DEV)
    ref = torch.from_numpy(g[f"all_rays_s{s}"])
    rays, rgbs, ts = bank.materialise(layout="camera")
    assert rays.shape == (ref.shape[0], 5) and bank.n_pixels == ref.shape[0]
    assert torch.equal(rays[:, :3].cpu(), ref[:, :3])
    assert torch.equal(rgbs.cpu(), torch.from_numpy(g[f"all_rgbs_s{s}"]))
    assert torch.equal(ts.cpu(), ref[:, 5].long())
    ulp = max(_ulp_apart(rays[:, 3].cpu().numpy(), ref[:, 3].numpy()), _ulp_apart(rays[:, 4].cpu().numpy(), ref[:, 4].numpy()))
    print(f"train rows s={s}: {ref.shape[0]} rows, near / far within {ulp} ulp")
    assert ulp <= 1


def test_frames_equal_the_reference_test_train_samples():
    g = _golden()
    bank = _data().ImageBank.from_phototourism(SCENE, "train", 2, device=DEV)
    all_ids = g["img_ids_s2"].tolist()
    for k in range(bank.n_images):
        rays, rgbs, ts = bank.frame(k)
        ref = torch.from_numpy(g[f"tt{k}_rays"])
        w, h = g[f"tt{k}_img_wh"].tolist()
        assert (int(bank.host_table[k]["width"]), int(bank.host_table[k]["height"])) == (w, h)
        assert rays.shape == ref.shape == (h * w, 8)
        assert torch.equal(rgbs.cpu(), torch.from_numpy(g[f"tt{k}_rgbs"]))
        assert torch.equal(ts.cpu(), torch.from_numpy(g[f"tt{k}_ts"]))
        got = rays.cpu()
        # origins: the scaled translation, within 1 fp32 ulp of the golden pose's (and of the reference's rows)
        t = g["poses_s2"][all_ids.index(bank.img_ids[k]), :, 3].astype(np.float32)
        assert _ulp_apart(got[:, :3].numpy(), np.broadcast_to(t, (h * w, 3))) <= 1
        assert _ulp_apart(got[:, :3].numpy(), ref[:, :3].numpy()) <= 1
        err = (got[:, 3:6] - ref[:, 3:6]).abs().max().item()
        print(f"frame {k}: {w} x {h}, max direction err {err:.3e}")
        assert err <= du.RAY_TOL                           # tests/test_data_gpu.py's bound for reference-made world rows
        assert _ulp_apart(got[:, 6].numpy(), ref[:, 6].numpy()) <= 1 and _ulp_apart(got[:, 7].numpy(), ref[:, 7].numpy()) <= 1


def test_train_then_score_the_held_out_images():
    """One NeRF-W trainer on the train bank, then the NeRF-W test protocol on the test bank."""
    from nerf_fl_amd import eval as ev
    from nerf_fl_amd.train import RayTrainer
    data = _data()
    train = data.ImageBank.from_phototourism(SCENE, "train", 1, device=DEV)
    test = data.ImageBank.from_phototourism(SCENE, "test", 1, device=DEV)
    assert test.img_ids == _golden()["img_ids_test_s1"].tolist() and test.n_images == 2
    tr = RayTrainer(DEV, N_samples=32, N_importance=32, batch_size=256, lr=1e-3, seed=5, white_back=False, encode_a=True,
                    encode_t=True, N_vocab=train.max_id + 1)
    losses = [tr.fit_epoch(train)[0] for _ in range(3)]
    print("mean loss per epoch:", losses, "steps", tr.global_step)
    assert tr.global_step == 3 * (train.n_pixels // 256) and tr.global_step >= 6
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    res = ev.evaluate_bank(tr.models, tr.embeddings, test, 32, 32, halves=True, fit=dict(n_iters=4, lr=0.1))
    print("held-out psnr", res["psnr"].tolist(), "ssim", res["ssim"].tolist())
    assert res["table"].shape == (2, 8) and res["codes"].shape[0] == 2
    assert torch.isfinite(res["psnr"]).all() and torch.isfinite(res["ssim"]).all()
