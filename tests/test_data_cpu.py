"""nerf_fl_amd.data without a GPU: ImageBank.from_blender against fixtures written by the real reference's
datasets/blender.py and datasets/ray_utils.py (tests/golden/make_data_golden.py), the generic constructor against
Phototourism-style rows, the keyed permutation's properties (on the restatement in data_util, which the GPU test pins
the kernel to), the batch arithmetic of fit_epoch(bank), and the C entry point's argument checks."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import data_util as du
from abi_probe import probe
from nerf_fl_amd import _lib, data


def _bank_rows(bank, q, layout="world"):
    return du.expected_rows(bank.host_table, bank.host_pixels, q, layout)


def _check_blender_meta(bank, K, size, n):
    t = bank.host_table
    assert bank.n_images == n and bank.n_pixels == n * size * size and bank.white_back and bank.channels == 4
    assert bank.nbytes == n * size * size * 4 + n * data.RECORD.itemsize
    assert (t["width"] == size).all() and (t["height"] == size).all() and (t["id"] == np.arange(n)).all()
    assert (t["pix0"] == np.arange(n) * size * size).all() and (t["byte0"] == t["pix0"] * 4).all()
    assert (t["near"] == 2.0).all() and (t["far"] == 6.0).all()
    for k, v in (("fx", K[0, 0]), ("fy", K[1, 1]), ("cx", K[0, 2]), ("cy", K[1, 2])):
        assert (t[k] == np.float32(v)).all(), k


@pytest.mark.parametrize("tag,pert", [("plain", ()), ("pert", ("color", "occ"))])
def test_from_blender_small_scene_in_full(tag, pert):
    g = du.golden("g23_data_small.npz")
    bank = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), pert)
    _check_blender_meta(bank, g["K"], 24, 3)
    ref_rays, ref_rgbs = torch.from_numpy(g[f"rays_{tag}"]), torch.from_numpy(g[f"rgbs_{tag}"])
    # c2w[:, 3] is the reference's origin column, image by image
    assert np.array_equal(bank.host_table["c2w"][:, [3, 7, 11]], g[f"rays_{tag}"][::576, :3])
    rays, rgbs, ts = _bank_rows(bank, np.arange(bank.n_pixels))
    assert torch.equal(rgbs, ref_rgbs)
    assert torch.equal(ts, ref_rays[:, 8].long())
    print("small", tag, "max ray err", du.check_rays(rays, ref_rays[:, :8]))


def test_from_blender_800_with_color_and_occluders():
    g = du.golden("g23_data_big.npz")
    bank = data.ImageBank.from_blender(du.SCENE, "train", (800, 800), ("color", "occ"))
    _check_blender_meta(bank, g["K"], 800, 3)
    assert np.array_equal(bank.host_pixels.reshape(3, 800, 800, 4), g["pixels"])
    alpha = g["pixels"][..., 3]
    assert ((alpha > 0) & (alpha < 255)).any()
    assert not np.array_equal(g["pixels"][1, 200:600, 200:600], np.array(_open(du.SCENE, 1))[200:600, 200:600])
    rays, rgbs, ts = _bank_rows(bank, g["rows"])
    assert torch.equal(rgbs, torch.from_numpy(g["rgbs"]))
    assert torch.equal(ts, torch.from_numpy(g["rays"][:, 8]).long())
    print("big max ray err", du.check_rays(rays, torch.from_numpy(g["rays"][:, :8])))


def _open(root, t):
    from PIL import Image
    return Image.open(os.path.join(root, "train", f"r_{t}.png"))


def test_from_blender_resizes_with_lanczos_after_the_perturbation():
    from PIL import Image
    g = du.golden("g23_data_big.npz")
    bank = data.ImageBank.from_blender(du.SCENE, "train", (200, 200), ("color", "occ"))
    K = g["K"].copy()
    K[0, 0] = K[1, 1] = g["K"][0, 0] * (200 / 800)
    K[0, 2] = K[1, 2] = 100.0
    _check_blender_meta(bank, K, 200, 3)
    exp = np.stack([np.array(Image.fromarray(p).resize((200, 200), Image.LANCZOS)) for p in g["pixels"]])
    assert np.array_equal(bank.host_pixels.reshape(3, 200, 200, 4), exp)


@pytest.mark.parametrize("layout,key", [("camera", "cam_rows"), ("world", "world_rows")])
def test_generic_constructor_on_unequal_rgb_images(layout, key):
    g, kw = du.photo_inputs()
    bank = data.ImageBank(**kw)
    sizes = g["sizes"]
    assert bank.n_pixels == int((sizes[:, 0] * sizes[:, 1]).sum()) and not bank.white_back
    assert bank.nbytes == bank.n_pixels * 3 + 3 * data.RECORD.itemsize
    assert (bank.host_table["pix0"] == np.concatenate([[0], np.cumsum(sizes[:, 0] * sizes[:, 1])[:-1]])).all()
    rays, rgbs, ts = _bank_rows(bank, np.arange(bank.n_pixels), layout)
    assert torch.equal(rgbs, torch.from_numpy(g["rgbs"]))
    assert torch.equal(ts, torch.from_numpy(g["cam_rows"][:, 5]).long())
    ref = torch.from_numpy(g[key])
    du.check_rays(rays, ref[:, :5] if layout == "camera" else ref, layout)


def test_constructor_rejects_bad_input():
    g, kw = du.photo_inputs()
    with pytest.raises(ValueError):
        data.ImageBank(**dict(kw, images=kw["images"][:2]))
    with pytest.raises(ValueError):
        data.ImageBank(**dict(kw, images=[kw["images"][0].astype(np.float32)] + kw["images"][1:]))
    with pytest.raises(ValueError):       # RGB and RGBA mixed
        data.ImageBank(**dict(kw, images=[np.zeros((4, 4, 4), np.uint8)] + kw["images"][1:]))
    with pytest.raises(RuntimeError, match="no CPU path"):
        data.ImageBank(**kw).gather(0, 4)
    with pytest.raises(RuntimeError, match="no CPU path"):
        data.ImageBank(**kw).to("cpu")


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 2 ** 16, 2 ** 16 + 1, 999983])
def test_permutation_is_a_bijection(n):
    p = np.arange(n)
    a, b = du.perm(0x1234, n, p), du.perm(0x1235, n, p)
    for x in (a, b):
        assert x.min() >= 0 and x.max() < n and np.unique(x).size == n
    if n >= 1000:
        assert (a != b).mean() > 0.9 and (a != p).mean() > 0.9
    assert np.array_equal(du.perm(0, n, p), p)


def test_epoch_keys():
    keys = {data.epoch_key(s, e) for s in range(4) for e in range(16)}
    assert len(keys) == 64 and 0 not in keys and all(0 < k < 2 ** 64 for k in keys)
    # the package's splitmix64 is the stream the restatement (and the kernel's host side) draws round keys from
    assert data.splitmix64(5) & 0xFFFFFFFF == du.round_keys(5)[0]


@pytest.mark.parametrize("key", [1, 2, 3])
def test_first_batches_are_uniform_over_the_images(key):
    """64 equal images of 128 x 128; the image histogram of the first 64 batches of 1024 positions stays below the
    0.999 chi-square quantile (63 degrees of freedom) -- and so does a true randperm seeded with the same number, i.e.
    the keys are not picked to flatter the bound."""
    from scipy.stats import chi2
    n_img, per = 64, 128 * 128
    n, m = n_img * per, 64 * 1024
    bound = chi2.ppf(0.999, n_img - 1)

    def stat(q):
        hist = np.bincount(q // per, minlength=n_img)
        return float(((hist - m / n_img) ** 2 / (m / n_img)).sum())

    true = stat(torch.randperm(n, generator=torch.Generator().manual_seed(key))[:m].numpy())
    ours = stat(du.perm(key, n, np.arange(m)))
    print(f"key {key}: chi2 ours {ours:.1f}, randperm {true:.1f}, bound {bound:.1f}")
    assert true < bound
    assert ours < bound


@pytest.mark.parametrize("world", [1, 2, 8])
def test_batch_ranges_are_disjoint_and_cover_a_prefix(world):
    n, bs = 100000, 96
    steps = n // (bs * world)
    starts = sorted(data.batch_range(s, r, world, bs) for s in range(steps) for r in range(world))
    assert starts == list(range(0, steps * world * bs, bs))
    assert starts[-1] + bs <= n < (steps + 1) * world * bs


def test_gather_entry_point_validates_arguments():
    L = _lib.lib()
    assert L.nfl_gather_batch(None, None) == -1
    a = _lib.GatherArgs()
    assert L.nfl_gather_batch(C.byref(a), None) == -1                       # no pixels, no table
    a.d_pixels, a.d_table, a.n_images, a.n_pixels, a.count = 16, 16, 1, 64, 8
    a.start = 60
    assert L.nfl_gather_batch(C.byref(a), None) == -1                       # range past the end
    a.start, a.layout = 0, 2
    assert L.nfl_gather_batch(C.byref(a), None) == -1                       # unknown layout
    a.layout, a.n_pixels = 0, 1 << 40
    assert L.nfl_gather_batch(C.byref(a), None) == -1                       # >= 2^40 pixels
    a.n_pixels, a.count = 64, 0
    assert L.nfl_gather_batch(C.byref(a), None) == 0                        # empty range
    a.count = 8
    assert L.nfl_gather_batch(C.byref(a), None) == 0                        # every output NULL: nothing to launch


def test_struct_layouts_match_the_header():
    """data.RECORD against the compiled nfl_image_rec (every struct's ctypes mirror: tests/test_abi_cpu.py)."""
    rec = probe()["structs"]["nfl_image_rec"]
    assert data.RECORD.itemsize == rec["size"] == C.sizeof(_lib.ImageRec)
    for name, _ in _lib.ImageRec._fields_:
        assert data.RECORD.fields[name][1] == rec["fields"][name][0] == getattr(_lib.ImageRec, name).offset, name
