"""nfl_image_metrics / nfl_depth_image without a device: the argument checks of the C ABI (everything refused or empty
returns before a launch, so no GPU is touched), and the torch restatement of the SSIM definition the GPU tests compare
the kernel with (tests/metrics_util.py)."""
import ctypes as C

import pytest
import torch

import data_util as du
import metrics_util as mu
from nerf_fl_amd import _lib

EINVAL = -1
FAKE = 0x1000          # a non-NULL pointer that is never followed: every call below returns before a launch


def _metrics_args(**over):
    a = _lib.MetricsArgs()
    a.d_pred = a.d_target = a.d_results = a.d_scratch = FAKE
    a.width, a.height = 40, 30
    a.x0, a.x1, a.y0, a.y1 = 0, 40, 0, 30
    a.clip, a.slot, a.n_slots = 1, 0, 1
    a.scratch_bytes = 1 << 20
    for k, v in over.items():
        setattr(a, k, v)
    return a


def _depth_args(**over):
    a = _lib.DepthArgs()
    a.d_depth = a.d_image = a.d_scratch = FAKE
    a.width, a.height = 40, 30
    a.x0, a.x1, a.y0, a.y1 = 0, 40, 0, 30
    a.scratch_bytes = 1 << 20
    for k, v in over.items():
        setattr(a, k, v)
    return a


BANK = dict(d_target=None, d_pixels=FAKE, d_table=FAKE, n_images=3, image=1)


@pytest.mark.parametrize("why,over", [
    ("no prediction", dict(d_pred=None)),
    ("no results", dict(d_results=None)),
    ("no scratch", dict(d_scratch=None)),
    ("neither ground truth", dict(d_target=None)),
    ("both ground truths", dict(d_pixels=FAKE, d_table=FAKE, n_images=1)),
    ("bank without table", dict(BANK, d_table=None)),
    ("bank image out of range", dict(BANK, image=3)),
    ("mask without target", dict(BANK, d_mask=FAKE)),
    ("region right of the image", dict(x1=41)),
    ("region below the image", dict(y1=31)),
    ("negative origin", dict(x0=-1)),
    ("reversed region", dict(x0=20, x1=10)),
    ("one pixel wide", dict(x0=7, x1=8)),
    ("one pixel high", dict(y0=7, y1=8)),
    ("slot outside the table", dict(slot=1)),
    ("no image", dict(width=0, x1=0)),
    ("scratch too small", dict(scratch_bytes=39)),
])
def test_image_metrics_refuses(why, over):
    assert _lib.lib().nfl_image_metrics(C.byref(_metrics_args(**over)), None) == EINVAL, why


def test_image_metrics_null_args_and_empty_regions():
    lib = _lib.lib()
    assert lib.nfl_image_metrics(None, None) == EINVAL
    for over in (dict(x0=5, x1=5), dict(y0=30, y1=30), dict(BANK, x0=0, x1=0)):
        assert lib.nfl_image_metrics(C.byref(_metrics_args(**over)), None) == 0, over


def test_scratch_sizes():
    lib = _lib.lib()
    # one partial of 5 doubles per tile of 64 columns x 16 rows
    assert lib.nfl_image_metrics_scratch_bytes(30, 40) == 2 * 40
    assert lib.nfl_image_metrics_scratch_bytes(800, 800) == 13 * 50 * 40
    assert lib.nfl_image_metrics_scratch_bytes(0, 40) == 0 and lib.nfl_image_metrics_scratch_bytes(4, -1) == 0
    assert 0 < lib.nfl_depth_image_scratch_bytes(800, 800) <= 2048 and lib.nfl_depth_image_scratch_bytes(1, 1) == 8
    assert lib.nfl_depth_image_scratch_bytes(0, 3) == 0


@pytest.mark.parametrize("why,over", [
    ("no depth", dict(d_depth=None)), ("no image", dict(d_image=None)), ("no scratch", dict(d_scratch=None)),
    ("region outside", dict(y1=31)), ("reversed", dict(y0=9, y1=8)), ("scratch too small", dict(scratch_bytes=15)),
])
def test_depth_image_refuses(why, over):
    assert _lib.lib().nfl_depth_image(C.byref(_depth_args(**over)), None) == EINVAL, why


def test_depth_image_null_args_and_empty_region():
    lib = _lib.lib()
    assert lib.nfl_depth_image(None, None) == EINVAL
    assert lib.nfl_depth_image(C.byref(_depth_args(x0=3, x1=3)), None) == 0


def test_python_surface_exists_and_refuses_the_host():
    from nerf_fl_amd import eval as ev, metrics
    from nerf_fl_amd.train import RayTrainer
    assert metrics.METRIC_COLUMNS == ("sse", "count", "sse_valid", "count_valid", "ssim_sum", "psnr", "psnr_valid", "ssim")
    assert callable(ev.evaluate_bank) and callable(RayTrainer.validate_bank)
    with pytest.raises(RuntimeError):
        metrics.image_metrics(torch.zeros(16, 3), 4, 4, target=torch.zeros(16, 3))
    with pytest.raises(RuntimeError):
        metrics.depth_image(torch.zeros(16), 4, 4)


# ---- the restatement itself -------------------------------------------------------------------------------------------
def _images():
    from nerf_fl_amd import data
    small = data.ImageBank.from_blender(du.SCENE_SMALL, "train", (24, 24), ())
    photo = data.ImageBank(**du.photo_inputs()[1])
    return [mu.host_image(small, 1)[0]] + [mu.host_image(photo, i)[0] for i in range(photo.n_images)]


def test_window_sums_to_one_and_ssim_of_an_image_with_itself_is_one():
    assert abs(mu.window(torch.float64).sum().item() - 1.0) < 1e-15
    for img in _images():
        for dtype in (torch.float32, torch.float64):
            m = mu.ssim_map(img, img, dtype)
            assert m.shape == img.shape and torch.equal(m, torch.ones_like(m))
            assert mu.reference(img, img, dtype=dtype)["ssim"] == 1.0


def test_fp32_and_fp64_restatements_agree():
    """d_ref: the largest per-pixel distance between the reference's fp32 arithmetic and the truth.  Bound: the moments
    are sums of 9 products of values in [0, 1] (noise: up to about 3), so F(p p) - mu^2 carries a few fp32 roundings of
    numbers up to 10: below 1e-5 absolute against s1 + s2 + C2 >= about C2 = 9e-4, i.e. a relative error of the
    quotient of the order 1e-2 in the worst pixel."""
    worst = 0.0
    for k, img in enumerate(_images()):
        for name, sigma in mu.NOISE:
            for clip in (True, False):
                pred = mu.noisy(img, sigma, 10 * k + 1)
                a, b = (mu.reference(pred, img, clip=clip, dtype=d) for d in (torch.float32, torch.float64))
                d_ref = (a["map"].double() - b["map"]).abs().max().item()
                worst = max(worst, d_ref)
                print(f"image {k} {tuple(img.shape)} noise {name} clip {clip}: d_ref {d_ref:.3e}, ssim fp32 {a['ssim']:.8f} "
                      f"fp64 {b['ssim']:.8f}")
                assert a["sse"] == b["sse"] and a["count"] == b["count"] == img.numel()
                assert abs(a["ssim"] - b["ssim"]) <= d_ref
    assert 0.0 < worst <= 5e-2


def test_region_is_the_crop():
    img = _images()[1]
    H, W = img.shape[:2]
    pred = mu.noisy(img, 0.1, 3)
    valid = torch.rand(H, W, generator=torch.Generator().manual_seed(1)) < 0.7
    for region in ((W // 2, W, 0, H), (1, 3, 2, H - 1), (3, W - 2, 1, 3)):
        a = mu.reference(pred, img, valid, region=region)
        b = mu.reference(mu.crop(pred, region).contiguous(), mu.crop(img, region).contiguous(), mu.crop(valid, region))
        assert torch.equal(a["map"], b["map"]) and all(a[k] == b[k] for k in a if k != "map")
        # the border of the crop is a reflection of the crop, not the neighbouring pixels of the full image
        full = mu.reference(pred, img)["map"]
        assert not torch.equal(mu.crop(full, region), a["map"])


def test_depth_restatement():
    import numpy as np
    d = np.array([[1.0, np.nan, 3.0], [2.0, 2.5, 1.5]], dtype=np.float32)
    out = mu.depth_reference(d)
    assert out.dtype == np.uint8 and out.shape == (2, 3, 3)
    assert out[0, 1, 0] == 0 and out[0, 2, 0] in (254, 255) and out[0, 0, 1] == int(np.float32(255) * np.float32(1 / 3))
    assert (mu.depth_reference(np.full((2, 2), 4.0, np.float32)) == 0).all()
