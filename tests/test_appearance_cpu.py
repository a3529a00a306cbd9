"""Appearance fitting (nerf_fl_amd.appearance, C ABI nfl_appearance_cache / nfl_appearance_fit): what can be checked
without a device -- argument validation (nfl_appfit_args and the signatures are held to the header in
tests/test_abi_cpu.py)."""
import ctypes as C

import pytest
import torch

from nerf_fl_amd import NeRF, PosEmbedding, _lib
from nerf_fl_amd.appearance import AppearanceFit


def test_c_argument_validation():
    L = _lib.lib()
    assert L.nfl_appfit_partials_floats(10) == 10 * 129
    assert L.nfl_appfit_partials_floats(-1) == 0
    assert L.nfl_appearance_fit(None, None) == -1
    assert L.nfl_appearance_cache(None, None, None, None, None, 64, None) == -1
    a = _lib.AppFitArgs()
    dummy = C.c_void_p(16)
    a.d_codes = a.d_w_dir = a.d_grad = a.d_loss = a.d_image_items = dummy
    a.n_rays, a.n_samples, a.n_pad, a.n_items, a.n_images, a.n_a, a.ld_dir, a.col_a = 8, 96, 100, 0, 1, 48, 331, 283
    assert L.nfl_appearance_fit(C.byref(a), None) == -1          # n_pad not a multiple of 64
    a.n_pad = 64
    assert L.nfl_appearance_fit(C.byref(a), None) == -1          # n_pad < n_samples
    a.n_pad, a.n_samples = 320, 260
    assert L.nfl_appearance_fit(C.byref(a), None) == -1          # more than 256 samples
    a.n_pad, a.n_samples, a.ld_dir = 128, 96, 330
    assert L.nfl_appearance_fit(C.byref(a), None) == -1          # appearance columns beyond the weight's row
    a.ld_dir, a.n_items = 331, 4
    assert L.nfl_appearance_fit(C.byref(a), None) == -1          # work items but no cache / partials


def _models(appearance=True):
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    return {"coarse": NeRF("coarse"), "fine": NeRF("fine", encode_appearance=appearance, in_channels_a=48)}, emb


def test_python_validation_needs_no_device():
    rays = torch.zeros(10, 8)
    rgb = torch.zeros(10, 3)
    idx = torch.zeros(10, dtype=torch.int64)
    models, emb = _models(appearance=False)
    with pytest.raises(ValueError, match="appearance"):
        AppearanceFit(models, emb, rays, rgb, idx, 64, 64)
    models, emb = _models()
    with pytest.raises(ValueError, match="N_importance"):
        AppearanceFit(models, emb, rays, rgb, idx, 64, 0)
    with pytest.raises(ValueError, match="max_cache_bytes"):
        AppearanceFit(models, emb, rays, rgb, idx, 64, 64, max_cache_bytes=10 * 128 * 128 * 4 - 1)
    with pytest.raises(ValueError, match="256"):
        AppearanceFit(models, emb, rays, rgb, idx, 128, 160)
