"""Appearance fitting (nerf_fl_amd.appearance, C ABI nfl_appearance_cache / nfl_appearance_fit): what can be checked
without a device -- the exported symbols, the ctypes mirror of nfl_appfit_args, argument validation."""
import ctypes as C
import os
import subprocess
import tempfile

import pytest
import torch

from nerf_fl_amd import NeRF, PosEmbedding, _lib
from nerf_fl_amd.appearance import AppearanceFit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("nfl_appearance_cache", "nfl_appfit_partials_floats", "nfl_appearance_fit")


def test_new_symbols_are_exported():
    names = [s[0] for s in _lib.SYMBOLS]
    L = _lib.lib()
    for n in NEW:
        assert n in names
        getattr(L, n)
    assert L.nfl_abi_version() == _lib.NFL_ABI_VERSION == 10


def test_appfit_args_layout_matches_the_header():
    src = ('#include <stdio.h>\n#include <stddef.h>\n#include "nerf_fl_amd.h"\nint main(void) {\n'
           '  printf("%zu %zu %zu\\n", sizeof(nfl_appfit_args), offsetof(nfl_appfit_args, n_rays), '
           'offsetof(nfl_appfit_args, d_partials));\n  return 0;\n}\n')
    with tempfile.TemporaryDirectory() as td:
        c, exe = os.path.join(td, "sz.c"), os.path.join(td, "sz")
        with open(c, "w") as f:
            f.write(src)
        subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        size, off_n, off_p = map(int, subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_lib.AppFitArgs)
    assert off_n == _lib.AppFitArgs.n_rays.offset and off_p == _lib.AppFitArgs.d_partials.offset


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
