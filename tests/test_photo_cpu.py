"""nerf_fl_amd.colmap.read_phototourism on the fixture scene (tests/golden/make_photo_golden.py: written by its own COLMAP
writer, read back by the REAL reference's PhototourismDataset), and what of nfl_depth_bounds can be checked without a
device: argument validation (nfl_bounds_args and the signature are held to the header in tests/test_abi_cpu.py)."""
import ctypes as C
import os
import shutil
import struct

import numpy as np
import pytest

from nerf_fl_amd import _lib, colmap, data

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "data_photo")


def _golden():
    return dict(np.load(os.path.join(HERE, "golden", "g24_photo.npz")))


def _close(got, exp, rel=1e-12):
    """|got - exp| <= rel * max|exp|: both sides are fp64 and differ in the order of a few operations at most."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.float64
    err = np.abs(got - exp).max()
    assert err <= rel * np.abs(exp).max(), (err, np.abs(exp).max())
    return err


@pytest.mark.parametrize("s", [1, 2])
def test_read_phototourism_equals_the_reference(s):
    g = _golden()
    sc = colmap.read_phototourism(SCENE, s)
    assert sc.img_ids.dtype == np.int64 and np.array_equal(sc.img_ids, g[f"img_ids_s{s}"])
    assert sc.img_ids_train == g[f"img_ids_train_s{s}"].tolist() and len(sc.img_ids_train) == 4
    assert sc.img_ids_test == g[f"img_ids_test_s{s}"].tolist() and len(sc.img_ids_test) == 2
    assert sc.K.dtype == np.float32 and g[f"Ks_s{s}"].dtype == np.float32
    assert np.array_equal(sc.K, g[f"Ks_s{s}"])
    scale = g[f"scale_s{s}"]
    assert scale.dtype == np.float32
    exp = g[f"poses_s{s}"].copy()
    exp[..., 3] *= scale                                   # undo phototourism.py:135: the reader returns unscaled poses
    print("poses", _close(sc.poses, exp), "xyz", _close(sc.xyz_world, g[f"xyz_world_s{s}"] * scale))
    assert sc.xyz_world.shape == (600, 3)
    assert sc.w2c.shape == (6, 4, 4) and sc.w2c.dtype == np.float64
    assert sc.scene_name == "scene" and len(sc.filenames) == 6 and "dropped_077.png" not in sc.filenames


def test_the_fixture_exercises_the_id_rules():
    """TSV order differs from images.bin, the `id` column is junk, one row is dropped, one image is unlisted, two
    images share a camera."""
    sc = colmap.read_phototourism(SCENE)
    by_name = colmap.read_images_bin(os.path.join(SCENE, "dense", "sparse", "images.bin"))
    assert len(by_name) == 8 and "unlisted_099.png" in by_name and "dropped_077.png" in by_name
    in_bin_order = [v[0] for v in by_name.values() if v[0] in set(sc.img_ids.tolist())]
    assert sorted(in_bin_order) == sorted(sc.img_ids.tolist()) and in_bin_order != sc.img_ids.tolist()
    cams = [by_name[n][1] for n in sc.filenames]
    assert len(set(cams)) == 5
    with open(os.path.join(SCENE, "scene.tsv")) as f:
        lines = f.read().splitlines()
    assert len(lines) == 8 and sum(1 for ln in lines[1:] if ln.split("\t")[1] == "") == 1
    assert all(int(ln.split("\t")[1]) not in sc.img_ids for ln in lines[1:] if ln.split("\t")[1])


def _copy_scene(tmp_path):
    dst = tmp_path / "scene"
    shutil.copytree(SCENE, dst)
    return str(dst)


def test_another_camera_model_raises_value_error(tmp_path):
    root = _copy_scene(tmp_path)
    path = os.path.join(root, "dense", "sparse", "cameras.bin")
    buf = bytearray(open(path, "rb").read())
    cam_id, model = struct.unpack_from("<ii", buf, 8)
    assert model == 1
    struct.pack_into("<i", buf, 12, 2)                     # SIMPLE_RADIAL: also 4 parameters, so the file stays well formed
    open(path, "wb").write(bytes(buf))
    with pytest.raises(ValueError, match="SIMPLE_RADIAL"):
        colmap.read_phototourism(root)
    struct.pack_into("<i", buf, 12, 77)
    open(path, "wb").write(bytes(buf))
    with pytest.raises(ValueError, match="77"):
        colmap.read_phototourism(root)


def test_a_file_name_missing_from_images_bin_raises_key_error(tmp_path):
    root = _copy_scene(tmp_path)
    with open(os.path.join(root, "scene.tsv"), "a") as f:
        f.write("nowhere.png\t5\ttrain\n")
    with pytest.raises(KeyError, match="nowhere.png"):
        colmap.read_phototourism(root)


def test_downscale_below_one_is_refused():
    with pytest.raises(ValueError):
        colmap.read_phototourism(SCENE, 0)


def test_c_argument_validation():
    """Everything nfl_depth_bounds refuses, it refuses before a launch: checkable without a device."""
    L = _lib.lib()
    assert L.nfl_depth_bounds(None, None) == -1
    dummy = C.c_void_p(64)
    good = dict(d_xyz=dummy, d_row=dummy, n_points=10, n_images=2, q_lo=0.001, q_hi=0.999, d_bounds=dummy, d_count=dummy)
    for bad in (dict(d_xyz=None), dict(d_row=None), dict(d_bounds=None), dict(d_count=None), dict(n_points=0),
                dict(n_points=2 ** 30 + 1), dict(n_images=0), dict(q_lo=-0.1), dict(q_hi=1.5), dict(q_lo=float("nan"))):
        a = _lib.BoundsArgs(**{**good, **bad})
        assert L.nfl_depth_bounds(C.byref(a), None) == -1, bad


def test_python_layer_needs_a_device_and_checks_shapes():
    xyz, w2c = np.zeros((5, 3)), np.tile(np.eye(4), (2, 1, 1))
    with pytest.raises(RuntimeError, match="no CPU path"):
        data.depth_bounds(xyz, w2c)
    with pytest.raises(RuntimeError, match="no CPU path"):
        data.ImageBank.from_phototourism(SCENE)
    with pytest.raises(ValueError):
        data.ImageBank.from_phototourism(SCENE, split="val", device="cuda:0")
