#!/usr/bin/env python3
"""Generate the Phototourism fixtures (tests/test_photo_cpu.py, tests/test_photo_gpu.py): write a tiny synthetic scene in
COLMAP's binary layout, then run the REAL reference's datasets/phototourism.py (PhototourismDataset) on it, loaded by
file path, and record what it computes.

The stubs of make_data_golden.py stand in for kornia.create_meshgrid and torchvision.transforms.ToTensor; bare `utils`
and `models` packages are registered so that utils.lie_group_helper and models.poses load by path without the
reference's utils/__init__.py (which pulls in optimiser packages the dataset does not need).

Written under tests/golden/:
  data_photo/scene.tsv                          columns filename, id, split; the `id` column holds junk on purpose
  data_photo/dense/sparse/{cameras,images,points3D}.bin   by this file's own struct writer
  data_photo/dense/images/*.png                 6 images, 12 .. 48 px, three odd sizes, one of them greyscale
  g24_photo.npz                                 per img_downscale s in (1, 2), from PhototourismDataset(root, 'train', s):
                                                img_ids, Ks (per image, TSV order), poses, nears, fars, xyz_world, scale,
                                                img_ids_train, img_ids_test, all_rays (., 6), all_rgbs; and from
                                                split='test_train' at s = 2 each sample's rays (h w, 8), rgbs, ts, img_wh

The scene satisfies, asserted below before anything is written: two images share one camera; the TSV order differs from
the images.bin order; one TSV row has an empty id; one image of images.bin is not in the TSV; 4 train and 2 test images;
every image has >= 200 points in front and >= 20 behind; no |depth| < 1e-6; both virtual percentile indexes of every
image are non-integer; the image with the largest far bound is a test image.

Runs only where the reference checkout is; the GPU machine sees the files alone.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_photo_golden.py [path/to/reference]
"""
import importlib.util
import os
import struct
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
from make_data_golden import _install_stubs, _np          # noqa: E402  (the same stubs)

REF = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].startswith("-") else "/root/reference"
SCENE = os.path.join(HERE, "data_photo")
N_POINTS = 600

# images.bin order: (image id, camera id, file name).  Cameras: id -> (w, h); camera 5 is shared by ids 11 and 1203.
CAMERAS = {2: (23, 17), 5: (30, 12), 9: (48, 31), 4: (16, 40), 7: (36, 24)}
IMAGES = [(42, 2, "b_042.png"), (11, 5, "a_011.png"), (7, 9, "c_007.png"), (1203, 5, "d_1203.png"),
          (350, 4, "e_350.png"), (58, 7, "f_058.png"),
          (77, 7, "dropped_077.png"),             # in the TSV with an empty id: dropped
          (99, 2, "unlisted_099.png")]            # not in the TSV
TSV_ORDER = [1203, 7, 77, 58, 42, 350, 11]        # differs from the images.bin order


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def _load_reference():
    for pkg in ("utils", "models", "datasets"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(REF, pkg)]
        sys.modules[pkg] = m
    _load("utils.lie_group_helper", os.path.join(REF, "utils", "lie_group_helper.py"))
    _load("models.poses", os.path.join(REF, "models", "poses.py"))
    _load("datasets.ray_utils", os.path.join(REF, "datasets", "ray_utils.py"))
    _load("datasets.colmap_utils", os.path.join(REF, "datasets", "colmap_utils.py"))
    return _load("datasets.phototourism", os.path.join(REF, "datasets", "phototourism.py"))


def _rotmat_to_qvec(R):
    """Unit quaternion (w, x, y, z) of a rotation matrix (trace branch chosen for the largest pivot)."""
    t = np.trace(R)
    if t > 0:
        s = 2 * np.sqrt(1 + t)
        q = np.array([s / 4, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
        q = np.empty(4)
        q[0] = (R[k, j] - R[j, k]) / s
        q[1 + i] = s / 4
        q[1 + j] = (R[j, i] + R[i, j]) / s
        q[1 + k] = (R[k, i] + R[i, k]) / s
    return q / np.linalg.norm(q)


def _make_scene(rng):
    """Points scattered round the origin; cameras a few units out, looking roughly at it, so each has points behind."""
    xyz = rng.standard_normal((N_POINTS, 3)) * np.array([3.0, 2.0, 3.0])
    cams = {}
    for img_id, _, _ in IMAGES:
        centre = rng.standard_normal(3)
        centre *= rng.uniform(1.5, 4.0) / np.linalg.norm(centre)
        fwd = -centre / np.linalg.norm(centre) + 0.2 * rng.standard_normal(3)
        fwd /= np.linalg.norm(fwd)
        right = np.cross(fwd, rng.standard_normal(3))
        right /= np.linalg.norm(right)
        down = np.cross(fwd, right)
        R = np.stack([right, down, fwd])                       # world -> camera ("right down front")
        q = _rotmat_to_qvec(R)
        cams[img_id] = (q, -R @ centre)
    return xyz, cams


def _write_binaries(root, xyz, cams, rng):
    sparse = os.path.join(root, "dense", "sparse")
    os.makedirs(sparse, exist_ok=True)
    with open(os.path.join(sparse, "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(CAMERAS)))
        for cam_id, (w, h) in CAMERAS.items():
            fx, fy = w * rng.uniform(0.9, 1.2), h * rng.uniform(1.1, 1.4)
            f.write(struct.pack("<iiQQ4d", cam_id, 1, w, h, fx, fy, w / 2, h / 2))            # model 1 = PINHOLE
    with open(os.path.join(sparse, "images.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(IMAGES)))
        for img_id, cam_id, name in IMAGES:
            q, t = cams[img_id]
            f.write(struct.pack("<i7di", img_id, *q, *t, cam_id) + name.encode() + b"\0" + struct.pack("<Q", 0))
    with open(os.path.join(sparse, "points3D.bin"), "wb") as f:
        f.write(struct.pack("<Q", len(xyz)))
        ids = rng.permutation(10 * len(xyz))[:len(xyz)]                                        # ids in no order
        for pid, p in zip(ids, xyz):
            f.write(struct.pack("<Q3d3BdQ", int(pid), *p, *rng.integers(0, 256, 3).tolist(), rng.random(), 2))
            f.write(struct.pack("<4i", IMAGES[0][0], 0, IMAGES[1][0], 0))                     # a short track


def _check_scene(xyz, cams):
    """The conditions of the module docstring that depend on the geometry; returns the unscaled far bound per id."""
    fars = {}
    xyz_h = np.concatenate([xyz, np.ones((len(xyz), 1))], -1)
    for img_id in [i for i in TSV_ORDER if i != 77]:
        q, t = cams[img_id]
        w, x, y, z = q
        row2 = np.array([2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x ** 2 - 2 * y ** 2, t[2]])
        depth = xyz_h @ row2
        m = int((depth > 0).sum())
        assert m >= 200 and int((depth <= 0).sum()) >= 20, (img_id, m)
        assert np.abs(depth).min() >= 1e-6, img_id
        for pct in (0.1, 99.9):
            v = pct / 100 * (m - 1)
            assert v != np.floor(v), (img_id, pct, m)
        fars[img_id] = np.percentile(depth[depth > 0], 99.9)
    return fars


def main():
    _install_stubs()
    photo = _load_reference()
    rng = np.random.default_rng(24)
    xyz, cams = _make_scene(rng)
    fars = _check_scene(xyz, cams)

    listed = [i for i in TSV_ORDER if i != 77]
    far_first = sorted(listed, key=lambda i: -fars[i])
    test_ids = {far_first[0], far_first[3]}                     # the farthest-reaching image is held out
    names = {img_id: name for img_id, _, name in IMAGES}
    cam_of = {img_id: cam for img_id, cam, _ in IMAGES}
    assert [i for i, _, _ in IMAGES if i in listed] != listed                                  # TSV order differs
    assert len({cam_of[i] for i in listed}) < len(listed)                                      # a shared camera
    assert 99 not in TSV_ORDER and max(fars, key=fars.get) in test_ids
    assert len(test_ids) == 2 and len(listed) - len(test_ids) == 4

    _write_binaries(SCENE, xyz, cams, rng)
    os.makedirs(os.path.join(SCENE, "dense", "images"), exist_ok=True)
    for k, img_id in enumerate(listed):
        w, h = CAMERAS[cam_of[img_id]]
        if k == 2:
            img = Image.fromarray(rng.integers(0, 256, (h, w), dtype=np.uint8), "L")           # .convert('RGB') matters
        else:
            img = Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB")
        img.save(os.path.join(SCENE, "dense", "images", names[img_id]), optimize=True)
    with open(os.path.join(SCENE, "scene.tsv"), "w") as f:
        f.write("filename\tid\tsplit\n")
        for k, img_id in enumerate(TSV_ORDER):
            junk = "" if img_id == 77 else str(900 + k)
            f.write(f"{names[img_id]}\t{junk}\t{'test' if img_id in test_ids else 'train'}\n")

    out = {}
    for s in (1, 2):
        ds = photo.PhototourismDataset(SCENE, "train", s)
        assert ds.img_ids == listed
        out[f"img_ids_s{s}"] = np.asarray(ds.img_ids, dtype=np.int64)
        out[f"Ks_s{s}"] = np.stack([ds.Ks[ds.image_to_cam[i]] for i in ds.img_ids])
        out[f"poses_s{s}"] = ds.poses
        out[f"nears_s{s}"] = np.array([ds.nears[i] for i in ds.img_ids])
        out[f"fars_s{s}"] = np.array([ds.fars[i] for i in ds.img_ids])
        out[f"xyz_world_s{s}"] = ds.xyz_world
        scale = np.float32(max(fars.values())) / 5
        assert np.float32(out[f"fars_s{s}"].max()) == np.float32(max(fars.values()) / scale)
        out[f"scale_s{s}"] = np.asarray(scale)
        out[f"img_ids_train_s{s}"] = np.asarray(ds.img_ids_train, dtype=np.int64)
        out[f"img_ids_test_s{s}"] = np.asarray(ds.img_ids_test, dtype=np.int64)
        out[f"all_rays_s{s}"], out[f"all_rgbs_s{s}"] = _np(ds.all_rays), _np(ds.all_rgbs)
        assert set(ds.img_ids_test) == test_ids and len(ds.img_ids_train) == 4
    ds = photo.PhototourismDataset(SCENE, "test_train", 2)
    for k in range(len(ds)):
        sample = ds[k]
        for key in ("rays", "rgbs", "ts", "img_wh"):
            out[f"tt{k}_{key}"] = _np(sample[key])
    np.savez_compressed(os.path.join(HERE, "g24_photo.npz"), **out)
    total = 0
    for d, _, files in os.walk(SCENE):
        for name in files:
            size = os.path.getsize(os.path.join(d, name))
            assert size < 100_000, name
            total += size
    assert total < 300_000
    print("data_photo", total, "bytes; g24_photo.npz", os.path.getsize(os.path.join(HERE, "g24_photo.npz")), "bytes; scale",
          float(out["scale_s1"]), "test ids", sorted(test_ids))


if __name__ == "__main__":
    main()
