#!/usr/bin/env python3
"""Generate the fixtures of nerf_fl_amd.data (tests/test_data_cpu.py, tests/test_data_gpu.py) by running the REAL
reference's datasets/ray_utils.py and datasets/blender.py, loaded by file path.

Two of their imports are not installed here and are replaced by stub modules (our own code, below):
  kornia.create_meshgrid(H, W, normalized_coordinates=False) -> (1, H, W, 2) fp32 pixel grid, [..., 0] = x, [..., 1] = y;
  torchvision.transforms.ToTensor()                          -> PIL image -> (C, H, W) fp32 = uint8 / 255.

Written under tests/golden/:
  data_blender/                 a Blender-format scene of three 800 x 800 RGBA frames (flat blocks, so a PNG is a few KB;
                                alpha takes values strictly between 0 and 255; the occluder rectangles at 200 .. 600 px
                                land inside), transforms_train.json
  data_blender/small/           the same with three 24 x 24 frames of noise
  g23_data_small.npz            BlenderDataset(small, img_wh=(24, 24)) with [] and ['color', 'occ']: all_rays, all_rgbs in full
  g23_data_big.npz              BlenderDataset(data_blender, img_wh=(800, 800), ['color', 'occ']): every STRIDE-th row of
                                all_rays / all_rgbs and the row indices, K, and the uint8 pixels add_perturbation returns
  g23_data_photo.npz            three RGB images of different sizes, intrinsics, bounds and ids: the training rows
                                phototourism.py:169-180 builds (camera-frame direction, near, far, id; colours) and the
                                world rows of phototourism.py:229-236 (get_rays), from the real get_ray_directions

Runs only where the reference checkout is; the GPU machine sees the files alone.
Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_data_golden.py [path/to/reference]
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
SCENE = os.path.join(HERE, "data_blender")
STRIDE = 997


# ---- stubs (stand in for kornia.create_meshgrid and torchvision.transforms.ToTensor) ----------------------------
def create_meshgrid(height, width, normalized_coordinates=True):
    assert not normalized_coordinates
    ys, xs = torch.meshgrid(torch.arange(height, dtype=torch.float32), torch.arange(width, dtype=torch.float32),
                            indexing="ij")
    return torch.stack([xs, ys], -1)[None]


class ToTensor:
    def __call__(self, pic):
        a = np.array(pic)
        if a.ndim == 2:
            a = a[:, :, None]
        return torch.from_numpy(a).permute(2, 0, 1).contiguous().to(torch.float32).div(255)


def _install_stubs():
    kornia = types.ModuleType("kornia")
    kornia.create_meshgrid = create_meshgrid
    tv, tr = types.ModuleType("torchvision"), types.ModuleType("torchvision.transforms")
    tr.ToTensor = ToTensor
    tv.transforms = tr
    sys.modules.update({"kornia": kornia, "torchvision": tv, "torchvision.transforms": tr})


def _load_reference():
    pkg = types.ModuleType("datasets")
    pkg.__path__ = [os.path.join(REF, "datasets")]
    sys.modules["datasets"] = pkg
    mods = {}
    for name in ("ray_utils", "blender"):
        spec = importlib.util.spec_from_file_location(f"datasets.{name}", os.path.join(REF, "datasets", f"{name}.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[f"datasets.{name}"] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods["ray_utils"], mods["blender"]


# ---- the scene --------------------------------------------------------------------------------------------------
def _pose(rng):
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    q *= np.sign(np.linalg.det(q))
    m = np.eye(4)
    m[:3, :3] = q
    m[:3, 3] = 4.0 * rng.standard_normal(3) / np.sqrt(3)
    return m


def _write_scene(root, size, n_frames, block, seed):
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "train"), exist_ok=True)
    frames = []
    for t in range(n_frames):
        nb = size // block
        cells = rng.integers(0, 256, (nb, nb, 4), dtype=np.uint8)
        cells[..., 3] = rng.choice(np.array([0, 1, 37, 128, 200, 254, 255], dtype=np.uint8), (nb, nb))
        img = np.repeat(np.repeat(cells, block, 0), block, 1)
        Image.fromarray(img, "RGBA").save(os.path.join(root, "train", f"r_{t}.png"), optimize=True)
        frames.append({"file_path": f"./train/r_{t}", "transform_matrix": _pose(rng).tolist()})
    with open(os.path.join(root, "transforms_train.json"), "w") as f:
        json.dump({"camera_angle_x": 0.6911112070083618, "frames": frames}, f, indent=1)


def _np(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def main():
    _install_stubs()
    ray_utils, blender = _load_reference()
    _write_scene(SCENE, 800, 3, 100, 23)
    _write_scene(os.path.join(SCENE, "small"), 24, 3, 1, 24)

    out = {}
    for tag, pert in (("plain", []), ("pert", ["color", "occ"])):
        ds = blender.BlenderDataset(os.path.join(SCENE, "small"), "train", (24, 24), pert)
        out[f"rays_{tag}"], out[f"rgbs_{tag}"] = _np(ds.all_rays), _np(ds.all_rgbs)
        out["K"] = ds.K
    np.savez_compressed(os.path.join(HERE, "g23_data_small.npz"), **out)

    ds = blender.BlenderDataset(SCENE, "train", (800, 800), ["color", "occ"])
    rows = np.arange(0, len(ds.all_rays), STRIDE, dtype=np.int64)
    meta = json.load(open(os.path.join(SCENE, "transforms_train.json")))
    pixels = []
    for t, frame in enumerate(meta["frames"]):
        img = Image.open(os.path.join(SCENE, f"{frame['file_path']}.png"))
        if t != 0:
            img = blender.add_perturbation(img, ["color", "occ"], t)
        pixels.append(np.array(img))
    np.savez_compressed(os.path.join(HERE, "g23_data_big.npz"), rows=rows, rays=_np(ds.all_rays)[rows],
                        rgbs=_np(ds.all_rgbs)[rows], K=ds.K, pixels=np.stack(pixels))

    # Phototourism-style rows: unequal sizes, one intrinsic matrix per image (fp64, as the reference's self.Ks), RGB
    rng = np.random.default_rng(25)
    sizes = [(17, 23), (30, 12), (8, 41)]                       # (h, w)
    ids, nears, fars = [7, 1203, 42], [0.31, 1.7, 0.05], [4.2, 9.9, 31.0]
    out = dict(ids=np.asarray(ids, dtype=np.int64), near=np.asarray(nears), far=np.asarray(fars), sizes=np.asarray(sizes))
    Ks, c2ws, cam_rows, world_rows, rgbs = [], [], [], [], []
    transform = ToTensor()
    for i, (h, w) in enumerate(sizes):
        K = np.array([[w * (0.9 + 0.3 * rng.random()), 0, w / 2 + rng.random()],
                      [0, h * (1.1 + 0.3 * rng.random()), h / 2 - rng.random()], [0, 0, 1]])
        img8 = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out[f"image{i}"] = img8
        img = transform(Image.fromarray(img8, "RGB"))
        rgbs.append(img.view(3, -1).permute(1, 0))                               # phototourism.py:169-171
        directions = ray_utils.get_ray_directions(h, w, K)                       # phototourism.py:173
        d = directions.view(-1, 3)
        rays_t = ids[i] * torch.ones(len(d), 1)
        cam_rows.append(torch.cat([d, nears[i] * torch.ones_like(d[:, :1]), fars[i] * torch.ones_like(d[:, :1]),
                                   rays_t], 1))                                  # phototourism.py:175-180
        c2w = torch.FloatTensor(_pose(rng)[:3])
        rays_o, rays_d = ray_utils.get_rays(directions, c2w)                     # phototourism.py:230
        world_rows.append(torch.cat([rays_o, rays_d, nears[i] * torch.ones_like(rays_o[:, :1]),
                                     fars[i] * torch.ones_like(rays_o[:, :1])], 1))
        Ks.append(K)
        c2ws.append(_np(c2w))
    out.update(K=np.stack(Ks), c2w=np.stack(c2ws), cam_rows=_np(torch.cat(cam_rows)), world_rows=_np(torch.cat(world_rows)),
               rgbs=_np(torch.cat(rgbs)))
    np.savez_compressed(os.path.join(HERE, "g23_data_photo.npz"), **out)
    for name in ("g23_data_small.npz", "g23_data_big.npz", "g23_data_photo.npz"):
        print(name, os.path.getsize(os.path.join(HERE, name)), "bytes")


if __name__ == "__main__":
    main()
