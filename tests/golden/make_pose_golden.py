#!/usr/bin/env python3
"""Generate tests/golden/g20_pose_rays.npz by running the REAL reference's pose path: models/poses.py (LearnPose) and
utils/lie_group_helper.py (make_c2w / Exp), one `learn_poses(i)` call per camera and one c2w per ray, as train.py:86-98
does.  datasets/ray_utils.get_rays needs kornia at import time, so its four lines are restated here (rotate the camera
direction by c2w[:, :3], normalise, origin = c2w[:, 3]; ray_utils.py:29-55).

Runs only in the build container (needs the reference checkout); the GPU box only sees the .npz.  Stored: the inputs
(r, t, init_c2w, the image id -> pose row table, camera-frame rays, image ids, a seeded g_rays) and, with and without
init_c2w, the world rays in fp32 (the reference's precision) and the (r, t) gradients of sum(rays * g_rays) in fp32 and
in fp64 (the same reference code on .double() parameters).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_pose_golden.py [path/to/reference]
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True
REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


# the reference's utils/__init__.py pulls in packages the pose helper does not need: register its lie_group_helper
# under the name models/poses.py imports it by, then load models/poses.py by path
sys.modules.setdefault("utils", types.ModuleType("utils"))
lie = _load("utils.lie_group_helper", os.path.join(REF, "utils", "lie_group_helper.py"))
ref_poses = _load("ref_models_poses", os.path.join(REF, "models", "poses.py"))

N_CAMS, N_RAYS = 40, 704
# pose rows by |r| class: exactly 0, ~1e-3, ~1e-2, up to ~1.5 rad; the last row has no ray in the batch
CLASSES = {"zero": range(0, 10), "1e-3": range(10, 20), "1e-2": range(20, 30), "large": range(30, 40)}
ABSENT_ROW = 39


def get_rays(directions, c2w):
    """datasets/ray_utils.py:29-55, restated (the module imports kornia)."""
    rays_d = directions.view(-1, 1, 1, 3) @ torch.transpose(c2w[..., :3], 1, 2).view(-1, 1, 3, 3)
    rays_d = rays_d.view(-1, 3)
    rays_d = rays_d / torch.norm(rays_d, dim=-1, keepdim=True)
    rays_o = c2w[:, :, 3].expand(rays_d.shape)
    return rays_o, rays_d


def reference_rays(r, t, init, image_ids, rays_cam, ts, g_rays, dtype):
    learn = ref_poses.LearnPose(N_CAMS, True, True, init_c2w=None if init is None else init.clone())
    with torch.no_grad():
        learn.r.copy_(r)
        learn.t.copy_(t)
    learn = learn.to(dtype)
    poses = {img_id: learn(i) for i, img_id in enumerate(image_ids)}       # train.py:84
    c2ws = torch.stack([poses[int(i)] for i in ts])[:, :3]                 # train.py:92
    rays_o, rays_d = get_rays(rays_cam[:, :3].to(dtype), c2ws)
    rays = torch.cat([rays_o, rays_d, rays_cam[:, 3:5].to(dtype)], 1)      # train.py:95
    (rays * g_rays.to(dtype)).sum().backward()
    return rays.detach(), learn.r.grad.detach(), learn.t.grad.detach()


def main():
    g = torch.Generator().manual_seed(20)
    r = torch.zeros(N_CAMS, 3)
    for name, rows in CLASSES.items():
        if name == "zero":
            continue
        axis = torch.randn(len(rows), 3, generator=g)
        axis = axis / axis.norm(dim=-1, keepdim=True)
        mag = {"1e-3": 1e-3 * (0.5 + torch.rand(len(rows), generator=g)),
               "1e-2": 1e-2 * (0.5 + torch.rand(len(rows), generator=g)),
               "large": 0.05 + 1.45 * torch.rand(len(rows), generator=g)}[name]
        r[list(rows)] = axis * mag[:, None]
    t = 0.05 * torch.randn(N_CAMS, 3, generator=g)
    # initial poses: random rotations (QR of a Gaussian) and camera centres ~4 from the origin
    q, _ = torch.linalg.qr(torch.randn(N_CAMS, 3, 3, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.linalg.det(q))[:, None, None]
    init = torch.eye(4).repeat(N_CAMS, 1, 1)
    init[:, :3, :3] = q.float()
    init[:, :3, 3] = 4.0 * torch.randn(N_CAMS, 3, generator=g) / np.sqrt(3)
    # image ids: sparse and not in row order (poses_dict keys of a phototourism split)
    image_ids = (torch.randperm(3 * N_CAMS, generator=g)[:N_CAMS] + 1).tolist()
    row_of_id = np.full(max(image_ids) + 1, -1, dtype=np.int64)
    for i, img in enumerate(image_ids):
        row_of_id[img] = i
    rows = torch.randint(0, N_CAMS - 1, (N_RAYS,), generator=g)            # interleaved; ABSENT_ROW never drawn
    assert ABSENT_ROW == N_CAMS - 1 and not (rows == ABSENT_ROW).any()
    ts = torch.tensor([image_ids[k] for k in rows.tolist()], dtype=torch.int64)
    # camera-frame directions of pixels of a 400 x 300 image (get_ray_directions: no half-pixel), near, far, one extra
    # column (the training layout may carry more; nfl_pose_rays reads the first five)
    px, py = torch.randint(0, 400, (N_RAYS,), generator=g).float(), torch.randint(0, 300, (N_RAYS,), generator=g).float()
    f, cx, cy = 350.0, 200.0, 150.0
    rays_cam = torch.stack([(px - cx) / f, -(py - cy) / f, -torch.ones(N_RAYS), 0.5 + torch.rand(N_RAYS, generator=g),
                            6.0 + torch.rand(N_RAYS, generator=g), torch.randn(N_RAYS, generator=g)], 1)
    g_rays = torch.randn(N_RAYS, 8, generator=g)

    out = dict(r=r, t=t, init_c2w=init, image_ids=np.asarray(image_ids, dtype=np.int64), row_of_id=row_of_id,
               rays_cam=rays_cam, ts=ts, g_rays=g_rays)
    for tag, ini in (("init", init), ("noinit", None)):
        rays32, gr32, gt32 = reference_rays(r, t, ini, image_ids, rays_cam, ts, g_rays, torch.float32)
        _, gr64, gt64 = reference_rays(r, t, ini, image_ids, rays_cam, ts, g_rays, torch.float64)
        assert gr64[ABSENT_ROW].abs().max() == 0 and gt64[ABSENT_ROW].abs().max() == 0
        out.update({f"rays_{tag}": rays32, f"g_r32_{tag}": gr32, f"g_t32_{tag}": gt32,
                    f"g_r64_{tag}": gr64, f"g_t64_{tag}": gt64})
    cfg = {"n_cams": N_CAMS, "n_rays": N_RAYS, "absent_row": ABSENT_ROW,
           "classes": {k: [v.start, v.stop] for k, v in CLASSES.items()}}
    arrays = {k: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    np.savez_compressed(os.path.join(HERE, "g20_pose_rays.npz"), cfg=json.dumps(cfg), **arrays)
    print(f"wrote g20_pose_rays.npz  ({len(arrays)} arrays)")


if __name__ == "__main__":
    main()
