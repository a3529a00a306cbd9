#!/usr/bin/env python3
"""Generate tests/golden/g22_ref_param_order.json from the REAL reference: the order of the parameters its optimiser
holds, which is the index space of a Lightning checkpoint's `optimizer_states[0]`.

For every configuration below, the reference's own modules -- nn.Embedding for embedding_a / embedding_t,
models/nerf.py's NeRF for the coarse and fine fields, models/poses.py's LearnPose -- are put into models_to_train in
train.py's order (train.py:46-76, then :134-136 in setup()), and the reference's own get_parameters
(utils/__init__.py:11-22) lists them.  Stored per configuration: [checkpoint name, shape, requires_grad] of every
parameter in that order, plus the settings.  Names only, no values.

utils/__init__.py imports torch_optimizer and cv2 (through utils/visualization.py), and models/poses.py imports
utils/lie_group_helper.py; none of their code is used here, so the two missing packages are replaced by empty stand-ins.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_param_order_golden.py path/to/reference
"""
import importlib
import json
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

N_VOCAB, N_A, N_TAU, N_CAMS, N_EMB_XYZ, N_EMB_DIR = 100, 48, 16, 5, 10, 4
CONFIGS = {
    "base": dict(encode_a=False, encode_t=False, N_importance=64, refine_pose=False),
    "coarse_only": dict(encode_a=False, encode_t=False, N_importance=0, refine_pose=False),
    "nerf_a": dict(encode_a=True, encode_t=False, N_importance=64, refine_pose=False),
    "nerf_w": dict(encode_a=True, encode_t=True, N_importance=64, refine_pose=False),
    "refine_pose": dict(encode_a=False, encode_t=False, N_importance=64, refine_pose=True),
    "refine_pose_w": dict(encode_a=True, encode_t=True, N_importance=64, refine_pose=True),
}


def _reference(root):
    sys.path.insert(0, root)
    for name in ("torch_optimizer", "cv2"):
        if name not in sys.modules:
            try:
                importlib.import_module(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    vis = types.ModuleType("utils.visualization")
    vis.__all__ = []
    sys.modules["utils.visualization"] = vis
    utils = importlib.import_module("utils")
    nerf = importlib.import_module("models.nerf")
    poses = importlib.import_module("models.poses")
    return utils.get_parameters, nerf.NeRF, poses.LearnPose


def order(get_parameters, NeRF, LearnPose, cfg):
    named, models_to_train = {}, []
    if cfg["encode_a"]:
        named["embedding_a"] = torch.nn.Embedding(N_VOCAB, N_A)
        models_to_train.append(named["embedding_a"])
    if cfg["encode_t"]:
        named["embedding_t"] = torch.nn.Embedding(N_VOCAB, N_TAU)
        models_to_train.append(named["embedding_t"])
    cx, cd = 6 * N_EMB_XYZ + 3, 6 * N_EMB_DIR + 3
    models = {"coarse": NeRF("coarse", in_channels_xyz=cx, in_channels_dir=cd, refine_pose=cfg["refine_pose"])}
    named["nerf_coarse"] = models["coarse"]
    if cfg["N_importance"] > 0:
        models["fine"] = NeRF("fine", in_channels_xyz=cx, in_channels_dir=cd, encode_appearance=cfg["encode_a"],
                              in_channels_a=N_A, encode_transient=cfg["encode_t"], in_channels_t=N_TAU,
                              refine_pose=cfg["refine_pose"])
        named["nerf_fine"] = models["fine"]
    models_to_train.append(models)
    named["learn_poses"] = LearnPose(N_CAMS, cfg["refine_pose"], cfg["refine_pose"],
                                     init_c2w=torch.eye(4).repeat(N_CAMS, 1, 1))
    models_to_train.append(named["learn_poses"])
    name_of = {id(p): f"{prefix}.{n}" for prefix, m in named.items() for n, p in m.named_parameters()}
    return [[name_of[id(p)], list(p.shape), bool(p.requires_grad)] for p in get_parameters(models_to_train)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    get_parameters, NeRF, LearnPose = _reference(os.path.abspath(sys.argv[1]))
    out = {"settings": dict(N_vocab=N_VOCAB, N_a=N_A, N_tau=N_TAU, n_cams=N_CAMS, N_emb_xyz=N_EMB_XYZ,
                            N_emb_dir=N_EMB_DIR, torch=torch.__version__),
           "configs": {k: dict(cfg, params=order(get_parameters, NeRF, LearnPose, cfg)) for k, cfg in CONFIGS.items()}}
    path = os.path.join(HERE, "g22_ref_param_order.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    counts = ", ".join(f"{k} {len(v['params'])}" for k, v in out["configs"].items())
    print(f"wrote {path}: {counts} parameters")


if __name__ == "__main__":
    main()
