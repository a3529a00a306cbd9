#!/usr/bin/env python3
"""Generate tests/golden/g21_lr_schedules.npz from the REAL reference's warm-up scheduler: utils/warmup_scheduler.py,
loaded by file path (the package's utils/__init__.py imports torch_optimizer and cv2), driven with torch's MultiStepLR
and CosineAnnealingLR exactly as get_scheduler (utils/__init__.py:44-61) composes them, and stepped once per epoch as
Lightning does.

Stored, for every optimizer in {sgd, adam}, scheduler in {steplr, cosine}, warmup_epochs in {0, 3} and
warmup_multiplier in {1, 2}: the learning rate of each of NUM_EPOCHS epochs under key "<opt>_<sched>_w<T>_m<M>", plus
the settings and the torch version that produced them.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sched_golden.py path/to/reference
"""
import importlib.util
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.dont_write_bytecode = True

LR, NUM_EPOCHS, DECAY_STEP, DECAY_GAMMA = 5e-4, 20, [4, 10], 0.1


def _load(path):
    spec = importlib.util.spec_from_file_location("ref_warmup_scheduler", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def schedule(warmup_mod, opt_name, sched_name, warmup_epochs, multiplier):
    p = torch.nn.Parameter(torch.zeros(3))
    opt = (torch.optim.SGD([p], lr=LR, momentum=0.9) if opt_name == "sgd" else torch.optim.Adam([p], lr=LR, eps=1e-8))
    if sched_name == "steplr":
        sched = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=DECAY_STEP, gamma=DECAY_GAMMA)
    else:
        sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=NUM_EPOCHS, eta_min=1e-8)
    if warmup_epochs > 0 and opt_name not in ["radam", "ranger"]:
        sched = warmup_mod.GradualWarmupScheduler(opt, multiplier=multiplier, total_epoch=warmup_epochs,
                                                  after_scheduler=sched)
    lrs = []
    for _ in range(NUM_EPOCHS):
        lrs.append(opt.param_groups[0]["lr"])
        sched.step()
    return np.array(lrs, dtype=np.float64)


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    mod = _load(os.path.join(sys.argv[1], "utils", "warmup_scheduler.py"))
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")       # lr_scheduler.step() before optimizer.step(), get_lr() outside step()
        for o in ("sgd", "adam"):
            for s in ("steplr", "cosine"):
                for w in (0, 3):
                    for m in (1, 2):
                        out[f"{o}_{s}_w{w}_m{m}"] = schedule(mod, o, s, w, m)
    meta = dict(lr=LR, num_epochs=NUM_EPOCHS, decay_step=DECAY_STEP, decay_gamma=DECAY_GAMMA, torch=torch.__version__)
    out["meta"] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, "g21_lr_schedules.npz")
    np.savez(path, **out)
    print(f"wrote {path}: {len(out) - 1} schedules, torch {torch.__version__}")


if __name__ == "__main__":
    main()
