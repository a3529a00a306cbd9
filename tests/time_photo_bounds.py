#!/usr/bin/env python3
"""What the per-image depth bounds of a Phototourism scene cost: data.depth_bounds (one launch of nfl_depth_bounds) against
the reference's loop (datasets/phototourism.py:127-131, restated below in numpy: one fp64 matmul, one filter and two
np.percentile calls per image) on the same synthetic scene, by default 1 400 images x 130 000 points (Brandenburg Gate's
order of size).  Not a test: prints one JSON record (and writes it to --out).

The device call is bracketed by device events, `--iters` calls after `--warmup`, median and spread; the point list and
the matrices are on the device before the window (as they are once per scene), and nothing synchronises inside it.  The
numpy loop runs once in full, under a host clock, on the threads the process is given (OMP_NUM_THREADS).  The results
of the two are compared at the size timed.  A point evaluation is one (image, point) depth of one pass; the kernel makes
8 passes, so it evaluates 8 N P depths where the loop evaluates N P.  The bytes are those the loads ask for (24 per
evaluation); the caches serve them, so their rate is no memory bandwidth."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
PASSES = 8


def scene(n_img, n_pts, seed):
    rng = np.random.default_rng(seed)
    xyz = rng.standard_normal((n_pts, 3)) * np.array([30.0, 10.0, 30.0])
    w2c = np.tile(np.eye(4), (n_img, 1, 1))
    for i in range(n_img):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        w2c[i, :3, :3] = q * np.sign(np.linalg.det(q))
        w2c[i, :3, 3] = 10.0 * rng.standard_normal(3)          # inside the cloud
    return xyz, w2c


def numpy_loop(xyz, w2c):
    """phototourism.py:124-131."""
    xyz_world_h = np.concatenate([xyz, np.ones((len(xyz), 1))], -1)
    nears, fars = np.empty(len(w2c)), np.empty(len(w2c))
    for i in range(len(w2c)):
        xyz_cam_i = (xyz_world_h @ w2c[i].T)[:, :3]
        xyz_cam_i = xyz_cam_i[xyz_cam_i[:, 2] > 0]
        nears[i] = np.percentile(xyz_cam_i[:, 2], 0.1)
        fars[i] = np.percentile(xyz_cam_i[:, 2], 99.9)
    return nears, fars


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1400)
    ap.add_argument("--points", type=int, default=130_000)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerf_fl_amd import data
    if not torch.cuda.is_available():
        raise SystemExit("time_photo_bounds.py measures on the MI355X: no device found")
    dev = torch.device("cuda:0")
    xyz, w2c = scene(a.images, a.points, 17)
    d_xyz, d_w2c = torch.from_numpy(xyz).to(dev), torch.from_numpy(w2c).to(dev)
    q = (0.1 / 100, 99.9 / 100)
    for _ in range(a.warmup):
        near, far, count = data.depth_bounds(d_xyz, d_w2c, q)
    torch.cuda.synchronize()
    events = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.iters)]
    for e0, e1 in events:
        e0.record()
        near, far, count = data.depth_bounds(d_xyz, d_w2c, q)
        e1.record()
    torch.cuda.synchronize()
    ms = sorted(e0.elapsed_time(e1) for e0, e1 in events)
    t0 = time.perf_counter()
    nears, fars = numpy_loop(xyz, w2c)
    numpy_s = time.perf_counter() - t0
    depth_max = float(np.abs(np.concatenate([xyz, np.ones((len(xyz), 1))], -1) @ w2c[:, 2, :].T).max())
    err = max(np.abs(near.cpu().numpy() - nears).max(), np.abs(far.cpu().numpy() - fars).max())
    med = statistics.median(ms)
    rec = dict(images=a.images, points=a.points, warmup=a.warmup, iters=a.iters, device=torch.cuda.get_device_name(0),
               host_threads=int(os.environ.get("OMP_NUM_THREADS", "0")) or None,
               device_ms=dict(median=round(med, 4), min=round(ms[0], 4), max=round(ms[-1], 4)),
               numpy_loop_s=round(numpy_s, 3), speedup=round(numpy_s * 1e3 / med, 1),
               passes=PASSES,
               point_evaluations_per_s=PASSES * a.images * a.points / (med * 1e-3),
               image_points_per_s=a.images * a.points / (med * 1e-3),
               bytes_requested_per_call=PASSES * a.images * a.points * 24,
               requested_read_rate_GBps=round(PASSES * a.images * a.points * 24 / (med * 1e-3) / 1e9, 1),
               max_abs_difference=float(err), max_abs_depth=depth_max)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
