#!/usr/bin/env python3
"""What nfl_tsdf_fuse costs on one MI355X (nerf_fl_amd.fusion.fuse_depth).  Not a test: prints one JSON
record (and writes it to --out).

    fuse     nfl_tsdf_fuse alone, through the C ABI: a 256^3 lattice over [-1.2, 1.2]^3, trunc = 3 spacings, one run of 32
             cameras of 800 x 800 on a Fibonacci sphere of radius 3 looking at the origin, their depth maps
             geometry.mesh_depth's of a ball of radius 0.8 (so the maps hold what a scene's do: a silhouette, +inf around
             it), pixel weights 1 (NULL) and present
    resolve  nfl_tsdf_resolve on the result

Kernel figures are medians over `--iters` calls after `--warmup`, each bracketed by device events, and the mean of `--iters`
calls between ONE pair of events.  The floor beside the fuse is its accumulator traffic: 12 B read and 12 B written per
lattice point and run, the bytes the definition needs whatever the images hold."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import timed  # noqa: E402
import meshcolor_ref as mref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=256)
    ap.add_argument("--frame", type=int, default=800)
    ap.add_argument("--images", type=int, default=32)
    ap.add_argument("--ball", type=int, default=65, help="lattice size the ball mesh is extracted on")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_tsdf.py measures on the GPU; there is none here")
    from nerf_fl_amd import _lib, fusion, geometry
    from nerf_fl_amd.data import ImageBank
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters}

    # ---- the scene: a ball, and cameras all round it
    c = torch.linspace(-1.0, 1.0, a.ball, device=dev, dtype=torch.float64)
    lat = (0.8 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()
    ball = geometry.extract_surface(lat, 0.0, (-1.0,) * 3, (1.0,) * 3)
    S, N = a.frame, a.images
    golden = math.pi * (3.0 - math.sqrt(5.0))
    eyes = []
    for k in range(N):
        z = 1.0 - 2.0 * (k + 0.5) / N
        r = math.sqrt(1.0 - z * z)
        eyes.append((3.0 * r * math.cos(golden * k), 3.0 * r * math.sin(golden * k), 3.0 * z))
    # the frame holds the box: its near face is 1.8 away and 1.2 wide each way
    K = np.array([[0.7 * (S - 1), 0, (S - 1) / 2], [0, 0.7 * (S - 1), (S - 1) / 2], [0, 0, 1]])
    image = np.zeros((S, S, 3), dtype=np.uint8)
    bank = ImageBank([image] * N, np.stack([mref.look_at(e) for e in eyes]), K, 1.0, 5.0, device=dev)
    depth = torch.stack([geometry.mesh_depth(ball, bank=bank, image=i) for i in range(N)]).view(-1)
    weights = torch.rand(depth.shape, device=dev) * 0.5 + 0.5
    rec["scene"] = {"images": N, "frame": [S, S], "depth_words": depth.numel(), "covered": torch.isfinite(depth).float().mean().item(),
                    "ball_triangles": ball["triangles"].shape[0]}

    # ---- fuse
    n = a.points
    P = n ** 3
    lo, sp = -1.2, 2.4 / (n - 1)
    acc = torch.empty(P, 2, dtype=torch.float32, device=dev)
    views = torch.empty(P, dtype=torch.int32, device=dev)
    f = _lib.TsdfFuseArgs()
    f.d_table, f.n_images, f.first, f.count, f.start = bank.table.data_ptr(), N, 0, N, 1
    f.d_depth, f.n_depth = depth.data_ptr(), depth.numel()
    f.nx, f.ny, f.nz, f.trunc = n, n, n, 3.0 * sp
    f.lo[:], f.spacing[:] = (lo,) * 3, (sp,) * 3
    f.d_acc, f.d_views = acc.data_ptr(), views.data_ptr()
    fuse = lambda: _lib.check(lib.nfl_tsdf_fuse(C.byref(f), stream()), "fuse")

    def batch(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.iters):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.iters

    floor_bytes = 24 * P
    for name, pw in (("fuse", None), ("fuse_pixel_weights", weights)):
        f.d_pixel_weights = None if pw is None else pw.data_ptr()
        t = timed(fuse, a.warmup, a.iters)
        pairs = int(views.sum(dtype=torch.int64).item())
        rec[name] = {"lattice": [n, n, n], "ms": t, "ms_mean_of_a_batch": batch(fuse), "point_image_pairs": P * N,
                     "contributing_pairs": pairs, "pairs_per_s": P * N / t["median"] * 1e3,
                     "accumulator_bytes": floor_bytes, "accumulator_GBps": floor_bytes / t["median"] / 1e6,
                     "floor_ms_at_6.29_TBps": floor_bytes / 6.29e12 * 1e3}
    # the Python wrapper gives the same bits
    out = fusion.fuse_depth(bank, depth, (lo,) * 3, (-lo,) * 3, (n, n, n), 3.0 * sp, pixel_weights=weights)
    rec["python_equal"] = bool(torch.equal(out["acc"].view(P, 2), acc) and torch.equal(out["views"].view(P), views))

    # ---- resolve
    lattice = torch.empty(P, dtype=torch.float32, device=dev)
    known = torch.empty(P, dtype=torch.uint8, device=dev)
    r = _lib.TsdfResolveArgs()
    r.d_acc, r.d_views, r.nx, r.ny, r.nz, r.min_views = acc.data_ptr(), views.data_ptr(), n, n, n, 1
    r.min_weight, r.fill, r.d_lattice, r.d_known = 0.5, -1.0, lattice.data_ptr(), known.data_ptr()
    t = timed(lambda: _lib.check(lib.nfl_tsdf_resolve(C.byref(r), stream()), "resolve"), a.warmup, a.iters)
    rec["resolve"] = {"ms": t, "bytes": 17 * P, "GBps": 17 * P / t["median"] / 1e6, "known": known.float().mean().item()}

    text = json.dumps(rec)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
