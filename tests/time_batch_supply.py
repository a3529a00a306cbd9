#!/usr/bin/env python3
"""What supplying one training batch costs: the tensor path of RayTrainer.fit_epoch(rays, rgbs, ts) with use_graph=True
(perm[i:i+bs], three index gathers, GraphedTrainStep.load's three copies) against ImageBank.gather(out=...) (one
launch), on a bank of `--images` 800 x 800 RGBA images.  Not a test: prints one JSON record (and writes it to --out).

Both variants fill the same static buffers.  They alternate in one process, iteration by iteration, with the tensor
path run twice per iteration (A, A'): the difference of the medians of A and A' is the spread a difference between A and
the bank path has to exceed to mean anything.  Each iteration is bracketed by device events (the span the stream was
busy or waiting for the host to launch) and by a host clock (the time the host spent issuing it); medians over
`--iters` iterations after `--warmup`."""
import argparse
import json
import os
import statistics
import sys
import time
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--rays", type=int, nargs="+", default=[1024, 4096])
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from nerf_fl_amd import data
    from nerf_fl_amd.train import GraphedTrainStep
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (a.size, a.size, 4), dtype=np.uint8) for _ in range(a.images)]
    c2w = np.tile(np.eye(4)[None, :3], (a.images, 1, 1))
    c2w[:, :, 3] = rng.standard_normal((a.images, 3))
    K = np.array([[1111.0, 0, a.size / 2], [0, 1111.0, a.size / 2], [0, 0, 1]])
    bank = data.ImageBank(imgs, c2w, K, 2.0, 6.0, device=dev)
    del imgs
    n = bank.n_pixels
    rays, rgbs, ts = bank.materialise()
    perm = torch.randperm(n, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    key = data.epoch_key(0, 0)
    rec = dict(images=a.images, size=a.size, n_pixels=n, bank_bytes=bank.nbytes,
               tensor_path_bytes=rays.numel() * 4 + rgbs.numel() * 4 + ts.numel() * 8 + perm.numel() * 8,
               warmup=a.warmup, iters=a.iters, device=torch.cuda.get_device_name(0), unit="us", cases=[])
    for bs in a.rays:
        buf = types.SimpleNamespace(rays=torch.empty(bs, 8, device=dev), ts=torch.empty(bs, dtype=torch.int64, device=dev),
                                    target=torch.empty(bs, 3, device=dev))

        def tensor_path(i):
            idx = perm[i:i + bs]
            GraphedTrainStep.load(buf, rays[idx], ts[idx], rgbs[idx])

        def bank_path(i):
            bank.gather(i, bs, key, "world", out=(buf.rays, buf.target, buf.ts))

        variants = (("tensor", tensor_path), ("tensor_again", tensor_path), ("bank", bank_path))
        dev_t, host_t = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
        events = []
        for it in range(a.warmup + a.iters):
            i = (it * bs) % (n - bs)
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                fn(i)
                e1.record()
                t1 = time.perf_counter()
                if it >= a.warmup:
                    events.append((name, e0, e1))
                    host_t[name].append((t1 - t0) * 1e6)
            if it % 16 == 15:
                torch.cuda.synchronize()         # keep the host from running far ahead of the device
        torch.cuda.synchronize()
        for name, e0, e1 in events:
            dev_t[name].append(e0.elapsed_time(e1) * 1e3)
        med = lambda d: {k: round(statistics.median(v), 2) for k, v in d.items()}
        md, mh = med(dev_t), med(host_t)
        case = dict(rays=bs, device_us=md, host_us=mh,
                    device_spread_us=round(abs(md["tensor"] - md["tensor_again"]), 2),
                    host_spread_us=round(abs(mh["tensor"] - mh["tensor_again"]), 2))
        case["bank_not_slower"] = bool(md["bank"] <= md["tensor"] + case["device_spread_us"]
                                       and mh["bank"] <= mh["tensor"] + case["host_spread_us"])
        rec["cases"].append(case)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
