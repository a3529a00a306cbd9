#!/usr/bin/env python3
"""What scoring one rendered image costs: the route the package offered before nerf_fl_amd.metrics (ImageBank.frame(i),
then the PSNR expression and the torch restatement of the SSIM on the device; tests/metrics_util.py) against
metrics.image_metrics in bank form (two launches that read the uint8 image where it lies).  Not a test: prints one JSON
record (and writes it to --out).

The routes alternate in one process, iteration by iteration, with the old route run twice per iteration (A, A'): the
difference of the medians of A and A' is the spread a difference between A and B has to exceed to mean anything.  Each
iteration is bracketed by device events and by a host clock; medians over `--iters` iterations after `--warmup`.  Neither
route synchronises inside an iteration.  Peak device memory above the resident state is taken per route in a pass of
its own."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[800, 24])
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import metrics_util as mu
    from nerf_fl_amd import data, metrics
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    rec = dict(images=a.images, warmup=a.warmup, iters=a.iters, device=torch.cuda.get_device_name(0), unit="us", cases=[])
    for size in a.sizes:
        imgs = [rng.integers(0, 256, (size, size, 4), dtype=np.uint8) for _ in range(a.images)]
        c2w = np.tile(np.eye(4)[None, :3], (a.images, 1, 1))
        K = np.array([[1111.0, 0, size / 2], [0, 1111.0, size / 2], [0, 0, 1]])
        bank = data.ImageBank(imgs, c2w, K, 2.0, 6.0, device=dev)
        del imgs
        pred = torch.rand(size * size, 3, device=dev)
        table = torch.zeros(a.images, 8, dtype=torch.float64, device=dev)
        old_out = torch.zeros(a.images, 2, dtype=torch.float64, device=dev)

        def old_route(i):
            _, rgbs, _ = bank.frame(i)
            p = pred.clamp(0.0, 1.0)
            old_out[i, 0] = -10.0 * torch.log10(((p - rgbs) ** 2).mean())
            old_out[i, 1] = mu.ssim_map(p.view(size, size, 3), rgbs.view(size, size, 3), torch.float32).mean()

        def new_route(i):
            metrics.image_metrics(pred, size, size, bank=bank, image=i, table=table, slot=i)

        variants = (("old", old_route), ("old_again", old_route), ("metrics", new_route))
        dev_t, host_t = {k: [] for k, _ in variants}, {k: [] for k, _ in variants}
        events = []
        for it in range(a.warmup + a.iters):
            i = it % a.images
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
        peaks = {}
        for name, fn in (("old", old_route), ("metrics", new_route)):
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            fn(0)
            torch.cuda.synchronize()
            peaks[name] = torch.cuda.max_memory_allocated() - base
        agree = dict(psnr=abs(old_out[0, 0].item() - table[0, 5].item()), ssim=abs(old_out[0, 1].item() - table[0, 7].item()))
        rec["cases"].append(dict(size=size, device_us=md, host_us=mh,
                                 device_spread_us=round(abs(md["old"] - md["old_again"]), 2),
                                 host_spread_us=round(abs(mh["old"] - mh["old_again"]), 2),
                                 peak_bytes=peaks, routes_differ_by=agree))
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
