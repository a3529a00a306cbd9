"""The two timers of the geometry timing scripts (time_geometry.py, time_mesh.py, time_occupancy.py, time_simplify.py)."""
import statistics
import time

import torch


def _summary(ms):
    return {"median": statistics.median(ms), "min": min(ms), "max": max(ms)}


def timed(fn, warmup, iters):
    """Milliseconds per call of `fn` between two stream events: what the device spends, launches included."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return _summary(ms)


def host_timed(fn, warmup, iters):
    """Milliseconds per call of `fn` on the host's clock, the device idle before and after: for calls that synchronise.
    `warmup` is explicit at every call site: time_mesh.py passes 0, as the numbers of DESIGN.md section 19 were taken."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return _summary(ms)
