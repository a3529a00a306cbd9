#!/usr/bin/env python3
"""What empty-space skipping costs and saves on one MI355X (geometry.occupancy_grid / clip_rays, eval.clipped_inference).
Not a test: prints one JSON record (and writes it to --out).

    build    nfl_occ_build on a ball lattice (default 257^3 points = 256^3 cells), dilate 1, through the C ABI
    clip     nfl_occ_clip_rays on the rays of an 800 x 800 frame through that grid
    frame    eval.render_frame at 800 x 800, 64 + 128 samples, base coarse + fine fields, with and without `occupancy`
             (the ball grid: the hit share is geometry, the weights are seeded noise), under a host clock with a
             synchronisation either side, since the clipped path synchronises once itself
    psnr     the clipped frame against the full one on a grid built from density_lattice of the same fine field, at
             64 + 128 and at 32 + 64 inside the tightened bounds, for thresholds at a few quantiles of that lattice

Kernel figures are medians over `--iters` calls after `--warmup`, bracketed by device events.  The bytes are those the
algorithm needs, computed from the shapes: the build reads 4 B per lattice point once, writes four word arrays of about
one bit per point and reads three of them back; the clip reads 32 B and writes 9 B per ray, plus the words its walk
touches (not counted: they stay in L2)."""
import argparse
import ctypes as C
import json
import math
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import host_timed, timed  # noqa: E402


def psnr(a, b):
    mse = ((a - b) ** 2).mean().item()
    return -10.0 * math.log10(mse) if mse > 0 else float("inf")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--frame", type=int, default=800)
    ap.add_argument("--field", type=int, default=128, help="lattice size of the grid built from the field (psnr)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_occupancy.py measures on the GPU; there is none here")
    from nerf_fl_amd import NeRF, PosEmbedding, _lib, eval as nfl_eval, geometry, rendering, synth
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters}

    # ---- build: a ball of radius 1.2 over [-1.5, 1.5]^3
    n = a.cells + 1
    lo, hi = (-1.5,) * 3, (1.5,) * 3
    c = torch.linspace(-1.5, 1.5, n, device=dev, dtype=torch.float64)
    lat = (1.2 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()
    grid = geometry.occupancy_grid(lat, 0.0, lo, hi, dilate=1)
    sbytes = lib.nfl_occ_build_bytes(n, n, n, 1)
    scratch = torch.empty((sbytes + 7) // 8, dtype=torch.int64, device=dev)
    bits = torch.empty_like(grid.bits)
    ba = _lib.OccBuildArgs()
    ba.d_lattice, ba.nx, ba.ny, ba.nz, ba.threshold, ba.dilate = lat.data_ptr(), n, n, n, 0.0, 1
    ba.d_scratch, ba.scratch_bytes, ba.d_bits = scratch.data_ptr(), scratch.numel() * 8, bits.data_ptr()
    t_build = timed(lambda: _lib.check(lib.nfl_occ_build(C.byref(ba), stream()), "build"), a.warmup, a.iters)
    assert torch.equal(bits, grid.bits)
    wpx, wx = (n + 31) // 32, (a.cells + 31) // 32
    # flags: lattice in, P out; x: P in, X out; y: X in, Y out; z: Y in, bits out
    b_build = 4 * n ** 3 + 4 * (2 * n * n * wpx + 2 * n * n * wx + 2 * n * a.cells * wx + a.cells * a.cells * wx)
    rec["build"] = {"lattice": [n, n, n], "dilate": 1, "ms": t_build, "bytes": b_build, "grid_bytes": bits.numel() * 4,
                    "scratch_bytes": sbytes, "GBps": b_build / t_build["median"] / 1e6, "occupied": grid.fraction()}
    del lat, scratch

    # ---- clip: the rays of one frame
    S = a.frame
    c2w = torch.eye(4)[:3].clone()
    c2w[2, 3] = 4.0
    K = nfl_eval.fov60_intrinsics(S, S)
    rays = nfl_eval.frame_rays(c2w, K, S, S, 2.0, 6.0, dev)
    R = rays.shape[0]
    nf = torch.empty(R, 2, device=dev)
    hit = torch.empty(R, dtype=torch.uint8, device=dev)
    ca = _lib.OccClipArgs()
    ca.d_rays, ca.n_rays, ca.d_bits, ca.nx, ca.ny, ca.nz = rays.data_ptr(), R, grid.bits.data_ptr(), n, n, n
    for k in range(3):
        ca.lo[k], ca.spacing[k] = grid.lo[k], grid.spacing[k]
    ca.d_near_far, ca.d_hit = nf.data_ptr(), hit.data_ptr()
    t_clip = timed(lambda: _lib.check(lib.nfl_occ_clip_rays(C.byref(ca), stream()), "clip"), a.warmup, a.iters)
    share = hit.float().mean().item()
    span = ((nf[:, 1] - nf[:, 0])[hit.bool()].mean() / 4.0).item()
    rec["clip"] = {"rays": R, "ms": t_clip, "bytes": 41 * R, "GBps": 41 * R / t_clip["median"] / 1e6,
                   "rays_per_s": R / t_clip["median"] * 1e3, "hit_share": share, "mean_kept_span_of_hit_rays": span}

    # ---- frames: base fields, seeded weights
    models = {"coarse": NeRF("coarse"), "fine": NeRF("fine")}
    models["coarse"].load_state_dict(synth.make_field_params(11, "sharp", typ="coarse"))
    models["fine"].load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    models = {k: m.to(dev) for k, m in models.items()}
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    frame = lambda occ, ns=64, ni=128: nfl_eval.render_frame(models, emb, c2w, K, S, S, 2.0, 6.0, ns, ni, device=dev,
                                                             occupancy=occ)
    with torch.no_grad():
        t_full = host_timed(lambda: frame(None), a.warmup, a.iters)
        t_skip = host_timed(lambda: frame(grid), a.warmup, a.iters)
    rec["frame"] = {"size": [S, S], "samples": [64, 128], "full_ms": t_full, "clipped_ms": t_skip, "hit_share": share,
                    "clipped_over_full": t_skip["median"] / t_full["median"], "precision": rendering.get_precision()}

    # ---- fidelity on a grid taken from the field itself
    m = a.field
    rec["psnr"] = []
    with torch.no_grad():
        sigma = geometry.density_lattice(models["fine"], emb, lo, hi, (m, m, m))
        full = frame(None)[1]["rgb_fine"]
        # seeded weights have no empty space of their own: the thresholds are quantiles of the lattice, not densities a
        # trained scene would suggest
        for q in (0.0, 0.5, 0.9, 0.99):
            thr = sigma.flatten().kthvalue(max(1, int(round(q * sigma.numel())))).values.item()
            g = geometry.occupancy_grid(sigma, thr, lo, hi)
            row = {"quantile": q, "threshold": thr, "lattice": [m, m, m], "dilate": 1, "occupied": g.fraction(),
                   "hit_share": geometry.clip_rays(g, rays)[1].float().mean().item()}
            for ns, ni in ((64, 128), (32, 64)):
                row[f"psnr_{ns}+{ni}_vs_full_64+128"] = psnr(frame(g, ns, ni)[1]["rgb_fine"], full)
            rec["psnr"].append(row)
    rendering.check_status(dev)
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
