#!/usr/bin/env python3
"""What rendering a coloured mesh costs on one MI355X (geometry.mesh_visibility / render_mesh, eval.evaluate_mesh,
csrc/nfl_meshrender.hip).  Not a test: prints one JSON record (and writes it to --out).

The scene is time_meshcolor.py's: a ball of radius 1.2 extracted on a 257^3 lattice, the same mesh simplified at 8 lattice
spacings, one 800 x 800 camera at fov 60 from distance 4, a bank of 100 such cameras on a Fibonacci spiral.  Per mesh:

    visibility      nfl_mesh_visibility of one camera: fill + raster, a 64-bit atomicMin per hit
    depth           nfl_mesh_depth on the same inputs in the same process: the yardstick, a 32-bit atomicMin per hit
    shade_<mode>    nfl_mesh_shade of that camera's words, all four outputs
    render_mesh     geometry.render_mesh end to end, on the host's clock
    evaluate_mesh   eval.evaluate_mesh over the bank (the fine mesh only)

Every figure is the median (and range) over `--iters` calls after `--warmup` calls of the same thing; kernels are
bracketed by device events, the end-to-end rows by the host's clock."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from geom_timing import host_timed, timed  # noqa: E402
import meshcolor_ref as mref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--frame", type=int, default=800)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_meshrender.py measures on the GPU; there is none here")
    from nerf_fl_amd import _lib, eval as nfl_eval, geometry
    from nerf_fl_amd.data import ImageBank
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "frame": [a.frame, a.frame]}

    n, S = a.cells + 1, a.frame
    lo, hi = (-1.5,) * 3, (1.5,) * 3
    c = torch.linspace(-1.5, 1.5, n, device=dev, dtype=torch.float64)
    lat = (1.2 - torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)).float().contiguous()
    fine = geometry.extract_surface(lat, 0.0, lo, hi)
    del lat
    fine["colors"] = (0.1 + 0.8 * (fine["vertices"] + 1.5) / 3.0).clamp(0.1, 0.9).contiguous()
    coarse = geometry.simplify_mesh(fine, 8 * 3.0 / a.cells, origin=lo)
    K = torch.as_tensor(nfl_eval.fov60_intrinsics(S, S), dtype=torch.float32)
    k = np.arange(a.images) + 0.5
    z, phi = 1 - 2 * k / a.images, np.pi * (1 + 5 ** 0.5) * k
    eyes = 4.0 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    c2w = np.stack([mref.look_at(e, up=(0.0, 0.0, 1.0) if abs(e[2]) < 3.9 else (0.0, 1.0, 0.0)) for e in eyes])
    image = np.random.default_rng(0).integers(0, 256, size=(S, S, 3), dtype=np.uint8)
    bank = ImageBank([image] * a.images, c2w, K.numpy(), 2.0, 6.0, device=dev)

    vis = torch.empty(S * S, dtype=torch.int64, device=dev)
    depth = torch.empty(S * S, dtype=torch.float32, device=dev)
    out = {"rgb": torch.empty(S * S, 3, dtype=torch.float32, device=dev), "u8": torch.empty(S * S, 3, dtype=torch.uint8, device=dev),
           "depth": torch.empty(S * S, dtype=torch.float32, device=dev), "tri": torch.empty(S * S, dtype=torch.int32, device=dev)}
    for name, mesh in (("fine", fine), ("simplified", coarse)):
        ver, nrm, col, tri = mesh["vertices"], mesh["normals"], mesh["colors"], mesh["triangles"]
        row = {"vertices": ver.shape[0], "triangles": tri.shape[0]}
        row["visibility_ms"] = timed(lambda: geometry.images._run_visibility(ver, tri, bank.table, bank.n_images, 0, 1, vis),
                                     a.warmup, a.iters)
        row["depth_ms"] = timed(lambda: geometry.images._run_depth(ver, tri, bank.table, bank.n_images, 0, 1, depth),
                                a.warmup, a.iters)
        row["visibility_over_depth"] = row["visibility_ms"]["median"] / row["depth_ms"]["median"]
        row["covered"] = (vis != -1).float().mean().item()
        s = _lib.MeshShadeArgs()
        s.d_vertices, s.d_triangles, s.n_vertices, s.n_triangles = ver.data_ptr(), tri.data_ptr(), ver.shape[0], tri.shape[0]
        s.d_table, s.n_images, s.first, s.count = bank.table.data_ptr(), bank.n_images, 0, 1
        s.d_vis, s.n_vis = vis.data_ptr(), S * S
        s.background[:] = (1.0, 1.0, 1.0)
        s.d_rgb, s.d_rgb_u8, s.d_depth, s.d_triangle = (out[k].data_ptr() for k in ("rgb", "u8", "depth", "tri"))
        for mode, attr in (("color", col), ("normal", nrm), ("facing", None)):
            s.mode, s.d_attr = _lib.SHADE_MODES[mode], attr.data_ptr() if attr is not None else None
            row[f"shade_{mode}_ms"] = timed(lambda: _lib.check(lib.nfl_mesh_shade(C.byref(s), stream()), "shade"), a.warmup, a.iters)
        assert torch.equal(out["depth"], depth)                     # the shade's depth IS the depth map
        # bytes of the shade per pixel: the word, 36 B of vertices and 36 B of attributes when covered, 12 + 3 + 4 + 4 out
        row["shade_bytes_per_covered_pixel"] = 8 + 12 + 36 + 36 + 23
        row["render_mesh_ms"] = host_timed(lambda: geometry.render_mesh(mesh, bank=bank, image=0), a.warmup, a.iters)
        rec[name] = row
    res = nfl_eval.evaluate_mesh(fine, bank)
    rec["evaluate_mesh"] = {"images": a.images, "ms": host_timed(lambda: nfl_eval.evaluate_mesh(fine, bank), a.warmup, a.iters),
                            "mean_psnr": res["mean_psnr"], "mean_ssim": res["mean_ssim"],
                            "note": "the bank's images are noise: the scores say nothing, the time does"}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
