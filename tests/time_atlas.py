#!/usr/bin/env python3
"""What baking and sampling a texture atlas costs on one MI355X (geometry.bake_texture / render_mesh(texture=),
csrc/nfl_atlas.hip).  Not a test: prints one JSON record (and writes it to --out).

The scene is time_meshcolor.py's and time_meshrender.py's: a ball of radius 1.2 extracted on a 257^3 lattice, the same mesh
simplified at 8 lattice spacings, 800 x 800 cameras at fov 60 from distance 4, a bank of 100 of them on a Fibonacci spiral.
The atlas is the SIMPLIFIED mesh's, at --cell texels a cell:

    points          nfl_atlas_points of the whole atlas
    blend_texels    nfl_mesh_blend of the texels over the bank in runs of --run images (depth maps of the simplified mesh,
                    rastered outside the timed region), and the time per (point, image) pair
    blend_vertices  the same call over the FINE mesh's vertices and depth maps, as color_mesh_from_images makes it: the
                    yardstick for the time per pair
    resolve         nfl_atlas_resolve of the whole atlas, all three outputs
    shade_atlas     nfl_mesh_shade_atlas of one camera's words (fp32 atlas, byte atlas) beside nfl_mesh_shade in COLOR mode
    bake_texture, render_mesh(texture=)   end to end, on the host's clock
    bench           with --bench-steps N: `bench.py --gpus 1 --steps N --warmup 10` in a child process after everything else,
                    to set the train step beside the parent's

Every figure is the median (and range) over `--iters` calls after `--warmup` calls of the same thing; kernels are bracketed
by device events, the end-to-end rows by the host's clock."""
import argparse
import ctypes as C
import json
import os
import subprocess
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
    ap.add_argument("--run", type=int, default=25)
    ap.add_argument("--cell", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--bench-steps", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_atlas.py measures on the GPU; there is none here")
    from nerf_fl_amd import _lib, eval as nfl_eval, geometry
    from nerf_fl_amd.data import ImageBank
    dev = torch.device("cuda:0")
    lib = _lib.lib()
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rec = {"device": torch.cuda.get_device_name(0), "warmup": a.warmup, "iters": a.iters, "frame": [a.frame, a.frame],
           "images": a.images, "run": a.run, "cell": a.cell}

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
    tol = 2 * 3.0 / a.cells

    ver, nrm, col, tri = (coarse[key] for key in ("vertices", "normals", "colors", "triangles"))
    V, T = ver.shape[0], tri.shape[0]
    lay = geometry.atlas_layout(T, a.cell)
    N = lay["width"] * lay["height"]
    rec["mesh"] = {"fine_vertices": fine["vertices"].shape[0], "fine_triangles": fine["triangles"].shape[0], "vertices": V,
                   "triangles": T}
    rec["atlas"] = dict(lay, texels=N)

    # ---- points
    pts, nor = (torch.empty(N, 3, dtype=torch.float32, device=dev) for _ in range(2))
    p = _lib.AtlasPointsArgs()
    p.d_vertices, p.d_vertex_normals, p.d_triangles, p.n_vertices, p.n_triangles = ver.data_ptr(), nrm.data_ptr(), tri.data_ptr(), V, T
    p.cell, p.cols, p.rows, p.first_texel, p.n_texels = lay["cell"], lay["cols"], lay["rows"], 0, N
    p.d_points, p.d_normals = pts.data_ptr(), nor.data_ptr()
    rec["points"] = {"ms": timed(lambda: _lib.check(lib.nfl_atlas_points(C.byref(p), stream()), "points"), a.warmup, a.iters),
                     "bytes_written": 24 * N}

    # ---- the blend over the texels, and over the fine mesh's vertices: the same kernel, the time per (point, image) pair
    run = max(1, min(a.run, a.images))
    depths = torch.empty(run * S * S, dtype=torch.float32, device=dev)

    def blend(points, normals, mesh):
        n_pts = points.shape[0]
        sums = torch.empty(n_pts, 4, dtype=torch.float32, device=dev)
        views = torch.empty(n_pts, dtype=torch.int32, device=dev)
        ms, pairs = [], 0
        for first in range(0, a.images, run):
            count = min(run, a.images - first)
            geometry.images._run_depth(mesh["vertices"], mesh["triangles"], bank.table, bank.n_images, first, count,
                                       depths[:count * S * S])
            b = _lib.MeshBlendArgs()
            b.d_vertices, b.d_normals, b.n_vertices, b.d_pixels = points.data_ptr(), normals.data_ptr(), n_pts, bank.pixels.data_ptr()
            b.d_table, b.n_images, b.first, b.count, b.weighting = bank.table.data_ptr(), bank.n_images, first, count, 0
            b.d_depth, b.n_depth, b.min_cos, b.depth_tol, b.start = depths.data_ptr(), count * S * S, 0.0, tol, 1
            b.d_sum, b.d_views = sums.data_ptr(), views.data_ptr()
            ms.append(timed(lambda: _lib.check(lib.nfl_mesh_blend(C.byref(b), stream()), "blend"), a.warmup, a.iters)["median"])
            pairs += int(views.sum().item())
        total = sum(ms)
        return ({"points": n_pts, "ms_sum_of_run_medians": total, "ms_per_run": ms, "pairs": n_pts * a.images,
                 "contributing_pairs": pairs, "ns_per_pair": total * 1e6 / (n_pts * a.images)}, sums, views)

    rec["blend_texels"], sums, views = blend(pts, nor, coarse)
    rec["blend_vertices"], _, _ = blend(fine["vertices"], fine["normals"], fine)
    rec["ns_per_pair_texels_over_vertices"] = rec["blend_texels"]["ns_per_pair"] / rec["blend_vertices"]["ns_per_pair"]

    # ---- resolve (of the last run's sums: the time does not depend on what they hold)
    tex = torch.empty(N, 3, dtype=torch.float32, device=dev)
    tex8 = torch.empty(N, 3, dtype=torch.uint8, device=dev)
    seen = torch.empty(N, dtype=torch.uint8, device=dev)
    r = _lib.AtlasResolveArgs()
    r.d_triangles, r.n_vertices, r.n_triangles = tri.data_ptr(), V, T
    r.cell, r.cols, r.rows, r.first_texel, r.n_texels = lay["cell"], lay["cols"], lay["rows"], 0, N
    r.d_sum, r.d_views, r.d_vertex_colors = sums.data_ptr(), views.data_ptr(), col.data_ptr()
    r.d_texture, r.d_texture_u8, r.d_seen = tex.data_ptr(), tex8.data_ptr(), seen.data_ptr()
    rec["resolve"] = {"ms": timed(lambda: _lib.check(lib.nfl_atlas_resolve(C.byref(r), stream()), "resolve"), a.warmup, a.iters),
                      "bytes_per_texel": 16 + 4 + 12 + 3 + 1}

    # ---- the shading pass: the atlas beside the vertex colours, one camera's words
    vis = torch.empty(S * S, dtype=torch.int64, device=dev)
    geometry.images._run_visibility(ver, tri, bank.table, bank.n_images, 0, 1, vis)
    out = {"rgb": torch.empty(S * S, 3, dtype=torch.float32, device=dev), "u8": torch.empty(S * S, 3, dtype=torch.uint8, device=dev),
           "depth": torch.empty(S * S, dtype=torch.float32, device=dev), "tri": torch.empty(S * S, dtype=torch.int32, device=dev)}
    row = {"covered": (vis != -1).float().mean().item()}
    for name, args in (("shade_color", _lib.MeshShadeArgs()), ("shade_atlas_f32", _lib.MeshShadeAtlasArgs()),
                       ("shade_atlas_u8", _lib.MeshShadeAtlasArgs())):
        s = args
        s.d_vertices, s.d_triangles, s.n_vertices, s.n_triangles = ver.data_ptr(), tri.data_ptr(), V, T
        s.d_table, s.n_images, s.first, s.count = bank.table.data_ptr(), bank.n_images, 0, 1
        s.d_vis, s.n_vis = vis.data_ptr(), S * S
        s.background[:] = (1.0, 1.0, 1.0)
        s.d_rgb, s.d_rgb_u8, s.d_depth, s.d_triangle = (out[key].data_ptr() for key in ("rgb", "u8", "depth", "tri"))
        if name == "shade_color":
            s.mode, s.d_attr = _lib.SHADE_MODES["color"], col.data_ptr()
            fn = lambda: _lib.check(lib.nfl_mesh_shade(C.byref(s), stream()), "shade")
        else:
            s.cell, s.cols, s.rows = lay["cell"], lay["cols"], lay["rows"]
            s.d_atlas, s.d_atlas_u8 = (tex.data_ptr(), None) if name.endswith("f32") else (None, tex8.data_ptr())
            fn = lambda: _lib.check(lib.nfl_mesh_shade_atlas(C.byref(s), stream()), "shade_atlas")
        row[name + "_ms"] = timed(fn, a.warmup, a.iters)
    rec["shade"] = row

    # ---- end to end
    rec["bake_texture_ms"] = host_timed(lambda: geometry.bake_texture(coarse, bank, tol, cell=a.cell, batch_pixels=run * S * S),
                                        a.warmup, a.iters)
    baked = geometry.bake_texture(coarse, bank, tol, cell=a.cell, batch_pixels=run * S * S)
    rec["bake"] = {"seen": baked["seen"].float().mean().item(), "mean_views": baked["views"].float().mean().item()}
    rec["render_mesh_texture_ms"] = host_timed(lambda: geometry.render_mesh(coarse, bank=bank, image=0, texture=baked), a.warmup, a.iters)
    rec["render_mesh_colors_ms"] = host_timed(lambda: geometry.render_mesh(coarse, bank=bank, image=0), a.warmup, a.iters)

    if a.bench_steps > 0:
        del bank, depths, pts, nor, sums, views, tex, tex8, seen, vis, out, fine, coarse, baked
        torch.cuda.empty_cache()
        cmd = [sys.executable, os.path.join(os.path.dirname(HERE), "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", "10"]
        text = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=900).stdout
        rec["bench"] = json.loads([line for line in text.splitlines() if line.startswith("{")][-1])
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
