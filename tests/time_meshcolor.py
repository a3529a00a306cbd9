#!/usr/bin/env python3
"""What colouring a mesh from its images costs on one MI355X (geometry.mesh_depth / color_mesh_from_images,
csrc/nfl_meshcolor.hip).  Not a test: prints one JSON record (and writes it to --out).

    depth_fine_mesh    nfl_mesh_depth of one 800 x 800 camera for a ball extracted on a 257^3 lattice: nearly all boxes
                       are a few pixels and walked by their own lane
    depth_simplified   the same for that mesh after simplify_mesh at 8 lattice spacings: boxes of hundreds of pixels, the
                       wave path
    depth_fine_plus_frame_triangle   the fine mesh and one triangle that fills the frame: one box of 640 000 pixels
    blend              nfl_mesh_blend over a 100-image bank (depth maps of a run of --run images at a time)
    color_mesh         color_mesh_from_images end to end, beside surface_colors on the same mesh

Every figure is the median (and range) over `--iters` calls after `--warmup` calls of the same thing, each blend run
included; kernels are bracketed by device events, the end-to-end rows by the host's clock.  With `--variant-lib` the record
also holds the raster times of a library built with the wave path off, taken by this script in a child process.  For the raster the
triangle-pixel tests are counted from the boxes the kernel takes (the header's rule, restated here in torch), and the share
that hit is estimated as projected triangle area over box area.  For the blend the bytes are those a vertex-image pair
touches when it contributes: the 104-byte record (cached), one depth word, four pixels."""
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


def boxes(ver, tri, c2w, K, S):
    """(tests, estimated hits, share of boxes above 64 pixels) of one camera, by the kernel's rule."""
    R, t = c2w[:, :3].double(), c2w[:, 3].double()
    q = (ver.double() - t) @ R
    s = -q[:, 2]
    u, v = K[0, 2] + K[0, 0] * q[:, 0] / s, K[1, 2] - K[1, 1] * q[:, 1] / s
    i = tri.long()
    front = (s[i] > 0).all(dim=1)
    U, Vv = u[i][front], v[i][front]
    x0, x1 = (U.min(dim=1).values.floor() - 1).clamp(0, S), (U.max(dim=1).values.ceil() + 1).clamp(-1, S - 1)
    y0, y1 = (Vv.min(dim=1).values.floor() - 1).clamp(0, S), (Vv.max(dim=1).values.ceil() + 1).clamp(-1, S - 1)
    area = (x1 - x0 + 1).clamp(min=0) * (y1 - y0 + 1).clamp(min=0)
    proj = 0.5 * ((U[:, 1] - U[:, 0]) * (Vv[:, 2] - Vv[:, 0]) - (U[:, 2] - U[:, 0]) * (Vv[:, 1] - Vv[:, 0])).abs()
    return float(area.sum()), float(proj[area > 0].sum()), float((area > 64).double().mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=256)
    ap.add_argument("--frame", type=int, default=800)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--run", type=int, default=10, help="images whose depth maps are held at a time")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-depth", action="store_true", help="the raster figures only (what --variant-lib runs in a child)")
    ap.add_argument("--variant-lib", default=None,
                    help="a library built with the wave path off (make variant VTU=nfl_meshcolor VNAME=_nobig "
                         "VFLAGS=-DNMC_SMALL_BOX=1073741824): its raster times are taken in a child process and recorded "
                         "beside each depth row as ms_wave_path_off")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("time_meshcolor.py measures on the GPU; there is none here")
    from nerf_fl_amd import NeRF, PosEmbedding, _lib, eval as nfl_eval, geometry, synth
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
    coarse = geometry.simplify_mesh(fine, 8 * 3.0 / a.cells, origin=lo)
    K = torch.as_tensor(nfl_eval.fov60_intrinsics(S, S), dtype=torch.float32)
    # cameras on a sphere of radius 4 (a Fibonacci spiral), looking at the centre
    k = np.arange(a.images) + 0.5
    z, phi = 1 - 2 * k / a.images, np.pi * (1 + 5 ** 0.5) * k
    eyes = 4.0 * np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], axis=1)
    c2w = np.stack([mref.look_at(e, up=(0.0, 0.0, 1.0) if abs(e[2]) < 3.9 else (0.0, 1.0, 0.0)) for e in eyes])
    image = np.random.default_rng(0).integers(0, 256, size=(S, S, 3), dtype=np.uint8)
    bank = ImageBank([image] * a.images, c2w, K.numpy(), 2.0, 6.0, device=dev)

    # ---- raster: one camera, through the C ABI
    depth = torch.empty(S * S, dtype=torch.float32, device=dev)
    # the fine mesh with ONE triangle behind it that fills the frame of camera 0: a single box of frame * frame pixels among
    # a million small ones, the case of divergent trip counts
    back = torch.tensor([[-20.0, -12.0, -6.0], [20.0, -12.0, -6.0], [0.0, 20.0, -6.0]], dtype=torch.float64)
    pose = torch.from_numpy(c2w[0])
    back = (back @ pose[:, :3].T + pose[:, 3]).float().to(dev)
    V0 = fine["vertices"].shape[0]
    mixed = {"vertices": torch.cat([fine["vertices"], back]),
             "triangles": torch.cat([fine["triangles"], torch.tensor([[V0, V0 + 1, V0 + 2]], dtype=torch.int32, device=dev)])}
    for name, mesh in (("depth_fine_mesh", fine), ("depth_simplified", coarse), ("depth_fine_plus_frame_triangle", mixed)):
        ver, tri = mesh["vertices"], mesh["triangles"]
        call = lambda: geometry.images._run_depth(ver, tri, bank.table, bank.n_images, 0, 1, depth)
        t = timed(call, a.warmup, a.iters)
        tests, hits, big = boxes(ver, tri, torch.from_numpy(c2w[0]).to(dev), K.double(), S)
        rec[name] = {"vertices": ver.shape[0], "triangles": tri.shape[0], "ms": t, "tests": tests,
                     "tests_per_s": tests / t["median"] * 1e3, "hit_share_estimate": hits / max(tests, 1.0),
                     "boxes_above_64_pixels": big, "covered": torch.isfinite(depth).float().mean().item()}

    if a.only_depth:
        print(json.dumps(rec))
        return
    if a.variant_lib:
        # a fresh process: the library is chosen when the package loads it (NERF_FL_AMD_DEV=1 NFL_LIB=...)
        cmd = [sys.executable, os.path.abspath(__file__), "--only-depth", "--cells", str(a.cells), "--frame", str(a.frame),
               "--images", str(a.images), "--warmup", str(a.warmup), "--iters", str(a.iters)]
        env = dict(os.environ, NERF_FL_AMD_DEV="1", NFL_LIB=os.path.abspath(a.variant_lib))
        out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=600).stdout
        off = json.loads([line for line in out.splitlines() if line.startswith("{")][-1])
        rec["variant_lib"] = os.path.basename(a.variant_lib)
        for name in ("depth_fine_mesh", "depth_simplified", "depth_fine_plus_frame_triangle"):
            rec[name]["ms_wave_path_off"] = off[name]["ms"]

    # ---- blend: the bank in runs, depth maps rastered outside the timed region
    ver, nrm, tri = fine["vertices"], fine["normals"], fine["triangles"]
    V = ver.shape[0]
    sums = torch.empty(V, 4, dtype=torch.float32, device=dev)
    views = torch.empty(V, dtype=torch.int32, device=dev)
    tol = 2 * 3.0 / a.cells
    run = max(1, min(a.run, a.images))
    depths = torch.empty(run * S * S, dtype=torch.float32, device=dev)
    ms, pairs = [], 0
    for first in range(0, a.images, run):
        count = min(run, a.images - first)
        geometry.images._run_depth(ver, tri, bank.table, bank.n_images, first, count, depths[:count * S * S])
        b = _lib.MeshBlendArgs()
        b.d_vertices, b.d_normals, b.n_vertices, b.d_pixels = ver.data_ptr(), nrm.data_ptr(), V, bank.pixels.data_ptr()
        b.d_table, b.n_images, b.first, b.count, b.weighting = bank.table.data_ptr(), bank.n_images, first, count, 0
        b.d_depth, b.n_depth, b.min_cos, b.depth_tol, b.start = depths.data_ptr(), count * S * S, 0.0, tol, 1
        b.d_sum, b.d_views = sums.data_ptr(), views.data_ptr()
        t = timed(lambda: _lib.check(lib.nfl_mesh_blend(C.byref(b), stream()), "blend"), a.warmup, a.iters)
        ms.append(t["median"])
        pairs += int(views.sum().item())
    total = sum(ms)
    rec["blend"] = {"vertices": V, "images": a.images, "run": run, "ms_sum_of_run_medians": total, "ms_per_run": ms,
                    "vertex_image_pairs": V * a.images, "contributing_pairs": pairs,
                    "pairs_per_s": V * a.images / total * 1e3, "bytes_per_contributing_pair": 4 + 4 * 3,
                    "bytes_per_vertex": 24 + 16 + 4 + 16 + 4, "record_bytes_cached": 104}

    # ---- end to end, beside the field's own colours
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(dev)
    emb = {"xyz": PosEmbedding(9, 10), "dir": PosEmbedding(3, 4)}
    with torch.no_grad():
        t_img = host_timed(lambda: geometry.color_mesh_from_images(fine, bank, tol, batch_pixels=run * S * S), a.warmup, a.iters)
        t_fld = host_timed(lambda: geometry.surface_colors(model, emb, ver, nrm), a.warmup, a.iters)
    got = geometry.color_mesh_from_images(fine, bank, tol, batch_pixels=run * S * S)
    rec["color_mesh"] = {"from_images_ms": t_img, "surface_colors_ms": t_fld, "seen": got["seen"].float().mean().item(),
                         "mean_views": got["views"].float().mean().item()}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
