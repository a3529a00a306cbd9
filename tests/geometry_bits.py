"""Every output of a small fixed walk through nerf_fl_amd.geometry, written to an .npz: the check that a change of the
Python layer computes the same bits.  Public names only, so the same file runs at two commits:

    python tests/geometry_bits.py --out a.npz             (on the GPU; twice per commit)
    python tests/geometry_bits.py --compare a.npz b.npz   (anywhere: the arrays that differ, by name)

The walk: density_lattice of a seeded synth field at (70, 3, 2) with chunk=200 and at (300, 2, 2); an analytic ball on 17^3;
extract_surface, clean_mesh(largest=1), smooth_mesh(2), simplify_mesh in both placements with its map, mesh_adjacency,
vertex_normals, occupancy_grid and clip_rays of 65 rays; mesh_depth, mesh_visibility and render_mesh in both camera forms
against a bank of three 48 x 40 images, color_mesh_from_images (plain, with reject, with batch_pixels below one image),
bake_texture(cell=6) in batches with reject, render_mesh(texture=); write_ply and write_obj as file bytes."""
import argparse
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def walk():
    import torch
    import meshcolor_ref as mref
    from gpu_util import DEV, make_embeddings
    from nerf_fl_amd import NeRF, geometry, synth
    from nerf_fl_amd.data import ImageBank

    out = {}

    def put(name, value):
        if isinstance(value, dict):
            for k, v in value.items():
                put(f"{name}.{k}", v)
        elif isinstance(value, (tuple, list)) and any(torch.is_tensor(v) or isinstance(v, dict) for v in value):
            for k, v in enumerate(value):
                put(f"{name}.{k}", v)
        else:
            out[name] = value.detach().cpu().numpy() if torch.is_tensor(value) else np.asarray(value)

    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(DEV)
    emb = make_embeddings(10, False)
    with torch.no_grad():
        put("lattice.70x3x2", geometry.density_lattice(model, emb, (-1.0, -0.5, 0.0), (1.0, 0.5, 0.25), (70, 3, 2), chunk=200))
        put("lattice.300x2x2", geometry.density_lattice(model, emb, (-1.0, -0.5, 0.0), (1.0, 0.5, 0.25), (300, 2, 2)))
        put("lattice.colour", geometry.density_lattice(model, emb, (-1.0, -0.5, 0.0), (1.0, 0.5, 0.25), (33, 3, 2),
                                                       view_dir=(0.0, 0.6, 0.8)))

    lo, hi = (-1.0,) * 3, (1.0,) * 3
    c = torch.linspace(-1.0, 1.0, 17, device=DEV, dtype=torch.float64)
    r = torch.sqrt(c[:, None, None] ** 2 + c[None, :, None] ** 2 + c[None, None, :] ** 2)
    lat = torch.maximum(0.8 - r, 0.2 - torch.sqrt((c[:, None, None] - 0.75) ** 2 + (c[None, :, None] - 0.75) ** 2 + (c[None, None, :] - 0.75) ** 2))
    lat = lat.float().contiguous()                                       # a ball, and a speck of its own near the corner
    put("points", geometry.lattice_points(lo, hi, (17, 17, 17), DEV))
    raw = geometry.extract_surface(lat, 0.0, lo, hi)
    put("surface", raw)
    put("components", geometry.mesh_components(raw))
    mesh = geometry.clean_mesh(raw, largest=1)
    put("cleaned", mesh)
    put("cleaned.box", geometry.clean_mesh(raw, min_triangles=1, box=((-0.9,) * 3, (0.9,) * 3)))
    put("smoothed", geometry.smooth_mesh(mesh, iterations=2))
    for placement in ("mean", "quadric"):
        put(f"simplified.{placement}", geometry.simplify_mesh(mesh, 0.3, origin=lo, placement=placement, return_map=True))
    put("adjacency", geometry.mesh_adjacency(mesh))
    put("normals.area", geometry.vertex_normals(mesh))
    put("normals.uniform", geometry.vertex_normals(mesh, weighting="uniform", fallback=mesh["normals"]))
    grid = geometry.occupancy_grid(lat, 0.0, lo, hi, dilate=1)
    put("occupancy.bits", grid.bits)
    rng = np.random.default_rng(3)
    rays = np.concatenate([rng.uniform(-2, 2, (65, 3)), rng.normal(size=(65, 3)), np.full((65, 1), 0.1), np.full((65, 1), 6.0)], axis=1)
    put("clipped", geometry.clip_rays(grid, torch.from_numpy(rays.astype(np.float32)).to(DEV)))

    eyes = [(3, 0, 0), (0, 3, 0), (0, 0, 3)]
    poses = np.stack([mref.look_at(e, up=(0.0, 0.0, 1.0) if e[2] == 0 else (0.0, 1.0, 0.0)) for e in eyes])
    K = np.array([[50.0, 0, 48 / 2 - 0.25], [0, 50.0, 40 / 2 - 0.5], [0, 0, 1]])
    images = [rng.integers(0, 256, size=(40, 48, 3), dtype=np.uint8) for _ in eyes]
    bank = ImageBank(images, poses, np.stack([K] * 3), 2.0, 6.0, device=DEV)
    d_pose, d_K = torch.from_numpy(poses[1]).float().to(DEV), torch.from_numpy(K).float().to(DEV)
    mesh["colors"] = (0.1 + 0.4 * (mesh["vertices"] + 1.0)).contiguous()
    for form, args, kw in (("free", (d_pose, d_K, 40, 48), {}), ("bank", (), dict(bank=bank, image=1))):
        put(f"depth.{form}", geometry.mesh_depth(mesh, *args, **kw))
        put(f"visibility.{form}", geometry.mesh_visibility(mesh, *args, **kw))
        for shade in ("color", "normal", "facing"):
            put(f"render.{form}.{shade}", geometry.render_mesh(mesh, *args, shade=shade, background=(0.25, 0.5, 0.75), **kw))
    put("coloured", geometry.color_mesh_from_images(mesh, bank, 0.1))
    put("coloured.reject", geometry.color_mesh_from_images(mesh, bank, 0.1, reject=0.2, fallback=(0.1, 0.2, 0.3)))
    put("coloured.runs", geometry.color_mesh_from_images(mesh, bank, 0.1, reject=0.2, batch_pixels=1000, weighting="uniform"))
    coarse = geometry.simplify_mesh(mesh, 0.3, origin=lo)
    lay = geometry.atlas_layout(coarse["triangles"].shape[0], 6)
    atlas = geometry.bake_texture(coarse, bank, 0.1, cell=6, texel_batch=lay["width"] * lay["height"] // 3 + 1, reject=0.2,
                                  background=(0.5, 0.25, 0.0))
    put("atlas", atlas)
    put("atlas.flat", geometry.bake_texture(coarse, bank, 0.1, cell=6, fallback=(0.1, 0.2, 0.3), images=[0, 2]))
    put("render.texture", geometry.render_mesh(coarse, bank=bank, image=2, texture=atlas))
    put("render.texture.free", geometry.render_mesh(coarse, d_pose, d_K, 40, 48, texture={k: atlas[k] for k in ("texture_u8", "cell", "cols")}))
    put("uv", geometry.atlas_uv(lay, coarse["triangles"].shape[0]))

    with tempfile.TemporaryDirectory() as tmp:
        geometry.write_ply(os.path.join(tmp, "m.ply"), mesh, mesh["colors"])
        geometry.write_obj(os.path.join(tmp, "m.obj"), coarse, atlas)
        for name in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, name), "rb") as f:
                out["file." + name] = np.frombuffer(f.read(), dtype=np.uint8)
    return out


def compare(paths):
    runs = [dict(np.load(p)) for p in paths]
    names = sorted(runs[0])
    assert all(sorted(r) == names for r in runs), "the runs hold different arrays"
    differ = []
    for n in names:
        first = runs[0][n]
        if not all(r[n].dtype == first.dtype and r[n].shape == first.shape and r[n].tobytes() == first.tobytes() for r in runs[1:]):
            differ.append(n)
    print(f"{len(names)} arrays, {sum(runs[0][n].nbytes for n in names)} bytes, {len(paths)} runs: {len(differ)} differ {differ}")
    return differ


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs="+")
    a = ap.parse_args()
    if a.compare:
        sys.exit(1 if compare(a.compare) else 0)
    arrays = walk()
    np.savez(a.out, **arrays)
    print(f"{len(arrays)} arrays written to {a.out}")
