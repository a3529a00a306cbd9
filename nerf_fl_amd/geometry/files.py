"""A mesh on disk: write_ply, write_obj.  They work on host arrays (numpy, and Pillow for the atlas) and call nothing in
the library."""
import os

import numpy as np

from ._call import _host, _host_mesh
from .images import atlas_layout, atlas_uv


def write_ply(path, mesh, colors=None):
    """Write `mesh` (the dict extract_surface returns; tensors or arrays) as a binary little-endian PLY: per vertex x, y,
    z, nx, ny, nz as float32 and, with `colors` ((V, 3) in [0, 1]), red, green, blue as uint8 (rounded); per face a
    uint8 count of 3 and three int32 indices."""
    ver, nrm, tri = _host_mesh(mesh)
    V, T = ver.shape[0], tri.shape[0]
    fields = [(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")]
    if colors is not None:
        col = _host(colors)
        if col.shape != (V, 3):
            raise ValueError(f"colors: expected ({V}, 3), got {col.shape}")
        fields += [(n, "u1") for n in ("red", "green", "blue")]
    vrec = np.empty(V, dtype=fields)
    for k, n in enumerate(("x", "y", "z")):
        vrec[n], vrec["n" + n] = ver[:, k], nrm[:, k]
    if colors is not None:
        c8 = np.rint(np.clip(np.nan_to_num(col.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        for k, n in enumerate(("red", "green", "blue")):
            vrec[n] = c8[:, k]
    frec = np.empty(T, dtype=[("n", "u1"), ("v", "<i4", (3,))])
    frec["n"], frec["v"] = 3, tri
    kinds = {"<f4": "float", "u1": "uchar"}
    header = ["ply", "format binary_little_endian 1.0", "comment nerf_fl_amd.geometry", f"element vertex {V}"]
    header += [f"property {kinds[t]} {n}" for n, t in fields]
    header += [f"element face {T}", "property list uchar int vertex_indices", "end_header"]
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vrec.tobytes())
        f.write(frec.tobytes())


def write_obj(path, mesh, atlas):
    """Write `mesh` with its texture `atlas` (the dict bake_texture returns; tensors or arrays) as `stem`.obj,
    `stem`.mtl and `stem`.png beside each other, `path` being any of the three or the bare stem: per vertex `v` and
    `vn`, per CORNER a `vt` ((x + 0.5) / W, 1 - (y + 0.5) / H of atlas_uv: the PNG's row 0 is the top), faces
    `f v/vt/vn` 1-based, the material's `map_Kd` the PNG of `texture_u8`.  Needs Pillow."""
    from PIL import Image
    ver, nrm, tri = _host_mesh(mesh)
    T = tri.shape[0]
    try:
        tex8, cell, cols = atlas.get("texture_u8"), int(atlas["cell"]), int(atlas["cols"])
    except (TypeError, KeyError, AttributeError):
        raise ValueError("atlas: a dict with `texture_u8` (H, W, 3) uint8, `cell` and `cols`") from None
    if tex8 is None:
        raise ValueError("atlas: a dict with `texture_u8` (H, W, 3) uint8, `cell` and `cols`")
    tex8 = _host(tex8)
    lay = atlas_layout(T, cell, cols)
    if tex8.dtype != np.uint8 or tex8.ndim != 3 or tex8.shape[2] != 3 or tex8.shape[1] != lay["width"] \
            or tex8.shape[0] % cell or tex8.shape[0] < lay["height"]:
        raise ValueError(f"atlas: texture_u8 {tex8.shape} is not an atlas of cell {cell} and {cols} columns for {T} triangles")
    H, W = tex8.shape[:2]
    stem = str(path)
    if stem.lower().endswith((".obj", ".mtl", ".png")):
        stem = stem[:-4]
    name = os.path.basename(stem)
    Image.fromarray(np.ascontiguousarray(tex8), "RGB").save(stem + ".png")
    with open(stem + ".mtl", "w") as f:
        f.write(f"# nerf_fl_amd.geometry\nnewmtl {name}\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nillum 0\nmap_Kd {name}.png\n")
    uv = atlas_uv(lay, T).reshape(-1, 2)
    vt = np.stack([(uv[:, 0] + 0.5) / W, 1.0 - (uv[:, 1] + 0.5) / H], axis=1)
    # numpy's tolist below, on host arrays: Python floats and ints, whose repr the file's numbers are
    lines = [f"# nerf_fl_amd.geometry\nmtllib {name}.mtl\nusemtl {name}\n"]
    lines += ["".join(f"v {x!r} {y!r} {z!r}\n" for x, y, z in ver.astype(np.float64).tolist())]
    lines += ["".join(f"vn {x!r} {y!r} {z!r}\n" for x, y, z in nrm.astype(np.float64).tolist())]
    lines += ["".join(f"vt {u!r} {v!r}\n" for u, v in vt.tolist())]
    lines += ["".join(f"f {a + 1}/{3 * t + 1}/{a + 1} {b + 1}/{3 * t + 2}/{b + 1} {c + 1}/{3 * t + 3}/{c + 1}\n"
                      for t, (a, b, c) in enumerate(tri.tolist()))]
    with open(stem + ".obj", "w") as f:
        f.write("".join(lines))
