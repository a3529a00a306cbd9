"""A mesh on disk: write_ply, write_obj, and read_ply (public as meshdist.read_ply).  They work on host arrays (numpy,
and Pillow for the atlas) and call nothing in the library; read_ply alone, handed a device, uploads what it read."""
import os

import numpy as np

from ._call import _host, _host_mesh
from .images import atlas_layout, atlas_uv

INT32_MAX = 2 ** 31 - 1


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


_PLY_FLOAT = {"float": "f4", "float32": "f4"}
_PLY_UCHAR = {"uchar": "u1", "uint8": "u1"}
_PLY_INDEX = {"int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4"}
_PLY_VERTEX = ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")


def _ply_header(f):
    """(format, V, T, vertex properties [(name, numpy type)], face (count type, index type)) of a PLY stream, which is left
    at the first byte of the body."""
    if f.readline().strip() != b"ply":
        raise ValueError("read_ply: not a PLY file (the first line is not 'ply')")
    fmt, elements, current = None, [], None
    while True:
        raw = f.readline()
        if not raw:
            raise ValueError("read_ply: the header has no end_header")
        words = raw.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            break
        if words[0] == "format":
            fmt = words[1] if len(words) > 1 else ""
        elif words[0] == "element" and len(words) == 3:
            current = {"name": words[1], "count": int(words[2]), "props": []}
            elements.append(current)
        elif words[0] == "property" and current is not None:
            current["props"].append(words[1:])
        else:
            raise ValueError(f"read_ply: header line {' '.join(words)!r}")
    if fmt not in ("binary_little_endian", "ascii"):
        raise ValueError(f"read_ply: format {fmt!r}; binary_little_endian and ascii are read")
    if [e["name"] for e in elements] != ["vertex", "face"]:
        raise ValueError(f"read_ply: elements {[e['name'] for e in elements]}; 'vertex' then 'face' are read")
    vprops = []
    for p in elements[0]["props"]:
        if len(p) != 2 or p[1] not in _PLY_VERTEX:
            raise ValueError(f"read_ply: vertex property {' '.join(p)!r}; float x y z nx ny nz and uchar red green blue are read")
        kinds = _PLY_UCHAR if p[1] in ("red", "green", "blue") else _PLY_FLOAT
        if p[0] not in kinds:
            raise ValueError(f"read_ply: vertex property {p[1]!r} of type {p[0]!r}; {sorted(kinds)} is read")
        vprops.append((p[1], kinds[p[0]]))
    names = [n for n, _ in vprops]
    if len(set(names)) != len(names) or not {"x", "y", "z"} <= set(names):
        raise ValueError(f"read_ply: vertex properties {names}; x, y and z are needed, each once")
    for group in (("nx", "ny", "nz"), ("red", "green", "blue")):
        if 0 < len(set(group) & set(names)) < 3:
            raise ValueError(f"read_ply: vertex properties {names}; {group} come together")
    fprops = elements[1]["props"]
    if (len(fprops) != 1 or len(fprops[0]) != 4 or fprops[0][0] != "list" or fprops[0][1] not in _PLY_UCHAR
            or fprops[0][2] not in _PLY_INDEX or fprops[0][3] not in ("vertex_indices", "vertex_index")):
        raise ValueError(f"read_ply: face properties {[' '.join(p) for p in fprops]}; one 'list uchar int vertex_indices' is read")
    return fmt, elements[0]["count"], elements[1]["count"], vprops, _PLY_INDEX[fprops[0][2]]


def read_ply(path, device=None):
    """Read a triangle mesh from a PLY file: what write_ply writes, and the plain variants ground-truth meshes come
    in -- `binary_little_endian` or `ascii`; vertex properties float x y z, optionally float nx ny nz and uchar red green
    blue, in any order; faces as lists of 3 indices named vertex_indices or vertex_index.  Anything else is refused with a
    ValueError that names what was found.  Parsed with numpy alone; a round trip through write_ply is exact.

    Returns a mesh dict: vertices (V, 3) fp32, normals (V, 3) fp32, triangles (T, 3) int32 and, when the file has them,
    colors (V, 3) fp32 = byte / 255.  With a `device` they are tensors there, and missing normals are filled through
    vertex_normals; without one they are numpy arrays and missing normals are zeros."""
    with open(path, "rb") as f:
        fmt, V, T, vprops, index = _ply_header(f)
        body = f.read()
    if V < 0 or T < 0 or V > INT32_MAX or 3 * T > INT32_MAX:
        raise ValueError(f"read_ply: {V} vertices and {T} faces")
    vtype = np.dtype([(n, "<" + t) for n, t in vprops])
    if fmt == "binary_little_endian":
        ftype = np.dtype([("n", "u1"), ("v", "<" + index, (3,))])
        if len(body) != V * vtype.itemsize + T * ftype.itemsize:
            raise ValueError(f"read_ply: a body of {len(body)} bytes; {V} vertices and {T} triangles take "
                             f"{V * vtype.itemsize + T * ftype.itemsize} (faces that are not triangles are not read)")
        vrec = np.frombuffer(body, dtype=vtype, count=V)
        frec = np.frombuffer(body, dtype=ftype, count=T, offset=V * vtype.itemsize)
        counts, tri = frec["n"], frec["v"]
    else:
        words = body.split()
        nv = V * len(vprops)
        if len(words) != nv + 4 * T:
            raise ValueError(f"read_ply: a body of {len(words)} numbers; {V} vertices and {T} triangles take {nv + 4 * T} "
                             "(faces that are not triangles are not read)")
        try:
            table = np.array(words[:nv], dtype=np.float64).reshape(V, len(vprops))
            faces = np.array(words[nv:], dtype=np.int64).reshape(T, 4)
        except ValueError:
            raise ValueError("read_ply: a word of the body is not a number") from None
        vrec = np.empty(V, dtype=vtype)
        for k, (name, _) in enumerate(vprops):
            vrec[name] = table[:, k]
        counts, tri = faces[:, 0], faces[:, 1:]
    if T and (counts != 3).any():
        raise ValueError(f"read_ply: a face of {int(counts[counts != 3][0])} vertices; triangles are read")
    if T and (tri.min() < 0 or tri.max() >= V):
        raise ValueError("read_ply: a face index lies outside the vertices")
    names = vrec.dtype.names
    stack = lambda keys: np.ascontiguousarray(np.stack([vrec[k] for k in keys], axis=1), dtype=np.float32).reshape(V, 3)
    mesh = {"vertices": stack("xyz"), "triangles": np.ascontiguousarray(tri, dtype=np.int32).reshape(T, 3)}
    mesh["normals"] = stack(("nx", "ny", "nz")) if "nx" in names else None
    if "red" in names:
        mesh["colors"] = stack(("red", "green", "blue")) / np.float32(255.0)
    if device is None:
        if mesh["normals"] is None:
            mesh["normals"] = np.zeros((V, 3), dtype=np.float32)
        return mesh
    missing = mesh["normals"] is None
    if missing:
        mesh["normals"] = np.zeros((V, 3), dtype=np.float32)
    import torch                                                        # only the upload needs it, and the library
    from .mesh import vertex_normals
    out = {k: torch.from_numpy(v).to(device) for k, v in mesh.items()}
    if missing:
        out["normals"] = vertex_normals(out)
    return out


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
