"""CPU-side checks of the geometry feature (nerf_fl_amd.geometry, csrc/nfl_surface.hip): the numpy restatement of the
extraction (tests/geometry_ref.py), which the GPU tests hold the kernels to, is itself checked on an analytic volume;
write_ply round-trips; the three C entry points size their scratch and refuse bad arguments.  No kernel is launched."""
import ctypes as C
import os

import numpy as np
import pytest

import geometry_ref as gr
from abi_probe import L  # noqa: F401  (a fixture)

R0, N = 0.6, 24


@pytest.fixture(scope="module")
def sphere():
    lat, lo, sp = gr.sphere_lattice(N, R0)
    return gr.extract(lat, 0.0, lo, sp), float(sp[0])


def _edges(tri):
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)


def test_case_table_covers_every_tetrahedron_case():
    assert len(gr.TRI_TABLE) == 6 and all(len(t) == 16 for t in gr.TRI_TABLE)
    for t in range(6):
        cs = gr.tet_corners(t)
        assert cs[0] == 0 and cs[3] == 7 and cs[0] & cs[1] == cs[0] and cs[1] & cs[2] == cs[1]
        for k in range(16):
            n_in = bin(k).count("1")
            assert len(gr.TRI_TABLE[t][k]) == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[n_in]
            for tri in gr.TRI_TABLE[t][k]:
                for code in tri:        # an edge of THIS tetrahedron whose ends differ in the case
                    lo, hi = code >> 3, (code >> 3) | (code & 7)
                    assert lo in cs and hi in cs and lo != hi
                    assert ((k >> cs.index(lo)) ^ (k >> cs.index(hi))) & 1


def test_sphere_is_a_closed_manifold(sphere):
    mesh, _ = sphere
    tri = mesh["triangles"]
    V, T = len(mesh["vertices"]), len(tri)
    assert V > 0 and tri.min() == 0 and tri.max() == V - 1
    e = _edges(tri)
    _, n_directed = np.unique(e, axis=0, return_counts=True)
    assert (n_directed == 1).all()                                  # consistently wound: no directed edge twice
    und, n_und = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    assert (n_und == 2).all()                                       # every undirected edge belongs to exactly two triangles
    assert V - len(und) + T == 2


def test_sphere_faces_outwards(sphere):
    mesh, _ = sphere
    v, tri = mesh["vertices"].astype(np.float64), mesh["triangles"]
    n = np.cross(v[tri[:, 1]] - v[tri[:, 0]], v[tri[:, 2]] - v[tri[:, 0]])
    assert ((n * v[tri].mean(axis=1)).sum(axis=1) > 0).all()
    # the vertex normals are unit and point outwards too
    assert np.abs(np.linalg.norm(mesh["normals"].astype(np.float64), axis=1) - 1).max() <= 1e-6
    assert ((mesh["normals"] * v).sum(axis=1) > 0).all()


def test_sphere_vertices_lie_on_the_sphere(sphere):
    """r0 - |p| is concave with second derivative at most 1 / |p| along any line; over an edge of length L <= sqrt(3) h
    linear interpolation errs by at most L^2 / (8 |p|_min) in value, |p|_min >= r0 - sqrt(3) h on a crossing edge, and
    the value is the distance to the sphere: ||v| - r0| <= 3 h^2 / (8 (r0 - sqrt(3) h)).  fp32 slack: the lattice values
    (|v| <= 2) and the interpolation carry a few ulp of 2."""
    mesh, h = sphere
    bound = 3 * h * h / (8 * (R0 - np.sqrt(3) * h)) + 16 * np.finfo(np.float32).eps
    err = np.abs(np.linalg.norm(mesh["vertices"].astype(np.float64), axis=1) - R0).max()
    print(f"sphere {N}^3: worst | |v| - r0 | = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


def _components(n, tri):
    parent = list(range(n))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for a, b, c in tri:
        parent[find(a)] = find(b)
        parent[find(b)] = find(c)
    return np.array([find(i) for i in range(n)])


def _assert_closed_and_outward(lat, what, each_component):
    """The restatement's mesh of a lattice whose border is outside: closed (every undirected edge in two triangles),
    consistently wound (no directed edge twice) and facing outwards (positive enclosed volume; per connected component
    where the inside region cannot enclose a pocket of outside)."""
    nz, ny, nx = lat.shape
    mesh = gr.extract(lat, 0.0, (0, 0, 0), (1, 1, 1))
    v, tri = mesh["vertices"].astype(np.float64), mesh["triangles"].astype(np.int64)
    assert len(tri) > 0, what
    e = _edges(tri)
    _, n_directed = np.unique(e, axis=0, return_counts=True)
    assert (n_directed == 1).all(), what
    _, n_und = np.unique(np.sort(e, axis=1), axis=0, return_counts=True)
    assert (n_und == 2).all(), what
    vol = np.einsum("ij,ij->i", v[tri[:, 0]], np.cross(v[tri[:, 1]], v[tri[:, 2]])) / 6.0
    if each_component:
        comp = _components(len(v), tri)[tri[:, 0]]
        for c in np.unique(comp):
            assert vol[comp == c].sum() > 0, what
    assert vol.sum() > 0, what
    return mesh


def test_every_corner_pattern_gives_a_closed_outward_surface():
    """The case table is shared by the restatement and the kernel (the kernel carries its printed copy), so comparing
    the two cannot see a wrong entry: each of the 256 patterns of a 2 x 2 x 2 block, surrounded by outside points,
    exercises every (tetrahedron, case) pair of the table, and a wrong edge or winding leaves a hole or a flipped
    triangle."""
    seen = set()
    for pattern in range(1, 256):
        lat = -np.ones((4, 4, 4), dtype=np.float32)
        for c in range(8):
            if (pattern >> c) & 1:
                lat[1 + ((c >> 2) & 1), 1 + ((c >> 1) & 1), 1 + (c & 1)] = 1.0
        _assert_closed_and_outward(lat, f"pattern {pattern}", each_component=True)
        for t in range(6):
            cs = gr.tet_corners(t)
            seen.add((t, sum(((pattern >> cs[j]) & 1) << j for j in range(4))))
    assert len(seen) == 6 * 16                         # every case of every tetrahedron


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_random_lattices_give_closed_consistent_surfaces(seed):
    rng = np.random.default_rng(seed)
    lat = -np.ones((7, 8, 9), dtype=np.float32)
    lat[1:-1, 1:-1, 1:-1] = rng.standard_normal((5, 6, 7)).astype(np.float32)
    _assert_closed_and_outward(lat, f"random {seed}", each_component=False)


def _read_ply(path):
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    lines = head.decode("ascii").split("\n")
    assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
    n_v = int(next(l for l in lines if l.startswith("element vertex")).split()[2])
    n_f = int(next(l for l in lines if l.startswith("element face")).split()[2])
    kinds = {"float": "<f4", "uchar": "u1"}
    props = [l.split() for l in lines if l.startswith("property") and "list" not in l]
    vdt = np.dtype([(p[2], kinds[p[1]]) for p in props])
    fdt = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
    assert len(body) == n_v * vdt.itemsize + n_f * fdt.itemsize
    v = np.frombuffer(body, dtype=vdt, count=n_v)
    f = np.frombuffer(body, dtype=fdt, count=n_f, offset=n_v * vdt.itemsize)
    return v, f


@pytest.mark.parametrize("with_colors", [False, True])
def test_write_ply_round_trip(tmp_path, sphere, with_colors):
    from nerf_fl_amd.geometry import write_ply
    mesh, _ = sphere
    V = len(mesh["vertices"])
    colors = np.random.default_rng(3).uniform(0, 1, size=(V, 3)).astype(np.float32) if with_colors else None
    path = os.path.join(tmp_path, "m.ply")
    write_ply(path, mesh, colors)
    v, f = _read_ply(path)
    assert np.array_equal(np.stack([v["x"], v["y"], v["z"]], 1), mesh["vertices"])
    assert np.array_equal(np.stack([v["nx"], v["ny"], v["nz"]], 1), mesh["normals"])
    assert (f["n"] == 3).all() and np.array_equal(f["v"], mesh["triangles"])
    if with_colors:
        got = np.stack([v["red"], v["green"], v["blue"]], 1)
        assert np.array_equal(got, np.rint(colors.astype(np.float64) * 255).astype(np.uint8))
    else:
        assert "red" not in v.dtype.names


def test_write_ply_rejects_bad_meshes(tmp_path, sphere):
    from nerf_fl_amd.geometry import write_ply
    mesh, _ = sphere
    bad = dict(mesh, triangles=mesh["triangles"] + 1)
    with pytest.raises(ValueError):
        write_ply(os.path.join(tmp_path, "m.ply"), bad)
    with pytest.raises(ValueError):
        write_ply(os.path.join(tmp_path, "m.ply"), mesh, np.zeros((3, 3), np.float32))


def test_geometry_rejects_host_inputs():
    import torch
    from nerf_fl_amd import geometry
    with pytest.raises(RuntimeError):
        geometry.extract_surface(torch.zeros(4, 4, 4), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(RuntimeError):
        geometry.surface_colors(None, {}, torch.zeros(4, 3), torch.zeros(4, 3))
    with pytest.raises(ValueError):
        geometry.lattice_points((0, 0, 0), (1, 1, 1), (4, 1, 4), "cpu")
    with pytest.raises(ValueError):
        geometry.lattice_points((0, 0, 0), (1, 0, 1), (4, 4, 4), "cpu")
    p = geometry.lattice_points((-1, 0, 1), (1, 3, 2), (5, 4, 3), "cpu")
    assert p.shape == (3, 4, 5, 3)
    assert p[0, 0, 0].tolist() == [-1, 0, 1] and p[2, 3, 4].tolist() == [1, 3, 2]


# ---- the C entry points, without a GPU (structs and signatures: tests/test_abi_cpu.py)

def test_surface_symbols_exported(L):
    for name in ("nfl_surface_bytes", "nfl_surface_count", "nfl_surface_emit"):
        assert hasattr(L, name)


def test_surface_bytes(L):
    assert L.nfl_surface_bytes(1, 8, 8) == 0 and L.nfl_surface_bytes(8, 1, 8) == 0 and L.nfl_surface_bytes(8, 8, 1) == 0
    assert L.nfl_surface_bytes(-4, 8, 8) == 0
    assert L.nfl_surface_bytes(1024, 1024, 1025) == 0               # more than 2^30 points
    assert L.nfl_surface_bytes(2, 65536, 2) == 0                    # rows are a grid dimension
    assert L.nfl_surface_bytes(2, 2, 2) == 8 * 4 + 4 * 16           # 8 point records, 4 slabs
    assert L.nfl_surface_bytes(1024, 1024, 1024) == 4 * 2 ** 30 + 4 * 2 ** 20 * 16
    last = 0
    for n in (2, 3, 24, 255, 256, 257, 512, 513):                   # monotone, also across the slab width
        b = L.nfl_surface_bytes(n, 9, 7)
        assert b > last and b >= 4 * n * 9 * 7
        assert L.nfl_surface_bytes(n, 10, 7) > b and L.nfl_surface_bytes(n, 9, 8) > b
        last = b


def test_surface_calls_validate_arguments(L):
    from nerf_fl_amd import _lib
    EINVAL, ESMALL = -1, -4
    assert L.nfl_surface_count(None, None) == EINVAL and L.nfl_surface_emit(None, None) == EINVAL

    def args(**kw):
        a = _lib.SurfaceArgs()
        a.d_lattice, a.d_scratch, a.d_totals = 64, 64, 64           # never dereferenced: every call below is refused
        a.nx, a.ny, a.nz = 8, 8, 8
        a.scratch_bytes = L.nfl_surface_bytes(8, 8, 8)
        a.d_vertices = a.d_normals = a.d_triangles = 64
        a.n_vertices, a.n_triangles = 10, 10
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for fn in (L.nfl_surface_count, L.nfl_surface_emit):
        assert fn(C.byref(args(d_lattice=None)), None) == EINVAL
        assert fn(C.byref(args(d_scratch=None)), None) == EINVAL
        assert fn(C.byref(args(d_scratch=68)), None) == EINVAL      # not 8-byte aligned
        assert fn(C.byref(args(nx=1)), None) == EINVAL
        assert fn(C.byref(args(ny=1)), None) == EINVAL
        assert fn(C.byref(args(nz=0)), None) == EINVAL
        assert fn(C.byref(args(nx=1024, ny=1024, nz=1025, scratch_bytes=1 << 40)), None) == EINVAL
        assert fn(C.byref(args(scratch_bytes=L.nfl_surface_bytes(8, 8, 8) - 1)), None) == ESMALL
        assert fn(C.byref(args(scratch_bytes=0)), None) == ESMALL
    assert L.nfl_surface_count(C.byref(args(d_totals=None)), None) == EINVAL
    emit = L.nfl_surface_emit
    assert emit(C.byref(args(n_vertices=2 ** 31)), None) == EINVAL                  # V beyond int32
    assert emit(C.byref(args(n_triangles=(2 ** 31 - 1) // 3 + 1)), None) == EINVAL   # 3 T beyond int32
    assert emit(C.byref(args(n_vertices=-1)), None) == EINVAL
    assert emit(C.byref(args(d_vertices=None)), None) == EINVAL
    assert emit(C.byref(args(d_normals=None)), None) == EINVAL
    assert emit(C.byref(args(d_triangles=None)), None) == EINVAL
    assert emit(C.byref(args(n_vertices=0, n_triangles=0, d_vertices=None, d_normals=None, d_triangles=None)), None) == 0
