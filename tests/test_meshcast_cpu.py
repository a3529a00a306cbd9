"""CPU-side checks of the mesh cast (nerf_fl_amd.raycast, csrc/nfl_meshcast.hip): the symbols and constants are in _lib's
tables and the header, which gains no struct; the two C entry points refuse bad arguments before any launch; the module
stands beside meshdist.py; the numpy restatement (tests/meshcast_ref.py), which the GPU tests hold the kernels to bit for bit,
is checked on hand cases whose expected numbers are written out; THE CONTRACT -- the walk returns the bits of trying every
triangle -- is checked on the restatement for every cell size and origin; the occlusion on scenes whose openness is known.
No kernel is launched."""
import os
import re

import numpy as np
import pytest

import meshcast_ref as cref
import meshdist_ref as dref
from abi_probe import HEADER, L, declared, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL = -1
INF, NAN = np.inf, np.nan


# ---- tables, sources and refusals --------------------------------------------------------------------------------------------

def test_the_tables_and_the_header_name_the_new_entry_points_and_no_new_struct():
    names = [s[0] for s in _lib.SYMBOLS]
    assert "nfl_mesh_cast" in names and "nfl_mesh_occlusion" in names
    assert {"nfl_mesh_cast", "nfl_mesh_occlusion"} <= set(declared()["functions"])
    constants = probe()["constants"]
    assert (constants["NFL_CAST_FIRST"], constants["NFL_CAST_ANY"]) == (0, 1) == (cref.FIRST, cref.ANY)
    assert _lib.CAST_MODES == {"first": 0, "any": 1} and _lib.CONSTANTS["NFL_CAST_ANY"] == 1
    assert len(declared()["structs"]) == 42 == len(_lib.STRUCTS)
    text = open(HEADER).read()
    assert "#define NFL_ABI_VERSION 10\n" in text and _lib.NFL_ABI_VERSION == 10
    assert text.index("---- registration:") < text.index("---- mesh cast:") < text.index("---- hierarchical sampling")


def test_the_unit_is_built_with_the_common_flags():
    make = open(os.path.join(ROOT, "nerf_fl_amd", "csrc", "Makefile")).read()
    assert "nfl_meshcast.o" in make.split("all:")[0]                       # in OBJS
    assert re.search(r"^nfl_meshcast\.o:.*nfl_geom\.h.*nfl_geom_layout\.h.*nfl_trigrid\.h", make, flags=re.M)
    assert re.search(r"^nfl_meshdist\.o:.*nfl_geom\.h.*nfl_geom_layout\.h.*nfl_trigrid\.h", make, flags=re.M)
    assert len(re.findall(r"^.*nfl_trigrid\.h", make, flags=re.M)) == 3      # those two lines and a comment: no other unit compiles it
    assert "-ffp-contract=off" in re.search(r"^CXXFLAGS = .*$", make, flags=re.M).group(0)
    for unit in ("nfl_meshcast", "nfl_meshdist"):                           # no recipe of its own: the common rule builds it
        assert not re.search(rf"^{unit}\.o:.*\n\t", make, flags=re.M)
    csrc = os.path.join(ROOT, "nerf_fl_amd", "csrc")
    geom, shared, dist, cast = (open(os.path.join(csrc, n)).read()
                                for n in ("nfl_geom.h", "nfl_trigrid.h", "nfl_meshdist.hip", "nfl_meshcast.hip"))
    for piece in ("struct NdGrid", "nd_cellf(float", "nd_grid_ok(const", "nd_face(float"):      # the grid's pieces, once
        assert piece in geom and piece not in shared and piece not in dist and piece not in cast, piece
    # the view, the host check of the rows, the row read with its clamps and skips, the staged tile with its barriers: once
    for piece in ("struct NtMesh", "nt_rows_ok(const", "corner[9]", "usable[NT_TILE]", "r0 = r0 < 0 ? 0 : r0", "r1 = r1 > M.E ? M.E : r1",
                  "if (t < 0 || t >= M.T) continue", "ng_misaligned(off, 8)"):
        assert piece in shared and piece not in geom and piece not in dist and piece not in cast, piece
    assert shared.count("__syncthreads()") == 2 and "__syncthreads()" not in dist and "__syncthreads()" not in cast
    assert '#include "nfl_geom.h"' in shared
    for unit in (dist, cast):
        assert '#include "nfl_trigrid.h"' in unit and "nt_tiles(" in unit and "nt_row(" in unit and "nt_rows_ok(" in unit
        assert "_TILE" not in unit and "struct NcMesh" not in unit and "_try_row" not in unit
    others = [n for n in os.listdir(csrc) if n.endswith((".hip", ".h", ".cpp")) and n not in ("nfl_trigrid.h", "nfl_meshdist.hip", "nfl_meshcast.hip")]
    assert len(others) > 40 and not [n for n in others if "nfl_trigrid.h" in open(os.path.join(csrc, n)).read()]
    assert "nfl_mesh_closest_args a)" not in dist                             # the kernel takes the view, not the ABI struct by value


def _cast_args(grid=True):
    a = dict(d_rays=0x1000, n_rays=50, d_vertices=0x2000, d_triangles=0x3000, n_vertices=30, n_triangles=10, d_offsets=None,
             d_entries=None, n_entries=0, lo_x=0.0, lo_y=0.0, lo_z=0.0, cell=0.0, nx=0, ny=0, nz=0, mode=0, d_t=0x6000,
             d_triangle=0x7000, d_bary=0x8000, d_point=0x9000)
    if grid:
        a.update(d_offsets=0x4000, d_entries=0x5000, n_entries=20, lo_x=-1.0, lo_y=-1.0, lo_z=-1.0, cell=0.5, nx=4, ny=4, nz=4)
    return a


def test_cast_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    call = lambda a: L.nfl_mesh_cast(*a.values(), None)
    for grid in (True, False):
        for field, bad in (("d_rays", None), ("d_rays", 0x1002), ("n_rays", -1), ("n_rays", 1 << 31), ("d_vertices", None),
                           ("d_triangles", None), ("d_vertices", 0x2001), ("d_triangles", 0x3002), ("n_vertices", -1),
                           ("n_triangles", -1), ("n_vertices", 1 << 31), ("n_triangles", (2 ** 31 - 1) // 3 + 1), ("mode", 2),
                           ("mode", -1), ("d_t", None), ("d_t", 0x6002), ("d_triangle", 0x7001), ("d_bary", 0x8002),
                           ("d_point", 0x9003)):
            a = _cast_args(grid)
            a[field] = bad
            assert call(a) == EINVAL, (grid, field, bad)
        a = _cast_args(grid)                                                  # no ray: NFL_OK without a launch
        a["n_rays"] = 0
        assert call(a) == 0
    for field, bad in (("cell", 0.0), ("cell", -1.0), ("cell", NAN), ("cell", INF), ("d_offsets", 0x4004), ("d_entries", None),
                       ("d_entries", 0x5002), ("n_entries", -1), ("n_entries", 1 << 31), ("nx", 0), ("ny", 65536), ("nz", -1),
                       ("lo_x", NAN), ("lo_y", INF), ("lo_z", -INF)):
        a = _cast_args()
        a[field] = bad
        assert call(a) == EINVAL, (field, bad)
    a = _cast_args()
    a.update(nx=1024, ny=1024, nz=1025)                                       # cells above 2^30
    assert call(a) == EINVAL
    # brute mode with the box of a grid: the box is checked as a grid's; all zeros means none
    a = _cast_args()
    a.update(d_offsets=None, d_entries=None, n_entries=0, n_rays=0)
    assert call(a) == 0
    for field, bad in (("cell", 0.0), ("nx", 0), ("lo_x", NAN)):
        b = dict(a)
        b[field] = bad
        assert call(b) == EINVAL, (field, bad)


def _occ_args():
    return dict(d_points=0x1000, d_normals=0x1100, n=50, d_vertices=0x2000, d_triangles=0x3000, n_vertices=30, n_triangles=10,
                d_offsets=0x4000, d_entries=0x5000, n_entries=20, lo_x=-1.0, lo_y=-1.0, lo_z=-1.0, cell=0.5, nx=4, ny=4, nz=4,
                n_directions=64, radius=INF, bias=1e-3, seed=7, d_hits=0x6000, d_open=0x7000)


def test_occlusion_refuses_before_any_launch(L):
    call = lambda a: L.nfl_mesh_occlusion(*a.values(), None)
    for field, bad in (("d_points", None), ("d_points", 0x1002), ("d_normals", None), ("d_normals", 0x1101), ("n", -1), ("n", 1 << 31),
                       ("d_vertices", None), ("d_triangles", None), ("d_vertices", 0x2001), ("d_triangles", 0x3002),
                       ("n_vertices", -1), ("n_triangles", -1), ("n_vertices", 1 << 31), ("d_offsets", None), ("d_offsets", 0x4004),
                       ("d_entries", None), ("d_entries", 0x5002), ("n_entries", -1), ("n_entries", 1 << 31), ("cell", 0.0),
                       ("cell", NAN), ("cell", INF), ("nx", 0), ("ny", 65536), ("lo_z", NAN), ("n_directions", 0),
                       ("n_directions", 4097), ("n_directions", -3), ("radius", 0.0), ("radius", -1.0), ("radius", NAN),
                       ("bias", -1e-3), ("bias", NAN), ("bias", INF), ("d_hits", None), ("d_hits", 0x6002), ("d_open", None),
                       ("d_open", 0x7001)):
        a = _occ_args()
        a[field] = bad
        assert call(a) == EINVAL, (field, bad)
    a = _occ_args()
    a["n"] = 0
    assert call(a) == 0
    a.update(n_directions=4096, bias=0.0, radius=0.25)
    assert call(a) == 0


def test_the_module_stands_beside_meshdist():
    pkg = os.path.join(ROOT, "nerf_fl_amd")
    source = open(os.path.join(pkg, "raycast.py")).read()
    assert "_lib.check(" not in source and "C.byref(" not in source and "import ctypes" not in source
    assert ".item()" not in source and ".tolist()" not in source and ".cpu()" not in source
    assert "registration" not in re.sub(r'""".*?"""', "", source, flags=re.S)        # nothing of the ICP module, private or public
    for helper in ("_call", "_f32", "_is", "_mesh_tensors", "_on_device", "_positive", "_ptr", "_seed"):
        assert re.search(rf"^from \.geometry\._call import .*\b{helper}\b", source, flags=re.M), helper
    assert re.search(r"^from \.meshdist import .*\b_mesh_or_grid\b", source, flags=re.M) and "def _target" not in source
    sources = {n: open(os.path.join(pkg, n)).read() for n in ("meshdist.py", "registration.py", "raycast.py")}
    call = open(os.path.join(pkg, "geometry", "_call.py")).read()
    assert call.count("_lib.check(") == 2 and call.count("rendering._stream()") == 2      # _launch and _call, side by side
    for n, text in sources.items():
        assert "_lib.check(" not in text and "rendering." not in text and "def _f32" not in text and "def _call" not in text, n
        assert "2 ** 64" not in text and "np.float32(" not in text, n          # the seed check and the fp32 rounding, once
    everything = "".join(open(os.path.join(d, n)).read() for d, _, names in os.walk(pkg) for n in names if n.endswith(".py"))
    assert everything.count("def _f32(") == 1 == call.count("def _f32(") and call.count("2 ** 64") == 1
    assert everything.count("def _mesh_or_grid(") == 1 == sources["meshdist.py"].count("def _mesh_or_grid(")
    assert everything.count("def _finite_box(") == 1 and everything.count("def read_ply(") == 1
    assert "def _grid_or_mesh" not in everything
    assert sorted(n for n in os.listdir(os.path.join(pkg, "geometry")) if n.endswith(".py")) == [
        "__init__.py", "_call.py", "files.py", "images.py", "lattice.py", "mesh.py", "occupancy.py"]
    from nerf_fl_amd import fusion, geometry, meshdist, raycast, registration
    assert raycast.__all__ == ["cast_rays", "vertex_occlusion", "clip_rays_to_mesh", "MeshBand"]
    assert len(geometry.__all__) == 24 and len(fusion.__all__) == 6
    assert meshdist.__all__ == ["triangle_grid", "closest_on_mesh", "sample_surface", "mesh_distance", "read_ply"]
    assert registration.__all__ == ["fit_transform", "transform_points", "transform_mesh", "register_mesh", "registered_distance"]
    assert "usual practice" in raycast.vertex_occlusion.__doc__ and "NOT a measured" in raycast.vertex_occlusion.__doc__
    assert "render_mesh(mesh" in raycast.vertex_occlusion.__doc__ and "write_ply" in raycast.vertex_occlusion.__doc__
    evl = open(os.path.join(pkg, "eval.py")).read()
    assert "isinstance(grid, MeshBand) else geometry.clip_rays(grid, rays)" in evl


def test_bad_python_arguments_are_refused_before_any_tensor_is_looked_at():
    from nerf_fl_amd import raycast
    for bad in (dict(mode="last"), dict(method="bvh"), dict(mode=None)):
        with pytest.raises(ValueError):
            raycast.cast_rays(None, None, **bad)
    for bad in (dict(rays=0), dict(rays=4097), dict(rays=2.5), dict(rays=True), dict(radius=0.0), dict(radius=-1.0),
                dict(radius=NAN), dict(bias=-1.0), dict(bias=NAN), dict(bias=INF), dict(seed=-1), dict(seed=2 ** 64),
                dict(points=0), dict(normals=0), dict(grid=0)):
        with pytest.raises(ValueError):
            raycast.vertex_occlusion(None, **bad)
    for bad in (-1.0, NAN, INF):
        with pytest.raises(ValueError):
            raycast.clip_rays_to_mesh(None, None, bad)
        with pytest.raises(ValueError):
            raycast.MeshBand(None, bad)


# ---- the restatement: hand cases ---------------------------------------------------------------------------------------------

TRI = F([[0, 0, 0], [1, 0, 0], [0, 1, 0]])
ONE = [[0, 1, 2]]


def _ray(o, d, near=0.0, far=INF):
    return F([list(o) + list(d) + [near, far]])


def test_a_ray_through_the_interior_through_a_vertex_and_from_the_triangle_itself():
    got = cref.cast(_ray((0.25, 0.25, 1), (0, 0, -1)), TRI, ONE)
    assert got["t"].tolist() == [1.0] and got["triangle"].tolist() == [0]
    assert got["bary"].tolist() == [[0.5, 0.25, 0.25]] and got["point"].tolist() == [[0.25, 0.25, 0.0]]
    assert all(got[k].dtype == F for k in ("t", "bary", "point")) and got["triangle"].dtype == np.int32
    got = cref.cast(_ray((0.25, 0.25, 1), (0, 0, -4)), TRI, ONE)           # t is the ray's own parameter
    assert got["t"].tolist() == [0.25] and got["point"].tolist() == [[0.25, 0.25, 0.0]]
    got = cref.cast(_ray((0.25, 0.25, -2), (0, 0, 1)), TRI, ONE)           # from behind: both faces hit
    assert got["t"].tolist() == [2.0] and got["triangle"].tolist() == [0]
    got = cref.cast(_ray((1, 0, 2), (0, 0, -1)), TRI, ONE)                  # through the corner b: u = 1, v = 0
    assert got["t"].tolist() == [2.0] and got["bary"].tolist() == [[0, 1, 0]] and got["point"].tolist() == [[1, 0, 0]]
    got = cref.cast(_ray((0.25, 0.25, 0), (0, 0, 1)), TRI, ONE)             # starting on the triangle with near = 0
    assert got["t"].tolist() == [0.0] and got["triangle"].tolist() == [0] and got["point"].tolist() == [[0.25, 0.25, 0.0]]
    assert cref.cast(_ray((0.25, 0.25, 1), (0, 0, -1)), TRI, ONE, mode=cref.ANY)["t"].tolist() == [0.0]
    assert cref.cast(_ray((0.75, 0.75, 1), (0, 0, -1)), TRI, ONE, mode=cref.ANY)["t"].tolist() == [INF]     # u + v > 1


def test_along_a_shared_edge_the_lower_index_answers():
    sq = dref.square()
    rays = np.concatenate([_ray((0.5, 0.5, 1), (0, 0, -1)), _ray((0.25, 0.25, -3), (0, 0, 1)), _ray((0.9, 0.1, 1), (0, 0, -1)),
                           _ray((0.1, 0.9, 1), (0, 0, -1))])
    got = cref.cast(rays, sq["vertices"], sq["triangles"])
    assert got["triangle"].tolist() == [0, 0, 0, 1] and got["t"].tolist() == [1.0, 3.0, 1.0, 1.0]
    assert got["bary"][0].tolist() == [0.5, 0.0, 0.5]                       # triangle (0, 1, 2): on its edge 0-2
    got = cref.cast(rays, sq["vertices"], sq["triangles"][::-1])             # the index decides, not the triangle
    assert got["triangle"].tolist() == [0, 0, 1, 0] and got["bary"][0].tolist() == [0.5, 0.5, 0.0]


def test_a_parallel_ray_misses_and_near_and_far_cut_the_hit_off():
    for o, d in (((-1, 0.25, 0), (1, 0, 0)), ((-1, 0.25, 0.5), (1, 0, 0)), ((0.2, 0.2, 0), (0.1, 0.3, 0))):    # in the plane, and beside it
        got = cref.cast(_ray(o, d), TRI, ONE)
        assert got["t"].tolist() == [INF] and got["triangle"].tolist() == [-1]
        assert np.isnan(got["bary"]).all() and np.isnan(got["point"]).all()
    o, d = (0.25, 0.25, 1), (0, 0, -1)                                      # the hit lies at t = 1
    for near, far, hit in ((1.5, INF, False), (0.0, 0.5, False), (1.0, 1.0, True), (-INF, INF, True), (1.0000001, 2.0, False),
                           (0.0, 0.99999994, False), (2.0, 1.0, False)):
        assert (cref.cast(_ray(o, d, near, far), TRI, ONE)["triangle"][0] == 0) == hit, (near, far)
    assert cref.cast(_ray(o, (0, 0, 1)), TRI, ONE)["triangle"].tolist() == [-1]      # behind the origin: t = -1 < near
    assert cref.cast(_ray(o, (0, 0, 1), -2.0, 0.0), TRI, ONE)["t"].tolist() == [-1.0]
    for bad in (_ray((NAN, 0, 1), d), _ray(o, (0, INF, -1)), _ray(o, (0, 0, 0)), _ray(o, d, NAN, INF), _ray(o, d, 0.0, NAN)):
        assert cref.cast(bad, TRI, ONE)["triangle"].tolist() == [-1] and not cref.valid(bad)[0]


def test_degenerate_and_unusable_triangles_are_never_hit():
    ver = F([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [NAN, 0, 0], [0.5, 0.5, 0]])
    ray = _ray((0.25, 0.25, 1), (0, 0, -1))
    assert cref.cast(ray, ver, [[0, 1, 2]])["triangle"].tolist() == [-1]     # collinear: det = 0
    assert cref.cast(ray, ver, [[5, 5, 5]])["triangle"].tolist() == [-1]     # a point
    tri = [[4, 1, 3], [0, 1, 6], [0, 1, -1], [0, 1, 2], [0, 1, 3]]          # a NaN corner, two out of range, a line, and one triangle
    assert dref.usable(ver, tri).tolist() == [False, False, False, True, True]
    got = cref.cast(ray, ver, tri)
    assert got["triangle"].tolist() == [4] and got["t"].tolist() == [1.0]
    none = cref.cast(ray, ver[:0], np.zeros((0, 3), np.int32))
    assert none["triangle"].tolist() == [-1] and none["t"].tolist() == [INF]


def test_a_hit_outside_the_box_is_refused_with_the_box_and_accepted_without():
    ver = F([[0, 0, 0], [4, 0, 0], [0, 4, 0]])
    lo, cell, dims = (0.0, 0.0, -1.0), 1.0, [1, 1, 2]
    box = cref.box_of(lo, cell, dims)
    assert box[0].tolist() == [0, 0, -1] and box[1].tolist() == [1, 1, 1]
    rays = np.concatenate([_ray((2, 1, 1), (0, 0, -1)), _ray((0.5, 0.25, 1), (0, 0, -1)), _ray((1, 1, 3), (0, 0, -1))])
    assert cref.cast(rays, ver, ONE)["triangle"].tolist() == [0, 0, 0]
    assert cref.cast(rays, ver, ONE, box)["triangle"].tolist() == [-1, 0, 0]   # the third: on the box's corner, which is closed
    got, _ = cref.cast_grid(rays, ver, ONE, lo, cell, dims)
    assert got["triangle"].tolist() == [-1, 0, 0] and got["t"].tolist() == [INF, 1.0, 3.0]


def test_the_consistency_condition_lets_grazing_hits_through():
    """A triangle in the plane y = 1e-3 z, met head-on and at a slope of 1.2e-3 to its plane: both are hits, at the ray's
    point to within the tolerance -- the condition is there for conditioning far beyond this."""
    ver = F([[0, 0, 0], [1, 0, 0], [0, 1e-3, 1]])
    assert cref.cast(_ray((0.3, -2, 0.5), (0, 1, 0)), ver, ONE)["triangle"].tolist() == [0]
    got = cref.cast(_ray((0.3, 1e-3, -2), (0, -2e-4, 1)), ver, ONE)
    assert got["triangle"].tolist() == [0] and abs(got["t"][0] - 2.5) < 1e-5
    assert np.abs(got["point"][0] - F([0.3, 5e-4, 0.5])).max() < 1e-6 and np.abs(got["bary"][0] - F([0.2, 0.3, 0.5])).max() < 1e-5


# ---- THE CONTRACT on the restatement ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soup():
    ver, tri = cref.soup40()
    return dict(ver=ver, tri=tri, rays=cref.soup_rays(ver, tri))


def test_the_rays_are_of_every_kind(soup):
    rays = soup["rays"]
    got = cref.cast(rays, soup["ver"], soup["tri"])
    hits = got["triangle"] >= 0
    assert 380 <= len(rays) <= 460 and 60 <= hits.sum() <= len(rays) - 100
    assert {36, 37, 38} <= set(got["triangle"].tolist()) and 39 not in got["triangle"]        # the square, and the doubled one
    assert (~cref.valid(rays)).sum() == 6 and np.isinf(rays[:, 7]).sum() > 300 and (rays[:, 3:6] == 0).sum() > 80


@pytest.mark.parametrize("name,lo,cell,dims", cref.configs(), ids=[f"{n[0]}-{n[1]:.3g}" for n, _, _, _ in cref.configs()])
def test_the_walk_returns_the_bits_of_trying_every_triangle(soup, name, lo, cell, dims):
    lo32, cell32 = [float(F(x)) for x in lo], float(F(cell))
    box = cref.box_of(lo32, cell32, dims)
    for mode in (cref.FIRST, cref.ANY):
        brute = cref.cast(soup["rays"], soup["ver"], soup["tri"], box, mode)
        grid, most = cref.cast_grid(soup["rays"], soup["ver"], soup["tri"], lo, cell, dims, mode)
        for k in brute:
            assert grid[k].dtype == brute[k].dtype and grid[k].tobytes() == brute[k].tobytes(), (name, mode, k)
    assert (brute["t"] == 0).sum() >= 50
    assert most <= 9 * max(dims)                                              # at most 3 x 3 cells a slab here


def test_the_walk_far_from_the_origin_of_coordinates():
    """The same scene moved by 1000 along every axis: the tolerances grow with the coordinates, the answer stays brute's."""
    ver, tri = cref.soup40()
    ver = (ver + F(1000)).astype(F)
    rays = cref.soup_rays(ver - F(1000), tri)
    rays[:, :3] += F(1000)
    lo, cell, dims = (996.9, 997.7, 992.3), 0.25, cref.dims_of(0.25)
    box = cref.box_of([float(F(x)) for x in lo], cell, dims)
    brute = cref.cast(rays, ver, tri, box)
    grid, _ = cref.cast_grid(rays, ver, tri, lo, cell, dims)
    assert (brute["triangle"] >= 0).sum() >= 50
    for k in brute:
        assert grid[k].tobytes() == brute[k].tobytes(), k


# ---- occlusion on scenes whose answer is known ---------------------------------------------------------------------------------

def _open(scene, K, seed=0, radius=INF, bias=1e-3):
    return cref.occlusion(scene["point"], scene["normal"], scene["ver"], scene["tri"], scene["lo"], scene["cell"], scene["dims"],
                          K, radius, bias, seed)


def test_directions_are_unit_vectors_of_the_hemisphere_cosine_weighted():
    for n in (F([0, 0, 1]), F([0, 0, -1]), F([0.36, 0.48, 0.8]), F([-0.6, 0, -0.8]), F([1, 0, 0])):
        d = cref.directions(3, 5, n, 4096)
        assert d.dtype == F and d.shape == (4096, 3)
        assert np.abs(np.linalg.norm(d.astype(np.float64), axis=1) - 1).max() < 1e-6
        cos = d.astype(np.float64) @ n.astype(np.float64)
        assert cos.min() > 0 and abs(cos.mean() - 2 / 3) <= 5 * np.sqrt((1 / 18) / 4096)          # E cos = 2/3, var = 1/2 - 4/9
    assert not np.array_equal(cref.directions(3, 5, n, 64), cref.directions(4, 5, n, 64))
    assert not np.array_equal(cref.directions(3, 5, n, 64), cref.directions(3, 6, n, 64))
    assert np.array_equal(cref.directions(3, 5, n, 64), cref.directions(3, 5, n, 4096)[:64])


def test_open_sky_a_sealed_box_and_the_foot_of_a_wall():
    hits, opn = _open(cref.scene_square(), 256)
    assert hits.tolist() == [0] and opn.tolist() == [1.0] and opn.dtype == F and hits.dtype == np.int32
    hits, opn = _open(cref.scene_box(), 256)
    assert hits.tolist() == [256] and opn.tolist() == [0.0]
    assert _open(cref.scene_box(), 256, radius=0.5)[1].tolist() == [1.0]      # the nearest wall is 0.7 away
    hits, opn = _open(cref.scene_wall(), 4096)
    assert abs(float(opn[0]) - 0.5) <= 5 * np.sqrt(0.25 / 4096) and hits[0] == 4096 - round(float(opn[0]) * 4096)
    other = _open(cref.scene_wall(), 4096, seed=1)[0]
    assert other[0] != hits[0] and abs(int(other[0]) - 2048) <= 5 * 32


def test_a_point_that_is_no_point_has_no_openness():
    s = cref.scene_square()
    pts = F([[0, 0, 0], [NAN, 0, 0], [0, 0, 0], [0, 0, 0]])
    nrm = F([[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, INF, 1]])
    hits, opn = cref.occlusion(pts, nrm, s["ver"], s["tri"], s["lo"], s["cell"], s["dims"], 16, INF, 1e-3, 0)
    assert hits.tolist() == [0, -1, -1, -1] and opn[0] == 1.0 and np.isnan(opn[1:]).all()
