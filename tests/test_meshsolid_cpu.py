"""CPU-side checks of the mesh solid queries (nerf_fl_amd.solid, csrc/nfl_meshcast.hip): the two symbols are in _lib's tables and
the header, which gains no struct; both C entry points refuse bad arguments before any launch; the module stands beside
raycast.py; the numpy restatement (tests/meshsolid_ref.py), which the GPU tests hold the kernels to, is checked on hand cases
whose expected numbers are written out; THE CONTRACT -- the count-mode walk returns the integers of trying every triangle -- is
checked on the restatement for every cell size and origin, and shown to fail without THE ONCE-ONLY RULE; the votes on closed
meshes whose inside is known.  No kernel is launched."""
import os
import re

import numpy as np
import pytest

import meshcast_ref as cref
import meshdist_ref as dref
import meshsolid_ref as sref
from abi_probe import HEADER, L, declared, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL = -1
INF, NAN = np.inf, np.nan


# ---- tables, sources and refusals --------------------------------------------------------------------------------------------

def test_the_tables_and_the_header_name_the_new_entry_points_and_no_new_struct():
    names = [s[0] for s in _lib.SYMBOLS]
    assert "nfl_mesh_crossings" in names and "nfl_mesh_inside" in names
    assert {"nfl_mesh_crossings", "nfl_mesh_inside"} <= set(declared()["functions"])
    assert len(declared()["structs"]) == 42 == len(_lib.STRUCTS)
    text = open(HEADER).read()
    assert "#define NFL_ABI_VERSION 10\n" in text and _lib.NFL_ABI_VERSION == 10
    assert text.index("---- mesh cast:") < text.index("---- mesh solid:") < text.index("---- hierarchical sampling")
    assert _lib.CAST_MODES == {"first": 0, "any": 1}                          # counting is no mode of the cast
    assert probe()["constants"]["NFL_SOLID_MAX_DIRECTIONS"] == 7 == _lib.SOLID_MAX_DIRECTIONS == len(sref.DIRECTIONS)


def test_the_directions_are_the_header_s_and_what_the_header_says_of_them():
    text = open(HEADER).read()
    table = re.search(r"#define NFL_SOLID_DIRECTIONS (.*?)\n[^ ]", text, flags=re.S).group(1)
    literals = re.findall(r"(-?\d+\.\d+)f", table)
    header = F([float(x) for x in literals]).reshape(7, 3)
    assert header.tobytes() == sref.DIRECTIONS.tobytes()
    primes = np.array(sref.PRIMES)
    assert len(set(primes.ravel().tolist())) == 21 and all(p > 1 and all(p % q for q in range(2, p)) for p in primes.ravel().tolist())
    assert (np.abs(sref.DIRECTIONS) == np.sqrt(primes.astype(np.float64)).astype(F)).all()      # none zero, none rational
    assert np.abs(sref.DIRECTIONS).argmax(axis=1).tolist() == [0, 1, 2, 0, 1, 2, 0]                # the major axes
    signs = {tuple(np.sign(d).astype(int).tolist()) for d in sref.DIRECTIONS}
    assert len(signs) == 7                                                    # seven of the eight octants
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    section = design[design.index("\n## 38. "):]
    assert all(x in section for x in literals)                                # the table is written out in DESIGN.md too


def test_the_kernels_live_in_the_cast_unit_and_share_its_walk():
    csrc = os.path.join(ROOT, "nerf_fl_amd", "csrc")
    cast = open(os.path.join(csrc, "nfl_meshcast.hip")).read()
    assert 'extern "C" int nfl_mesh_crossings(' in cast and 'extern "C" int nfl_mesh_inside(' in cast
    assert len(re.findall(r"^__device__ __forceinline__ void nc_walk\(", cast, flags=re.M)) == 1      # one walk, not a copy
    assert cast.count("nd_face(lm, G.cell, nm") == 1 and cast.count("nc_span(l1") == 1
    assert cast.count("nc_walk(R, B, M,") == 2                               # the answer's use of it, and the count's
    assert "__syncthreads()" not in cast and "_TILE" not in cast and "_try_row" not in cast
    assert not [n for n in os.listdir(csrc) if "solid" in n]                  # no new unit
    assert cast.count("nc_grid_args_ok(d_offsets, d_entries, n_entries, lo, cell, dims, false)") == 3


def _cross_args(grid=True):
    a = dict(d_rays=0x1000, n_rays=50, d_vertices=0x2000, d_triangles=0x3000, n_vertices=30, n_triangles=10, d_offsets=None,
             d_entries=None, n_entries=0, lo_x=0.0, lo_y=0.0, lo_z=0.0, cell=0.0, nx=0, ny=0, nz=0, d_count=0x6000)
    if grid:
        a.update(d_offsets=0x4000, d_entries=0x5000, n_entries=20, lo_x=-1.0, lo_y=-1.0, lo_z=-1.0, cell=0.5, nx=4, ny=4, nz=4)
    return a


def _inside_args(grid=True):
    a = _cross_args(grid)
    del a["d_count"]
    a = {("d_points" if k == "d_rays" else "n" if k == "n_rays" else k): v for k, v in a.items()}
    a.update(n_directions=3, d_votes=0x6001, d_inside=0x7003)                 # bytes: no alignment to ask for
    return a


MESH_REFUSALS = (("d_vertices", None), ("d_triangles", None), ("d_vertices", 0x2001), ("d_triangles", 0x3002), ("n_vertices", -1),
                 ("n_triangles", -1), ("n_vertices", 1 << 31), ("n_triangles", (2 ** 31 - 1) // 3 + 1))
GRID_REFUSALS = (("cell", 0.0), ("cell", -1.0), ("cell", NAN), ("cell", INF), ("d_offsets", 0x4004), ("d_entries", None),
                 ("d_entries", 0x5002), ("n_entries", -1), ("n_entries", 1 << 31), ("nx", 0), ("ny", 65536), ("nz", -1),
                 ("lo_x", NAN), ("lo_y", INF), ("lo_z", -INF))


def _refusals(call, args, own, count):
    """Every pointer is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    for grid in (True, False):
        for field, bad in own + MESH_REFUSALS:
            a = args(grid)
            a[field] = bad
            assert call(a) == EINVAL, (grid, field, bad)
        a = args(grid)                                                        # nothing to do: NFL_OK without a launch
        a[count] = 0
        assert call(a) == 0
    for field, bad in GRID_REFUSALS:
        a = args()
        a[field] = bad
        assert call(a) == EINVAL, (field, bad)
    a = args()
    a.update(nx=1024, ny=1024, nz=1025)                                       # cells above 2^30
    assert call(a) == EINVAL
    a = args()                                                                # brute mode with the box of a grid
    a.update(d_offsets=None, d_entries=None, n_entries=0)
    a[count] = 0
    assert call(a) == 0
    for field, bad in (("cell", 0.0), ("nx", 0), ("lo_x", NAN)):
        b = dict(a)
        b[field] = bad
        assert call(b) == EINVAL, (field, bad)


def test_crossings_refuses_before_any_launch(L):
    own = (("d_rays", None), ("d_rays", 0x1002), ("n_rays", -1), ("n_rays", 1 << 31), ("d_count", None), ("d_count", 0x6002))
    _refusals(lambda a: L.nfl_mesh_crossings(*a.values(), None), _cross_args, own, "n_rays")


def test_inside_refuses_before_any_launch(L):
    own = (("d_points", None), ("d_points", 0x1002), ("n", -1), ("n", 1 << 31), ("d_votes", None), ("n_directions", 0),
           ("n_directions", 2), ("n_directions", 4), ("n_directions", 6), ("n_directions", 8), ("n_directions", 9),
           ("n_directions", -1), ("n_directions", -3))
    call = lambda a: L.nfl_mesh_inside(*a.values(), None)
    _refusals(call, _inside_args, own, "n")
    for k in (1, 3, 5, 7):                                                    # the four that are served; d_inside may be absent
        a = _inside_args()
        a.update(n=0, n_directions=k, d_inside=None)
        assert call(a) == 0
    a = _cross_args()
    del a["d_count"]
    assert L.nfl_mesh_cast(*a.values(), 2, 0x6000, None, None, None, None) == EINVAL      # counting is no mode of the cast


def test_the_module_stands_beside_raycast():
    pkg = os.path.join(ROOT, "nerf_fl_amd")
    source = open(os.path.join(pkg, "solid.py")).read()
    assert "_lib.check(" not in source and "C.byref(" not in source and "ctypes" not in source and "rendering" not in source
    assert ".item()" not in source and ".tolist()" not in source and "numpy" not in source and "def _f32" not in source
    assert source.count(".cpu()") == 1 and "THE host read" in source.split(".cpu()")[1].split("\n")[0]
    code = re.sub(r'""".*?"""', "", source, flags=re.S)
    assert code.count(".cpu()") == 1 and code.split(".cpu()")[0].rsplit("\ndef ", 1)[1].startswith("volume_overlap(")
    for helper in ("_call", "_f32", "_is", "_mesh_tensors", "_on_device", "_positive", "_ptr"):
        assert re.search(rf"^from \.geometry\._call import .*\b{helper}\b", source, flags=re.M), helper
    assert re.search(r"^from \.meshdist import .*\b_mesh_or_grid\b", source, flags=re.M)
    assert re.search(r"^from \.raycast import _grid_args, _rays$", source, flags=re.M)
    assert code.count("triangle_grid(") == 1                                  # solid_lattice: one grid, both queries
    from nerf_fl_amd import solid
    assert solid.__all__ == ["count_crossings", "inside_mesh", "signed_distance", "solid_lattice", "remesh", "volume_overlap",
                             "mesh_volume"]


def test_bad_python_arguments_are_refused_before_any_tensor_is_looked_at():
    from nerf_fl_amd import solid
    with pytest.raises(ValueError):
        solid.count_crossings(None, None, method="bvh")
    for bad in (0, 2, 4, 6, 8, 9, -1, 3.0, True, None, "3"):
        for call in (lambda: solid.inside_mesh(None, None, directions=bad), lambda: solid.signed_distance(None, None, directions=bad),
                     lambda: solid.solid_lattice(None, (-1,) * 3, (1,) * 3, (9,) * 3, directions=bad),
                     lambda: solid.remesh(None, (-1,) * 3, (1,) * 3, (9,) * 3, directions=bad),
                     lambda: solid.volume_overlap(None, None, (-1,) * 3, (1,) * 3, (9,) * 3, directions=bad)):
            with pytest.raises(ValueError):
                call()
    for bad in (dict(method="bvh"), dict(max_distance=0.0), dict(max_distance=-1.0), dict(max_distance=NAN)):
        with pytest.raises(ValueError):
            solid.signed_distance(None, None, **bad)
    with pytest.raises(ValueError):
        solid.inside_mesh(None, None, method="bvh")
    for bad in (0.0, -0.1, NAN, INF):
        with pytest.raises(ValueError):
            solid.solid_lattice(None, (-1,) * 3, (1,) * 3, (9,) * 3, trunc=bad)
        with pytest.raises(ValueError):
            solid.remesh(None, (-1,) * 3, (1,) * 3, (9,) * 3, trunc=bad)
    for box in (dict(lo=(0, 0), hi=(1, 1, 1), res=(9, 9, 9)), dict(lo=(0, 0, 0), hi=(1, 1, 1), res=(9, 9, 1)),
                dict(lo=(0, 0, 0), hi=(1, 0, 1), res=(9, 9, 9)), dict(lo=(0, 0, NAN), hi=(1, 1, 1), res=(9, 9, 9))):
        for call in (lambda: solid.solid_lattice(None, **box), lambda: solid.remesh(None, **box),
                     lambda: solid.volume_overlap(None, None, **box)):
            with pytest.raises(ValueError):
                call()
    # |offset| must stay below trunc: 3 x the spacing 0.25 by default
    for bad in (dict(offset=0.75), dict(offset=-0.75), dict(offset=1.0), dict(offset=NAN), dict(offset=0.1, trunc=0.1)):
        with pytest.raises(ValueError):
            solid.remesh(None, (-1,) * 3, (1,) * 3, (9,) * 3, **bad)
    for call in (lambda: solid.mesh_volume(None), lambda: solid.mesh_volume({"vertices": 0}),
                 lambda: solid.inside_mesh(None, None), lambda: solid.count_crossings(None, {"triangles": 0})):
        with pytest.raises(ValueError):
            call()


# ---- the restatement: hand cases ---------------------------------------------------------------------------------------------

def _ray(o, d, near=0.0, far=INF):
    return F([list(o) + list(d) + [near, far]])


def _box_of(scene):
    return cref.box_of([float(F(x)) for x in scene["lo"]], float(F(scene["cell"])), scene["dims"])


def _both(ray, scene):
    """Brute force and the count-mode walk, which must agree."""
    brute = sref.crossings(ray, scene["ver"], scene["tri"], _box_of(scene))
    grid = sref.crossings_grid(ray, scene["ver"], scene["tri"], scene["lo"], scene["cell"], scene["dims"])
    assert brute.dtype == np.int32 == grid.dtype and brute.tolist() == grid.tolist()
    return brute.tolist()


def test_a_ray_through_the_sealed_box_counts_two_from_outside_and_one_from_inside():
    s = cref.scene_box()                                                      # [-1, 1]^3, every face two triangles split along y = z, ...
    assert _both(_ray((-3, 0.3, 0.1), (1, 0, 0)), s) == [2]
    assert _both(_ray((0, 0.3, 0.1), (1, 0, 0)), s) == [1]
    assert _both(_ray((-3, 0.3, 0.1), (-1, 0, 0)), s) == [0]                  # pointing away
    assert _both(_ray((-3, 0.3, 0.1), (1, 0, 0), 0.0, 3.0), s) == [1]         # far cuts the second wall off: t = 2 and 4
    assert _both(_ray((-3, 0.3, 0.1), (1, 0, 0), 2.5, INF), s) == [1]
    assert _both(_ray((-3, 0.3, 0.1), (1, 0, 0), 2.0, 4.0), s) == [2]         # the bounds are closed
    assert _both(_ray((-3, 0.3, 0.1), (4, 0, 0)), s) == [2]                   # t is the ray's own parameter
    assert sref.crossings(_ray((-3, 0.3, 0.1), (1, 0, 0)), s["ver"], s["tri"]).tolist() == [2]     # no box: the same
    for bad in (_ray((NAN, 0, 0), (1, 0, 0)), _ray((0, 0, 0), (0, 0, 0)), _ray((0, 0, 0), (1, 0, 0), 3.0, 2.0),
                _ray((0, 0, 0), (1, INF, 0)), _ray((0, 0, 0), (1, 0, 0), NAN, INF)):
        assert _both(bad, s) == [0]                                           # a ray that can hit nothing


def test_a_ray_along_a_box_diagonal_counts_every_triangle_at_the_corners():
    """Through a corner the ray test accepts every triangle that has the corner: in scene_box each of the three faces there
    touches it with both its triangles, so a corner counts 6 -- an even number from INSIDE, which is the known limit that
    the majority over the directions is there for (no direction of the table runs along a diagonal either)."""
    s = cref.scene_box()
    assert _both(_ray((-2, -2, -2), (1, 1, 1)), s) == [12]
    assert _both(_ray((0, 0, 0), (1, 1, 1)), s) == [6]
    assert _both(_ray((0, 0, 0), (-1, -1, -1)), s) == [6]
    # without THE ONCE-ONLY RULE the walk counts a triangle in every cell it reads that lists it
    assert sref.crossings_grid(_ray((-2, -2, -2), (1, 1, 1)), s["ver"], s["tri"], s["lo"], s["cell"], s["dims"], once=False).tolist() == [56]


def test_a_degenerate_or_unusable_triangle_never_counts():
    ver = F([[0, 0, 0], [1, 0, 0], [2, 0, 0], [0, 1, 0], [NAN, 0, 0], [0.5, 0.5, 0]])
    ray = _ray((0.25, 0.25, 1), (0, 0, -1))
    assert sref.crossings(ray, ver, [[0, 1, 2]]).tolist() == [0]              # collinear
    assert sref.crossings(ray, ver, [[5, 5, 5]]).tolist() == [0]              # a point
    tri = [[4, 1, 3], [0, 1, 6], [0, 1, -1], [0, 1, 2], [0, 1, 3], [0, 1, 3]]   # NaN, out of range twice, a line, one triangle twice
    assert sref.crossings(ray, ver, tri).tolist() == [2]                      # a triangle the mesh holds twice is two
    assert sref.crossings_grid(ray, ver, tri, (-0.5, -0.5, -0.5), 0.5, [6, 4, 4]).tolist() == [2]
    assert sref.crossings(ray, ver[:0], np.zeros((0, 3), np.int32)).tolist() == [0]


# ---- THE CONTRACT on the restatement ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def soup():
    ver, tri, rays, whole = sref.soup()
    return dict(ver=ver, tri=tri, rays=rays, whole=whole)


def test_the_rays_are_of_every_kind_and_near_and_far_take_crossings_away(soup):
    rays, n = soup["rays"], len(soup["whole"])
    count = sref.crossings(rays, soup["ver"], soup["tri"])
    assert 380 <= len(rays) - n <= 460 and n >= 20 and (~cref.valid(rays)).sum() == 6 and np.isinf(rays[:-n, 7]).sum() > 300
    before = count[soup["whole"]]
    assert (before >= 2).all() and (count[-n::2] >= 1).all() and (count[-n::2] < before[::2]).all()        # far before the second crossing
    assert (count[-n + 1::2] >= 1).all() and (count[-n::2] + count[-n + 1::2] == before[::2]).all()       # near behind the first: the rest


@pytest.mark.parametrize("name,lo,cell,dims", cref.configs(), ids=[f"{n[0]}-{n[1]:.3g}" for n, _, _, _ in cref.configs()])
def test_the_count_mode_walk_returns_the_integers_of_trying_every_triangle(soup, name, lo, cell, dims):
    box = cref.box_of([float(F(x)) for x in lo], float(F(cell)), dims)
    brute = sref.crossings(soup["rays"], soup["ver"], soup["tri"], box)
    grid = sref.crossings_grid(soup["rays"], soup["ver"], soup["tri"], lo, cell, dims)
    assert grid.dtype == np.int32 and np.array_equal(grid, brute), name
    assert brute[~cref.valid(soup["rays"])].tolist() == [0] * 6
    if name[0] != "part":                                                     # the rays are of every kind: 0, 1, 2 and more crossings
        assert 380 <= len(brute) and (brute == 0).sum() >= 100 and (brute == 1).sum() >= 40 and (brute >= 2).sum() >= 15
        assert np.isinf(soup["rays"][brute >= 2, 7]).sum() >= 10
    if name == ("odd", 0.25):                                                 # shown once: the rule is what makes it hold
        loose = sref.crossings_grid(soup["rays"], soup["ver"], soup["tri"], lo, cell, dims, once=False)
        assert (loose >= brute).all() and (loose > brute).sum() >= 50


def test_the_count_far_from_the_origin_of_coordinates(soup):
    ver = (soup["ver"] + F(1000)).astype(F)
    rays = soup["rays"].copy()
    rays[:, :3] += F(1000)
    lo, cell, dims = (996.9, 997.7, 992.3), 0.25, cref.dims_of(0.25)
    brute = sref.crossings(rays, ver, soup["tri"], cref.box_of([float(F(x)) for x in lo], cell, dims))
    assert np.array_equal(sref.crossings_grid(rays, ver, soup["tri"], lo, cell, dims), brute) and (brute >= 2).sum() >= 15


# ---- INSIDE on the restatement -------------------------------------------------------------------------------------------------

def test_points_inside_and_outside_the_sealed_box():
    s = cref.scene_box()
    inner, outer = sref.box_points(s)
    assert len(inner) == 10 == len(outer) and (np.abs(inner).max(axis=1) < 1).all() and (np.abs(outer).max(axis=1) > 1).all()
    assert (np.abs(inner[2:]).min(axis=1) > 0.94).all()                       # near the corners
    for box in (None, _box_of(s)):
        for K in (1, 3, 5, 7):
            flag, votes = sref.inside(inner, s["ver"], s["tri"], K, box)
            assert votes.dtype == np.uint8 and votes.tolist() == [K] * 10 and flag.all()
            flag, votes = sref.inside(outer, s["ver"], s["tri"], K, box)
            assert votes.tolist() == [0] * 10 and not flag.any()
    far = F([[5, 5, 5], [-40, 0.1, 0.2], [NAN, 0, 0], [0, INF, 0]])           # outside the grid's box too, and no points
    flag, votes = sref.inside(far, s["ver"], s["tri"], 3, _box_of(s))
    assert votes.tolist() == [0, 0, 255, 255] and not flag.any()


def test_points_inside_and_outside_the_ball_are_unanimous():
    """A condition of the inputs that test_meshsolid_gpu.py shares: along all seven directions, so along every odd K."""
    ver, tri = sref.ball()
    assert len(tri) > 1000 and dref.usable(ver, tri).all()
    r = np.linalg.norm(ver.astype(np.float64), axis=1)
    assert 0.75 < r.min() and r.max() < 0.81
    pts = sref.ball_points()
    norm = np.linalg.norm(pts.astype(np.float64), axis=1)
    assert (norm[:200] < 0.7).all() and (norm[200:] > 0.9).all() and len(pts) == 400
    flag, votes = sref.inside(pts, ver, tri, 7)
    assert votes[:200].tolist() == [7] * 200 and votes[200:].tolist() == [0] * 200
    assert flag[:200].all() and not flag[200:].any()


def test_the_kept_lattice_reference_is_the_restatement_s_and_describes_a_ball():
    ver, tri = sref.ball()
    ref = sref.ball_lattice()
    assert ref["trunc"] == 0.375 and len(ref["pts"]) == 17 ** 3 == len(ref["sd"]) == len(ref["inside"]) == len(ref["votes"])
    r = np.linalg.norm(ref["pts"].astype(np.float64), axis=1)
    clear = np.abs(r - 0.8) > 0.03                                            # the facets cut at most 0.03 off the sphere
    assert (ref["inside"][clear] == (r[clear] < 0.8)).all() and (ref["votes"] == 3 * ref["inside"]).all()
    assert ((ref["sd"] < 0) == ref["inside"]).all()
    near = np.isfinite(ref["sd"])
    assert np.abs(-ref["sd"][near] - (0.8 - r[near])).max() < 0.03 and (np.abs(ref["sd"][near]) <= F(0.375)).all()
    assert (np.abs(r[~near] - 0.8) > 0.375 - 0.03).all() and (~near).sum() > 1000 and near.sum() > 2000
    some = np.random.default_rng(0).choice(17 ** 3, 150, replace=False)       # a fresh computation of the sides at some points
    flag, votes = sref.inside(ref["pts"][some], ver, tri, 3)
    assert np.array_equal(flag, ref["inside"][some]) and np.array_equal(votes, ref["votes"][some])


def test_culling_changes_no_parity():
    s = cref.scene_box()
    inner, outer = sref.box_points(s)
    ver, tri = cref.soup40()
    rays = cref.soup_rays(ver, tri)
    for pts, v, t in ((np.concatenate([inner, outer]), s["ver"], s["tri"]), (rays[:200, :3], ver, tri)):
        assert np.array_equal(sref.parities(pts, v, t, 7), sref.parities(pts, v, t, 7, cull=False))


def test_the_lattice_value_and_the_lattice_points():
    sd = F([0.0, 0.1, -0.1, 0.3, -0.3, 5.0, -5.0, INF, -INF])
    got = sref.lattice_value(sd, 0.3)
    assert got.dtype == F and got[[0, 5, 6, 7, 8]].tolist() == [0.0, -1.0, 1.0, -1.0, 1.0]
    assert got[1] == F(0.1) * F(-1.0 / 0.3) and got[2] == -got[1] and abs(float(got[3])) == 1.0
    p = sref.lattice_points((-1, -1, -1), (1, 1, 1), (17, 9, 5))
    assert p.shape == (5, 9, 17, 3) and p.dtype == F
    assert p[0, 0, :, 0].tolist() == [-1 + 0.125 * i for i in range(17)] and p[3, 2, 1].tolist() == [-0.875, -0.5, 0.5]
    assert sref.default_trunc((-1, -1, -1), (1, 1, 1), (17, 9, 5)) == 1.5
