"""GPU checks of the mesh simplification (csrc/nfl_simplify.hip through nerf_fl_amd.geometry.simplify_mesh) against the
numpy restatement of tests/simplify_ref.py.

What is compared how.  `cluster`, the triangles, V', T', the colours and the "mean" positions are integers, copied floats
or fp64 expressions of int64 sums rounded once: equality is EXACT (on the bits).  Normals go through an fp64 square root
and a division: 1e-6 absolute.  "quadric" positions come out of nine fp64 sums whose order the device does not fix, and
of a 3 x 3 solve: 2 fp32 ulps of the coordinate -- one for the final rounding sitting near a tie, one for the device's
fp64 divide and square root not being bit-equal to numpy's (tests/test_simplify_cpu.py shows that the order of the sums
alone moves nothing by more than one).  Measured worst on an MI355X: 0 ulp on the cube, 0 ulp on the ball.

Sizes.  Kernels run 256 threads (4 waves) a workgroup: 63 / 64 / 65 cross a wave, 257 a workgroup.  The scan works on
tiles of 2048: the soup of 70 000 vertices and 150 000 triangles crosses 35 and 74 of them (two levels) and loads both
hash tables (262 144 and 524 288 slots) to more than a quarter at cell = 0.05, where most clusters have one member and
nearly every triangle survives; at cell = 100 everything falls into the 8 cells that meet at the origin, every vertex
on one of 8 slots."""
import ctypes as C

import numpy as np
import pytest
import torch

import simplify_ref as sr
import nerf_fl_amd
from geom_gpu_util import bits as _bits, same as _same, to_dev as _to_dev
from gpu_util import DEV, make_embeddings
from nerf_fl_amd import NeRF, _lib, geometry, rendering, synth

pytestmark = pytest.mark.gpu


def _ulps(a, b):
    """|a - b| in units of the fp32 spacing at max(|a|, |b|)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return np.abs(a.astype(np.float64) - b.astype(np.float64)) / np.spacing(np.maximum(np.abs(a), np.abs(b))).astype(np.float64)


def _normals_close(got, exp, what):
    """Within 1e-6 absolute; a row copied bit for bit (a cluster of one may carry a NaN) is equal."""
    got, exp = got.cpu().numpy() if torch.is_tensor(got) else got, np.asarray(exp)
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    with np.errstate(invalid="ignore"):
        diff = np.where(_bits(got) == _bits(exp), 0.0, np.abs(got.astype(np.float64) - exp.astype(np.float64)))
    assert not diff.size or diff.max() <= 1e-6, (what, "normals")             # a NaN difference fails the comparison


def _check(mesh, cell, origin=(0.0, 0.0, 0.0), what="", exp=None, dev=None):
    """simplify_mesh, placement "mean", against the restatement: everything exact but the normals."""
    exp, exp_cluster, totals = exp if exp is not None else sr.simplify(mesh, cell, origin, "mean")
    got, cluster = geometry.simplify_mesh(dev if dev is not None else _to_dev(mesh), cell, origin=origin, return_map=True)
    assert set(got) == set(exp), what
    assert got["vertices"].shape == (totals[0], 3) and got["triangles"].shape == (totals[1], 3), what
    _same(cluster, exp_cluster, (what, "cluster"))
    _same(got["triangles"], exp["triangles"], (what, "triangles"))
    _same(got["vertices"], exp["vertices"], (what, "vertices"))
    if "colors" in exp:
        _same(got["colors"], exp["colors"], (what, "colors"))
    _normals_close(got["normals"], exp["normals"], what)
    return got, cluster, totals


# ---- small cases

@pytest.mark.parametrize("name", sorted(sr.hand_cases()))
def test_hand_cases(name):
    mesh, cell, origin = sr.hand_cases()[name]
    _check(mesh, cell, origin, name)


def test_empty_mesh_launches_nothing():
    mesh = _to_dev(sr._mesh(np.zeros((0, 3)), np.zeros((0, 3))))
    got, cluster = geometry.simplify_mesh(mesh, 0.5, return_map=True)
    assert got["vertices"].shape == got["normals"].shape == (0, 3) and got["triangles"].shape == (0, 3)
    assert got["triangles"].dtype == torch.int32 and cluster.shape == (0,) and cluster.dtype == torch.int32


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_small_soups(V):
    mesh = sr.soup(V, 3 * V + 1, seed=V)
    for cell in (0.7, 2.5):
        _check(mesh, cell, (0.1, -0.2, 0.3), f"V = {V}, cell = {cell}")


# ---- the soup that crosses scan tiles and loads both tables

@pytest.fixture(scope="module")
def big_soup():
    mesh = sr.soup(70_000, 150_000, seed=1)
    return mesh, _to_dev(mesh)


@pytest.mark.parametrize("cell", [0.05, 0.5, 100.0])
def test_big_soup(big_soup, cell):
    mesh, dev = big_soup
    exp = sr.simplify(mesh, cell)
    n = np.bincount(exp[1][exp[1] >= 0])
    if cell == 100.0:
        assert exp[2][0] == 8                                              # the cells that meet at the origin
    if cell == 0.05:
        assert (n == 1).mean() > 0.9                                       # the bit-for-bit rule does the work
    got, cluster, totals = _check(mesh, cell, what=f"soup, cell = {cell}", exp=exp, dev=dev)
    assert totals[3] == 3
    again = geometry.simplify_mesh(dev, cell)                              # two runs: identical bits
    for k in got:
        _same(again[k], _bits(got[k]), (cell, k))


# ---- a real surface

@pytest.fixture(scope="module")
def ball():
    lat, lo, hi, sp = sr.ball_lattice(33)
    dev = geometry.extract_surface(torch.from_numpy(lat).to(DEV), 0.0, lo, hi)
    dev["colors"] = (dev["normals"].abs() * 0.5 + 0.25).contiguous()
    return {k: v.cpu().numpy() for k, v in dev.items()}, dev, lo, float(sp[0])


@pytest.mark.parametrize("spacings", [2.0, 3.5])
def test_ball(ball, spacings):
    mesh, dev, lo, sp = ball
    got, cluster, totals = _check(mesh, spacings * sp, lo, f"ball, {spacings} spacings", dev=dev)
    assert 0 < totals[0] < len(mesh["vertices"]) and 0 < totals[1] < len(mesh["triangles"]) and totals[2:] == [0, 0]
    r = got["vertices"].double().norm(dim=1)
    assert (r - 0.6).abs().max().item() < spacings * sp


def _check_quadric(mesh, dev, cell, origin, what):
    exp, exp_cluster, totals = sr.simplify(mesh, cell, origin, "quadric")
    got, cluster = geometry.simplify_mesh(dev, cell, origin=origin, placement="quadric", return_map=True)
    _same(cluster, exp_cluster, (what, "cluster"))
    _same(got["triangles"], exp["triangles"], (what, "triangles"))
    if "colors" in exp:
        _same(got["colors"], exp["colors"], (what, "colors"))
    _normals_close(got["normals"], exp["normals"], what)
    ver = got["vertices"].cpu().numpy()
    assert ver.shape == exp["vertices"].shape and np.isfinite(ver).all()
    worst = float(_ulps(ver, exp["vertices"]).max())
    print(f"quadric positions, {what}: worst {worst} ulp against the restatement")
    assert worst <= 2.0, what
    return got, exp


def test_quadric_on_the_cube():
    mesh = sr.cube_surface(6)
    cell, origin = 0.8, (-1.2, -1.2, -1.2)
    got, exp = _check_quadric(mesh, _to_dev(mesh), cell, origin, "cube")
    mean = geometry.simplify_mesh(_to_dev(mesh), cell, origin=origin)
    corner = (mesh["vertices"] == np.float32(1)).all(axis=1).argmax()
    c = int(sr.clusters(mesh["vertices"], cell, origin)[0][corner])
    d_quad = (got["vertices"][c] - 1.0).abs().max().item()
    d_mean = (mean["vertices"][c] - 1.0).abs().max().item()
    assert d_quad < 1e-3 < 0.1 < d_mean                                     # the corner is kept


@pytest.mark.parametrize("spacings", [2.0, 3.5])
def test_quadric_on_the_ball(ball, spacings):
    mesh, dev, lo, sp = ball
    got, exp = _check_quadric(mesh, dev, spacings * sp, lo, f"ball, {spacings} spacings")
    again = geometry.simplify_mesh(dev, spacings * sp, origin=lo, placement="quadric")
    for k in ("triangles", "normals", "colors"):
        _same(again[k], _bits(got[k]), k)
    assert float(_ulps(again["vertices"].cpu().numpy(), got["vertices"].cpu().numpy()).max()) <= 2.0


# ---- the C ABI: nothing outside the outputs

def test_outputs_are_framed_by_sentinels():
    V, T, guard = 257, 700, 64
    mesh = sr.soup(V, T, seed=3)
    exp, exp_cluster, totals = sr.simplify(mesh, 1.5, (0.0, 0.0, 0.0), "quadric")
    dev = _to_dev(mesh)
    lib = _lib.lib()
    nbytes = lib.nfl_mesh_simplify_bytes(V, T)
    assert nbytes % 8 == 0
    f32 = lambda rows: torch.full((rows + 2 * guard, 3), -7.0, dtype=torch.float32, device=DEV)
    scratch = torch.full((nbytes // 8 + 2 * guard,), -7, dtype=torch.int64, device=DEV)
    d_totals = torch.full((4 + 2 * guard,), -7, dtype=torch.int64, device=DEV)
    cluster = torch.full((V + 2 * guard,), -7, dtype=torch.int32, device=DEV)
    out_v, out_n, out_c = f32(totals[0]), f32(totals[0]), f32(totals[0])
    out_t = torch.full((totals[1] + 2 * guard, 3), -7, dtype=torch.int32, device=DEV)
    a = _lib.MeshSimplifyArgs()
    a.d_vertices, a.d_normals, a.d_colors = dev["vertices"].data_ptr(), dev["normals"].data_ptr(), dev["colors"].data_ptr()
    a.d_triangles, a.n_vertices, a.n_triangles, a.cell, a.placement = dev["triangles"].data_ptr(), V, T, 1.5, 1
    a.d_scratch, a.scratch_bytes = scratch[guard:].data_ptr(), nbytes
    a.d_totals, a.d_cluster = d_totals[guard:].data_ptr(), cluster[guard:].data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(lib.nfl_mesh_simplify_count(C.byref(a), stream), "nfl_mesh_simplify_count")
    assert d_totals[guard:guard + 4].tolist() == totals
    a.n_out_vertices, a.n_out_triangles = totals[0], totals[1]
    a.d_out_vertices, a.d_out_normals, a.d_out_colors = out_v[guard:].data_ptr(), out_n[guard:].data_ptr(), out_c[guard:].data_ptr()
    a.d_out_triangles = out_t[guard:].data_ptr()
    _lib.check(lib.nfl_mesh_simplify_emit(C.byref(a), stream), "nfl_mesh_simplify_emit")
    torch.cuda.synchronize()
    for buf, n in ((scratch, nbytes // 8), (d_totals, 4), (cluster, V), (out_v, totals[0]), (out_n, totals[0]),
                   (out_c, totals[0]), (out_t, totals[1])):
        assert (buf[:guard] == -7).all() and (buf[guard + n:] == -7).all()          # nothing written out of range
    _same(cluster[guard:guard + V], exp_cluster, "cluster")
    _same(out_t[guard:guard + totals[1]], exp["triangles"], "triangles")
    _same(out_c[guard:guard + totals[0]], exp["colors"], "colors")
    assert float(_ulps(out_v[guard:guard + totals[0]].cpu().numpy(), exp["vertices"]).max()) <= 2.0


# ---- the Python layer

def test_out_of_range_index_raises_with_the_count():
    mesh = sr.soup(70, 40, seed=4)
    mesh["triangles"][[3, 17, 29]] = [[0, 1, 70], [-1, 4, 5], [2 ** 31 - 1, 6, 7]]
    with pytest.raises(ValueError, match="3 of 40 triangles"):
        geometry.simplify_mesh(_to_dev(mesh), 0.5)
    empty = _to_dev(sr._mesh(np.zeros((0, 3)), [[0, 1, 2]]))
    with pytest.raises(ValueError, match="1 of 1 triangles"):
        geometry.simplify_mesh(empty, 0.5)


def test_return_map_and_argument_checks():
    mesh = sr.soup(65, 100, seed=6)
    dev = _to_dev(mesh)
    alone = geometry.simplify_mesh(dev, 1.0)
    both = geometry.simplify_mesh(dev, 1.0, return_map=True)
    assert isinstance(alone, dict) and isinstance(both, tuple) and len(both) == 2
    assert both[1].dtype == torch.int32 and both[1].shape == (65,) and both[1].device == dev["vertices"].device
    for k in alone:
        _same(both[0][k], _bits(alone[k]), k)
    assert both[1].max().item() == alone["vertices"].shape[0] - 1
    without = {k: v for k, v in dev.items() if k != "colors"}
    assert "colors" not in geometry.simplify_mesh(without, 1.0)
    with pytest.raises(ValueError):
        geometry.simplify_mesh(dev, 0.0)
    with pytest.raises(ValueError):
        geometry.simplify_mesh(dev, 1.0, placement="median")
    with pytest.raises(ValueError):
        geometry.simplify_mesh(dev, 1.0, origin=(0, 0))
    with pytest.raises(ValueError):
        geometry.simplify_mesh(dict(dev, triangles=dev["triangles"].long()), 1.0)


def test_isolated_clusters_go_with_clean_mesh():
    """A cluster none of whose triangles survive stays as a vertex no triangle names; clean_mesh(min_triangles=1) drops it."""
    mesh, cell, origin = sr.hand_cases()["two_in_one_cell"]
    got = geometry.simplify_mesh(_to_dev(mesh), cell, origin=origin)
    assert got["vertices"].shape == (2, 3) and got["triangles"].shape == (0, 3)
    cleaned = geometry.clean_mesh(got, min_triangles=1)
    assert cleaned["vertices"].shape == (0, 3)


def test_extract_mesh_simplifies_before_colouring():
    nerf_fl_amd.set_precision("f16x3")
    try:
        rendering.check_status(DEV)
    except FloatingPointError:
        pass
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(DEV)
    emb = make_embeddings(10, False)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (25, 25, 25)
    cell = 2.0 * 2.0 / 24
    with torch.no_grad():
        lattice = geometry.density_lattice(model, emb, lo, hi, res)
        iso = lattice.median().item()
        plain = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso)
        for placement in ("mean", "quadric"):
            got = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, simplify=cell, placement=placement)
            exp = geometry.simplify_mesh(geometry.extract_surface(lattice, iso, lo, hi), cell, origin=lo, placement=placement)
            Vs = exp["vertices"].shape[0]
            assert 0 < Vs < plain["vertices"].shape[0] and 0 < exp["triangles"].shape[0] < plain["triangles"].shape[0]
            assert set(got) == {"vertices", "normals", "triangles", "colors"} and got["colors"].shape == (Vs, 3)
            _same(got["triangles"], _bits(exp["triangles"]), "triangles")
            _same(got["normals"], _bits(exp["normals"]), "normals")
            if placement == "mean":
                _same(got["vertices"], _bits(exp["vertices"]), "vertices")
            else:
                assert float(_ulps(got["vertices"].cpu().numpy(), exp["vertices"].cpu().numpy()).max()) <= 2.0
            _same(got["colors"], _bits(geometry.surface_colors(model, emb, got["vertices"], got["normals"])), "colors")
    rendering.check_status(DEV)
