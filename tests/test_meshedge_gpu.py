"""GPU checks of the mesh edges (csrc/nfl_meshedge.hip through nerf_fl_amd.topology) against the numpy restatement of
tests/meshedge_ref.py.

What is compared how.  Every table is EXACTLY equal to the restatement, the fp32 columns on the bits: the edge table and the
loops are integer work made independent of the order of the atomics by a sort of every row and by numbering loops from their
smallest half-edge; perimeter, centroid and the new vertex's normal and colour are sequential fp64 folds in walk order, every
operation rounded on its own (-ffp-contract=off), with one rounding to fp32.

Sizes.  Kernels run 256 threads (4 waves) a workgroup: soups of 63 / 64 / 65 vertices cross a wave, 257 a workgroup.  The
scan works on tiles of 2048: the soup of 70 000 vertices and 150 000 triangles crosses 220 of them over its 450 000
half-edges (two levels).  An edge's row of up to 8 half-edges is sorted by its thread, a longer one by the wave: the dense soup
(rows of about 14) and the book of 300 triangles on one edge take the long path.  The fan has a hub of 4096 triangles (a
binary search in a row of 4096) and a rim loop of 4096 edges that one thread folds in order."""
import numpy as np
import pytest
import torch

import meshedge_ref as eref
import meshsmooth_ref as sref
import tsdf_ref as tref
from geom_gpu_util import F, PAD, bits as _bits, dev as _dev, framed as _framed, same as _same, stream as _stream, to_dev as _to_dev, \
    unframe as _unframe
from gpu_util import DEV
from nerf_fl_amd import _lib, fusion, geometry, solid, topology
from nerf_fl_amd.data import ImageBank

pytestmark = pytest.mark.gpu

EDGE_KEYS = ("edges", "half_edge", "edge_offsets", "edge_halves", "kind", "twin")
EDGE_TOTALS = ("n_edges", "n_halves", "n_boundary", "n_flipped", "n_nonmanifold", "n_degenerate")
LOOP_KEYS = ("loop_offsets", "loop_halves", "loop_of", "length", "perimeter", "centroid")
MESH_KEYS = ("vertices", "normals", "colors", "triangles")
TOPO_ROWS = ("vertices", "edges", "triangles", "euler", "loops", "genus")


def _colored(mesh, seed=1):
    return dict(mesh, colors=np.random.default_rng(seed).uniform(0, 1, mesh["vertices"].shape).astype(F))


def _same_edges(got, exp, what):
    assert set(got) == set(EDGE_KEYS) | set(EDGE_TOTALS), what
    for k in EDGE_KEYS:
        _same(got[k], exp[k], (what, k))
    assert [got[k] for k in EDGE_TOTALS] == exp["totals"][:6], (what, [got[k] for k in EDGE_TOTALS], exp["totals"])


def _same_loops(got, exp, what):
    assert set(got) == set(LOOP_KEYS) | {"n_loops", "n_open"}, what
    for k in LOOP_KEYS:
        _same(got[k], exp[k], (what, k))
    assert (got["n_loops"], got["n_open"]) == (exp["n_loops"], exp["n_open"]), what


def _same_fill(got, exp, what):
    (gm, gi), (em, ei) = got, exp
    assert set(gm) == set(em), what
    for k in em:
        _same(gm[k], em[k], (what, k))
    for k in ("n_filled", "n_new_vertices", "n_new_triangles"):
        assert gi[k] == ei[k], (what, k, gi[k], ei[k])
    for k in ("new_vertices", "new_triangles"):
        _same(gi[k], ei[k], (what, k))


def _check(mesh, what, fill=True, **select):
    """The edge table, the loops, the report and the filled mesh of `mesh` (arrays) against the restatement; returns both."""
    V = len(mesh["vertices"])
    dev = _to_dev(mesh)
    exp_ed = eref.edges(mesh["triangles"], V)
    exp_lp = eref.loops(mesh["vertices"], mesh["triangles"], exp_ed)
    ed = topology.mesh_edges(dev)
    _same_edges(ed, exp_ed, what)
    lp = topology.boundary_loops(dev, edges=ed)
    _same_loops(lp, exp_lp, what)
    topo, exp_topo = topology.mesh_topology(dev, edges=ed, loops=lp), eref.topology(mesh, exp_ed, exp_lp)
    for k in ("closed", "manifold", "oriented", "n_loops", "n_open", "n_components"):
        assert topo[k] == exp_topo[k] and type(topo[k]) in (bool, int), (what, k, topo[k], exp_topo[k])
    _same(topo["component"], exp_topo["component"], (what, "component"))
    for k in TOPO_ROWS:
        _same(topo[k], exp_topo[k].astype(np.int64), (what, k))
    if fill:
        got = topology.fill_holes(dev, loops=lp, **select)
        if "keep" in select:
            select = dict(select, keep=select["keep"].cpu().numpy())
        exp = eref.fill(mesh, exp_lp, **select)
        if exp[1]["n_filled"] == 0:
            assert got[0] is dev and got[1]["n_filled"] == 0 and not got[1]["new_vertices"].any() and not got[1]["new_triangles"].any()
        else:
            _same_fill(got, exp, what)
    return dev, ed, lp, exp_ed, exp_lp


# ---- the cases -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(set(sref.hand_cases()) - {"out_of_range"}))
def test_hand_cases(name):
    _check(_colored(sref.hand_cases()[name]), name)


def test_more_hand_cases():
    _check(dict(sref.hand_cases()["tetrahedron"], triangles=np.int32([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 2, 3]])), "a face reversed")
    _, ed, lp, _, _ = _check(eref.moebius(), "moebius")
    assert ed["n_flipped"] >= 1 and ed["n_nonmanifold"] == 0
    _, ed, lp, _, _ = _check(_colored(sref.grid_patch(5)), "grid patch")
    assert lp["n_loops"] == 1 and lp["length"].tolist() == [16]


def test_an_index_out_of_range_raises_naming_the_count():
    dev = _to_dev(sref.hand_cases()["out_of_range"])
    for call in (topology.mesh_edges, topology.boundary_loops, topology.mesh_topology, topology.fill_holes):
        with pytest.raises(ValueError, match=r"2 of 4 triangles have an index outside \[0, 4\)"):
            call(dev)


def test_empty_meshes_launch_nothing():
    for V, T in ((0, 0), (5, 0)):
        mesh = sref._mesh(np.zeros((V, 3)), np.zeros((T, 3)))
        dev, ed, lp, _, _ = _check(mesh, f"empty {V} {T}")
        assert ed["n_edges"] == 0 and lp["n_loops"] == 0 and ed["edge_offsets"].tolist() == [0] and lp["loop_offsets"].tolist() == [0]


@pytest.mark.parametrize("V,T", [(1, 3), (63, 150), (64, 150), (65, 150), (257, 600)])
def test_soups_across_the_wave_and_the_workgroup(V, T):
    _check(_colored(sref.soup(V, T, seed=V)), f"soup {V}")


def test_a_dense_soup_has_many_nonmanifold_edges_with_long_rows():
    mesh = _colored(sref.soup(30, 2000, seed=4))
    _, ed, _, exp_ed, _ = _check(mesh, "dense soup")
    rows = np.diff(exp_ed["edge_offsets"])
    assert ed["n_nonmanifold"] > 400 and rows.max() > _lib.EDGE_SHORT_ROW and (rows <= _lib.EDGE_SHORT_ROW).any()


def test_a_book_of_300_triangles_on_one_edge():
    _, ed, lp, exp_ed, _ = _check(eref.book(300), "book")
    assert np.diff(exp_ed["edge_offsets"])[0] == 300 and ed["n_nonmanifold"] == 1 and lp["n_loops"] == 0 and lp["n_open"] == 600


def test_the_fan_has_a_hub_and_a_rim_loop_folded_in_order():
    mesh = _colored(sref.fan(4096))
    _, ed, lp, _, exp_lp = _check(mesh, "fan")
    assert sorted(lp["length"].tolist()) == [300, 4096]
    _check(mesh, "fan, the strip's rim alone", max_edges=300)
    _check(mesh, "fan, nothing", max_perimeter=1e-3)


@pytest.fixture(scope="module")
def big_soup():
    return sref.soup(70000, 150000, seed=5)


def test_the_big_soup_over_two_scan_levels_and_twice_the_same_bits(big_soup):
    dev, ed, lp, _, _ = _check(big_soup, "big soup", fill=False)
    ed2 = topology.mesh_edges(dev)
    lp2 = topology.boundary_loops(dev)
    for k in EDGE_KEYS:
        assert torch.equal(ed[k], ed2[k]), k
    for k in LOOP_KEYS:
        assert np.array_equal(_bits(lp[k]), _bits(lp2[k])), k
    a, b = topology.fill_holes(dev, loops=lp, max_edges=3), topology.fill_holes(dev, loops=lp2, max_edges=3)
    assert a[1]["n_filled"] == b[1]["n_filled"] > 1000
    for k in a[0]:
        assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])), k


@pytest.fixture(scope="module")
def punched():
    ball = _colored(eref.lattice_mesh(33, "ball"), 2)
    for seed in range(50):
        mesh, chosen, valence = eref.punch(ball, 5, seed)
        if len(chosen) == 5 and min(valence) < max(valence):
            return mesh, chosen, valence, ball
    raise AssertionError("no seed gives five one-rings of differing valence")


def test_the_punched_ball_and_its_fill_with_masks_and_both_limits(punched):
    mesh, chosen, valence, ball = punched
    dev, ed, lp, exp_ed, exp_lp = _check(mesh, "punched ball")
    assert lp["n_loops"] == 5 and sorted(lp["length"].tolist()) == sorted(valence) and lp["n_open"] == 0
    _check(mesh, "punched ball, max_edges", max_edges=max(valence) - 1)
    _check(mesh, "punched ball, max_perimeter", max_perimeter=float(np.sort(exp_lp["perimeter"])[1]))
    _check(mesh, "punched ball, keep", keep=_dev([1, 0, 1, 0, 0], np.bool_))
    _check(mesh, "punched ball, all three", keep=_dev([1, 1, 1, 0, 1], np.bool_), max_edges=max(valence), max_perimeter=10.0)
    got, info = topology.fill_holes(dev, keep=_dev([0] * 5, np.bool_))
    assert got is dev and info["n_filled"] == 0                               # nothing selected: the input object
    filled, info = topology.fill_holes(dev)
    topo = topology.mesh_topology(filled)
    assert topo["closed"] and topo["manifold"] and topo["oriented"] and topo["euler"][0] == 2 and topo["genus"][0] == 0
    smooth = geometry.smooth_mesh(filled, 2, pinned=~info["new_vertices"])    # relaxes the caps alone
    moved = (smooth["vertices"] != filled["vertices"]).any(dim=1)
    assert not moved[~info["new_vertices"]].any()


def test_tables_given_are_the_tables_built(punched):
    mesh = punched[0]
    dev = _to_dev(mesh)
    adj = geometry.mesh_adjacency(dev)
    ed, ed2 = topology.mesh_edges(dev), topology.mesh_edges(dev, adjacency=adj)
    lp, lp2 = topology.boundary_loops(dev), topology.boundary_loops(dev, edges=ed)
    for k in EDGE_KEYS:
        assert torch.equal(ed[k], ed2[k]), k
    for k in LOOP_KEYS:
        assert np.array_equal(_bits(lp[k]), _bits(lp2[k])), k
    a, b, c = topology.fill_holes(dev), topology.fill_holes(dev, loops=lp), topology.fill_holes(dev, edges=ed)
    for k in a[0]:
        assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])) and np.array_equal(_bits(a[0][k]), _bits(c[0][k])), k
    t1, t2 = topology.mesh_topology(dev), topology.mesh_topology(dev, edges=ed, loops=lp)
    assert all(torch.equal(t1[k], t2[k]) for k in TOPO_ROWS) and t1["closed"] == t2["closed"]
    for bad in (dict(edges={}), dict(edges=dict(ed, twin=ed["twin"][:-1])), dict(edges=dict(ed, n_boundary=-1)),
                dict(edges=dict(ed, kind=ed["kind"].int()))):
        with pytest.raises(ValueError, match="edges"):
            topology.boundary_loops(dev, **bad)
    for bad in (dict(loops={}), dict(loops=dict(lp, loop_of=lp["loop_of"][:-1])), dict(loops=dict(lp, centroid=lp["centroid"].double())),
                dict(keep=torch.ones(4, dtype=torch.bool, device=DEV)), dict(keep=torch.ones(5, dtype=torch.uint8, device=DEV)),
                dict(keep=torch.ones(5, dtype=torch.bool))):
        with pytest.raises((ValueError, RuntimeError)):
            topology.fill_holes(dev, **bad)


def test_foreign_tables_are_read_within_bounds():
    """The adjacency, the edge table and the loops of ANOTHER mesh of the same sizes: the output is wrong and every value that
    is used as an index downstream stays in range; the device answers a right question right afterwards."""
    a, b = _colored(sref.soup(257, 600, seed=1)), _colored(sref.soup(257, 600, seed=2))
    b["triangles"][::7] = b["triangles"][::7][:, [0, 0, 2]]                   # and some degenerate ones
    da, db = _to_dev(a), _to_dev(b)
    T = 600
    ed = topology.mesh_edges(da, adjacency=geometry.mesh_adjacency(db))
    E, H = ed["n_edges"], ed["n_halves"]
    assert 0 <= E <= 3 * T and 0 <= H <= 3 * T
    assert ((ed["half_edge"] >= -1) & (ed["half_edge"] < max(E, 1))).all() and ((ed["twin"] >= -1) & (ed["twin"] < 3 * T)).all()
    assert ((ed["edge_halves"] >= 0) & (ed["edge_halves"] < 3 * T)).all() and (ed["kind"] <= 3).all()
    assert (ed["edge_offsets"][1:] >= ed["edge_offsets"][:-1]).all() and ed["edge_offsets"][-1] == H
    theirs = topology.mesh_edges(db)
    for tables in (ed, theirs):
        lp = topology.boundary_loops(da, edges=tables)
        L = lp["n_loops"]
        assert 0 <= L <= T and ((lp["loop_of"] >= -1) & (lp["loop_of"] < max(L, 1))).all()
        assert (lp["loop_offsets"][1:] >= lp["loop_offsets"][:-1]).all() and lp["loop_offsets"][-1] == lp["loop_halves"].shape[0]
    for loops in (lp, topology.boundary_loops(db)):
        try:
            out, info = topology.fill_holes(da, loops=loops)
            assert out["vertices"].shape[0] == 257 + info["n_new_vertices"] and out["triangles"].shape[0] == T + info["n_new_triangles"]
        except RuntimeError as e:                                             # totals the emit call refuses: also an answer
            assert "nfl_mesh_fill_emit" in str(e)
    torch.cuda.synchronize()
    _check(a, "after the foreign tables")


# ---- the C ABI by hand: every output and the scratch between sentinels -------------------------------------------------------------

def _inner(buf):
    return buf[PAD:].data_ptr()


def test_outputs_and_scratch_are_framed_by_sentinels(punched):
    mesh = punched[0]
    V, T = len(mesh["vertices"]), len(mesh["triangles"])
    dev = _to_dev(mesh)
    adj = geometry.mesh_adjacency(dev)
    Lb, s = _lib.lib(), _stream()
    exp_ed = eref.edges(mesh["triangles"], V)
    exp_lp = eref.loops(mesh["vertices"], mesh["triangles"], exp_ed)
    exp_mesh, exp_info = eref.fill(mesh, exp_lp)
    i32, i64, u8, f32 = torch.int32, torch.int64, torch.uint8, torch.float32
    tri, ver = dev["triangles"].data_ptr(), dev["vertices"].data_ptr()

    def scratch(nbytes):
        assert nbytes % 8 == 0
        return _framed(nbytes // 8, (), 0x5A5A5A5A5A5A5A5A, i64), nbytes

    # edges
    sc, nb = scratch(Lb.nfl_mesh_edges_bytes(V, T))
    totals = _framed(_lib.EDGE_TOTALS, (), -7, i64)
    assert Lb.nfl_mesh_edges_count(tri, V, T, adj["offsets"].data_ptr(), adj["neighbors"].data_ptr(), adj["neighbors"].shape[0], _inner(sc),
                                   nb, _inner(totals), s) == 0
    tot = _unframe(totals, _lib.EDGE_TOTALS, -7, "edge totals").tolist()
    assert tot == exp_ed["totals"]
    E, H = tot[:2]
    out = {"edges": _framed(E, (2,), -3, i32), "half_edge": _framed(3 * T, (), -3, i32), "edge_offsets": _framed(E + 1, (), -3, i64),
           "edge_halves": _framed(H, (), -3, i32), "kind": _framed(E, (), 77, u8), "twin": _framed(3 * T, (), -3, i32)}
    assert Lb.nfl_mesh_edges_emit(tri, V, T, _inner(sc), nb, E, H, *(_inner(out[k]) for k in EDGE_KEYS), s) == 0
    ed = {k: _unframe(out[k], len(exp_ed[k]), 77 if k == "kind" else -3, k) for k in EDGE_KEYS}
    for k in EDGE_KEYS:
        _same(ed[k], exp_ed[k], k)
    _unframe(sc, nb // 8, 0x5A5A5A5A5A5A5A5A, "edge scratch")
    # loops
    sc, nb = scratch(Lb.nfl_mesh_loops_bytes(T))
    totals = _framed(_lib.LOOP_TOTALS, (), -7, i64)
    assert Lb.nfl_mesh_loops_count(ver, tri, V, T, _inner(out["half_edge"]), _inner(out["twin"]), _inner(out["kind"]), E, tot[2], _inner(sc), nb,
                                   _inner(totals), s) == 0
    L, B, n_open = _unframe(totals, _lib.LOOP_TOTALS, -7, "loop totals").tolist()
    assert (L, B, n_open) == (exp_lp["n_loops"], len(exp_lp["loop_halves"]), exp_lp["n_open"])
    lo = {"loop_offsets": _framed(L + 1, (), -3, i64), "loop_halves": _framed(B, (), -3, i32), "loop_of": _framed(3 * T, (), -3, i32),
          "length": _framed(L, (), -3, i32), "perimeter": _framed(L, (), -3.0, f32), "centroid": _framed(L, (3,), -3.0, f32)}
    assert Lb.nfl_mesh_loops_emit(T, _inner(sc), nb, L, B, *(_inner(lo[k]) for k in LOOP_KEYS), s) == 0
    for k in LOOP_KEYS:
        _same(_unframe(lo[k], len(exp_lp[k]), -3, k), exp_lp[k], k)
    _unframe(sc, nb // 8, 0x5A5A5A5A5A5A5A5A, "loop scratch")
    # fill
    sc, nb = scratch(Lb.nfl_mesh_fill_bytes(L))
    totals = _framed(_lib.FILL_TOTALS, (), -7, i64)
    assert Lb.nfl_mesh_fill_count(L, _inner(lo["length"]), _inner(lo["perimeter"]), None, 2 ** 62, float("inf"), _inner(sc), nb, _inner(totals),
                                  s) == 0
    n_filled, nv, nt = _unframe(totals, _lib.FILL_TOTALS, -7, "fill totals").tolist()
    assert (n_filled, nv, nt) == (exp_info["n_filled"], exp_info["n_new_vertices"], exp_info["n_new_triangles"])
    fo = {"vertices": _framed(V + nv, (3,), -3.0, f32), "normals": _framed(V + nv, (3,), -3.0, f32), "colors": _framed(V + nv, (3,), -3.0, f32),
          "triangles": _framed(T + nt, (3,), -3, i32), "new_vertices": _framed(V + nv, (), 77, u8), "new_triangles": _framed(T + nt, (), 77, u8)}
    assert Lb.nfl_mesh_fill_emit(ver, dev["normals"].data_ptr(), dev["colors"].data_ptr(), tri, V, T, _inner(lo["loop_offsets"]),
                                 _inner(lo["loop_halves"]), _inner(lo["loop_of"]), _inner(lo["centroid"]), L, B, _inner(sc), nb, nv, nt,
                                 *(_inner(fo[k]) for k in fo), s) == 0
    for k in MESH_KEYS:
        _same(_unframe(fo[k], len(exp_mesh[k]), -3, k), exp_mesh[k], k)
    for k in ("new_vertices", "new_triangles"):
        assert np.array_equal(_unframe(fo[k], len(exp_info[k]), 77, k).astype(bool), exp_info[k]), k
    _unframe(sc, nb // 8, 0x5A5A5A5A5A5A5A5A, "fill scratch")
    # a scratch one byte short, and totals the count cannot have given: refused on the device machine as on any other
    assert Lb.nfl_mesh_loops_emit(T, _inner(sc), 8, L, B, *(_inner(lo[k]) for k in LOOP_KEYS), s) == -4
    assert Lb.nfl_mesh_fill_emit(ver, dev["normals"].data_ptr(), dev["colors"].data_ptr(), tri, V, T, _inner(lo["loop_offsets"]),
                                 _inner(lo["loop_halves"]), _inner(lo["loop_of"]), _inner(lo["centroid"]), L, B, _inner(sc), nb, L + 1, nt,
                                 *(_inner(fo[k]) for k in fo), s) == -1


# ---- end to end --------------------------------------------------------------------------------------------------------------------

def test_the_filled_ball_has_an_inside_again_and_a_volume_between_its_bounds(punched):
    mesh, chosen, valence, ball = punched
    dev = _to_dev(mesh)
    filled, info = topology.fill_holes(dev)
    assert info["n_filled"] == 5
    # seeded points at least one lattice spacing (1 / 16) from the surface of radius 0.6, facets and caps included
    rng = np.random.default_rng(9)
    d = rng.standard_normal((400, 3))
    r = np.concatenate([rng.uniform(0.0, 0.5, 200), rng.uniform(0.7, 1.2, 200)])
    pts = _dev(d / np.linalg.norm(d, axis=1, keepdims=True) * r[:, None], F)
    open_votes = solid.inside_mesh(pts, dev, directions=7)["votes"]
    got = solid.inside_mesh(pts, filled, directions=7)
    votes = got["votes"].cpu().numpy()
    print("votes on the open mesh that are not unanimous:", int(((open_votes != 0) & (open_votes != 7)).sum()))
    assert votes[:200].tolist() == [7] * 200 and votes[200:].tolist() == [0] * 200
    assert got["inside"].cpu().numpy().tolist() == [True] * 200 + [False] * 200
    # the volume: a fan's volume is linear in its apex and the centroid is the mean of the loop's vertices, so it is at least that
    # of the lowest fan from one of the loop's own vertices (the polyhedron without the removed vertices); the removed vertices lay
    # outside their caps, so it is at most the closed ball's.  Both from the restatement; the slack is the fp32 rounding of the apex.
    exp_ed = eref.edges(mesh["triangles"], len(mesh["vertices"]))
    exp_lp = eref.loops(mesh["vertices"], mesh["triangles"], exp_ed)
    lower = eref.signed_volume(mesh["vertices"], np.concatenate([mesh["triangles"], eref.lowest_caps(mesh, exp_lp)]))
    upper = eref.signed_volume(ball["vertices"], ball["triangles"])
    volume = float(solid.mesh_volume(filled))
    print(f"volume: {lower:.9f} <= {volume:.9f} <= {upper:.9f}")
    assert 0.8 < lower < upper < 4.0 / 3.0 * np.pi * 0.6 ** 3
    assert lower - 1e-7 <= volume <= upper + 1e-7
    assert abs(volume - eref.signed_volume(*[eref.fill(mesh, exp_lp)[0][k] for k in ("vertices", "triangles")])) < 1e-9


def _bank_of(cams, seed=5):
    """An ImageBank with the cameras `cams` (its pixels are noise: fusion reads the cameras only)."""
    rng = np.random.default_rng(seed)
    images = [rng.integers(0, 256, size=(c["height"], c["width"], 3), dtype=np.uint8) for c in cams]
    K = np.stack([np.array([[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1]], dtype=np.float64) for c in cams])
    c2w = np.stack([c["c2w"].reshape(3, 4).astype(np.float64) for c in cams])
    return ImageBank(images, c2w, K, 2.0, 6.0, device=DEV)


def test_a_fused_mesh_before_and_after_drop_unsupported():
    """The sphere three cameras see, fused on a 17^3 lattice: as extracted the surface carries the sheets where the known
    region ends, and is what it is; drop_unsupported leaves the one closed surface.  Both are held to the restatement, and
    fill_holes closes what the drop leaves open, if anything."""
    fx = tref.sphere_fixture(17, 3, 33)
    box = (tref.BOX[0],) * 3, (tref.BOX[1],) * 3
    out = fusion.fuse_depth(_bank_of(fx["cams"]), _dev(np.stack(fx["depths"]), F), *box, fx["res"], float(fx["trunc"]))
    lat, kn = fusion.tsdf_lattice(out, min_weight=0.5)
    mesh = geometry.extract_surface(lat, 0.0, *box)
    kept = fusion.drop_unsupported(mesh, kn, *box)
    for name, m in (("extracted", mesh), ("kept", kept)):
        host = {k: m[k].cpu().numpy() for k in ("vertices", "normals", "triangles")}
        _check(host, name)
    topo = topology.mesh_topology(kept)
    filled, info = topology.fill_holes(kept)
    after = topology.mesh_topology(filled)
    print("kept:", {k: topo[k] for k in ("closed", "manifold", "oriented", "n_loops", "n_open")}, "filled loops:", info["n_filled"])
    assert topo["manifold"] and topo["oriented"] and topo["n_open"] == 0
    assert after["closed"] and after["manifold"] and after["oriented"] and info["n_filled"] == topo["n_loops"]
    assert (after["euler"][after["triangles"] > 0] == 2).all()
