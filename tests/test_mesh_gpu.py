"""GPU checks of the mesh cleaning (csrc/nfl_mesh.hip through nerf_fl_amd.geometry): component ids, the per-component
table and the compacted buffers against the numpy restatement of tests/mesh_ref.py, or against closed forms where the
mesh is large.  Everything compared is an integer or a copied float: equality is EXACT, there is no tolerance.

Sizes.  The library's scan works on tiles of TILE = 2048 elements and has three levels: one tile (n <= 2048), tile sums
scanned by one tile (n <= 2048^2 = 4 194 304), and a third level above that.  The small cases sit in the first, the
5 000-vertex chain in the second, and the scale cases have V = 3 T = 4 194 306 vertices: the smallest multiple of 3
above 2048^2, so the vertex scans of label and compact reach the third.  Kernels run 256 threads (4 waves) a workgroup:
63 / 64 / 65 cross a wave, 257 a workgroup."""
import ctypes as C

import numpy as np
import pytest
import torch

import geometry_ref as gr
import mesh_ref as mr
import nerf_fl_amd
from geom_gpu_util import bits as _bits, same as _same, to_dev as _to_dev
from gpu_util import DEV, make_embeddings
from nerf_fl_amd import NeRF, _lib, geometry, rendering, synth

pytestmark = pytest.mark.gpu

TILE = 2048
T_SCALE = (TILE * TILE) // 3 + 1                    # 1 398 102 triangles, 4 194 306 vertices
assert 3 * T_SCALE > TILE * TILE >= 3 * (T_SCALE - 1)


def _positions(V, seed):
    rng = np.random.default_rng(seed)
    pos = rng.standard_normal((V, 3)).astype(np.float32)
    if V >= 8:                                      # what the bounds have to step over or tell apart
        pos[1, 0], pos[2, 1], pos[3, 2], pos[4, 0], pos[5, 0] = np.nan, np.inf, -np.inf, -0.0, 0.0
    return pos


def _device_mesh(tri, pos, colors=True):
    tri = np.asarray(tri, dtype=np.int32).reshape(-1, 3)
    mesh = {"vertices": pos, "normals": (pos * np.float32(0.5)), "triangles": tri}
    if colors:
        mesh["colors"] = np.abs(pos) + np.float32(1)
    return mesh, _to_dev(mesh)


def _check(tri, V, what, seed=0, colors=True):
    """mesh_components and filter_mesh (odd components, then a seeded random choice) against the restatement."""
    host, dev = _device_mesh(tri, _positions(V, seed), colors)
    comp, n, ignored = mr.label(host["triangles"], V)
    assert ignored == 0
    n_ver, n_tri, bounds = mr.stats(comp, n, host["vertices"], host["triangles"])
    got = geometry.mesh_components(dev)
    assert got["n_components"] == n, what
    _same(got["component"], comp, what)
    _same(got["vertices"], n_ver, what)
    _same(got["triangles"], n_tri, what)
    _same(got["bounds"], bounds, what)
    for keep in (np.arange(n) % 2 == 1, np.random.default_rng(seed + 1).random(n) < 0.6):
        exp = mr.compact(comp, keep, host)
        out = geometry.filter_mesh(dev, torch.from_numpy(keep).to(DEV), got)
        assert set(out) == set(exp), what
        for k in exp:
            _same(out[k], exp[k].reshape(-1, 3), (what, k))
    return got


# ---- small cases

def test_empty_mesh():
    got = _check(np.zeros((0, 3)), 0, "empty")
    assert got["n_components"] == 0 and got["component"].shape == (0,) and got["bounds"].shape == (0, 2, 3)


def test_vertices_without_triangles():
    got = _check(np.zeros((0, 3)), 9, "V = 9, T = 0")
    assert got["component"].tolist() == list(range(9)) and got["triangles"].tolist() == [0] * 9


def test_one_triangle():
    got = _check([[2, 0, 1]], 3, "one triangle", colors=False)
    assert got["component"].tolist() == [0, 0, 0] and got["vertices"].tolist() == [3] and got["triangles"].tolist() == [1]


def test_bow_tie():
    got = _check([[0, 1, 2], [2, 3, 4]], 6, "bow-tie")
    assert got["component"].tolist() == [0, 0, 0, 0, 0, 1]


def test_repeated_indices():
    got = _check([[3, 3, 5], [1, 1, 1], [7, 6, 7]], 8, "repeated indices")
    assert got["component"].tolist() == [0, 1, 2, 3, 4, 3, 5, 5]


def test_unreferenced_vertices_between_referenced_ones():
    got = _check([[6, 2, 4], [5, 1, 1], [8, 9, 6]], 11, "unreferenced")
    assert got["component"].tolist() == [0, 1, 2, 3, 2, 1, 2, 4, 2, 2, 5]


def _label_abi(tri, V, guard=64):
    """nfl_mesh_label through the C ABI, its outputs in the middle of buffers of sentinels."""
    lib = _lib.lib()
    T = tri.shape[0]
    component = torch.full((V + 2 * guard,), -7, dtype=torch.int32, device=DEV)
    totals = torch.full((2 + 2 * guard,), -7, dtype=torch.int64, device=DEV)
    nbytes = lib.nfl_mesh_label_bytes(V, T)
    scratch = torch.full((nbytes // 8 + 2 * guard,), -7, dtype=torch.int64, device=DEV)
    a = _lib.MeshLabelArgs()
    a.d_triangles, a.n_vertices, a.n_triangles = tri.data_ptr(), V, T
    a.d_scratch, a.scratch_bytes = scratch[guard:].data_ptr(), nbytes
    a.d_component, a.d_totals = component[guard:].data_ptr(), totals[guard:].data_ptr()
    _lib.check(lib.nfl_mesh_label(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_mesh_label")
    torch.cuda.synchronize()
    for buf, n in ((component, V), (totals, 2), (scratch, nbytes // 8)):
        assert (buf[:guard] == -7).all() and (buf[guard + n:] == -7).all()          # nothing written out of range
    return component[guard:guard + V].contiguous(), totals[guard:guard + 2].tolist()


def test_out_of_range_triangle():
    V = 70
    tri = np.array([[0, 1, 2], [3, 4, V], [5, 6, 7], [8, -1, 9], [7, 20, 69], [2 ** 31 - 1, 0, 1]], dtype=np.int32)
    host, dev = _device_mesh(tri, _positions(V, 4))
    with pytest.raises(ValueError, match="3 of 6 triangles"):
        geometry.mesh_components(dev)
    with pytest.raises(ValueError, match="1 of 1 triangles"):
        geometry.mesh_components(_device_mesh([[0, 1, 2]], np.zeros((0, 3), np.float32))[1])     # V = 0
    comp, n, ignored = mr.label(tri, V)
    assert ignored == 3
    got, totals = _label_abi(dev["triangles"], V)
    assert totals == [n, 3]
    _same(got, comp, "ids with ignored triangles")
    # the ignored triangles are dropped by the compaction too
    keep = np.ones(n, dtype=bool)
    keep[1] = False
    out = geometry.filter_mesh(dev, torch.from_numpy(keep).to(DEV), {"component": got, "n_components": n})
    exp = mr.compact(comp, keep, host)
    assert len(exp["triangles"]) == 3
    for k in exp:
        _same(out[k], exp[k].reshape(-1, 3), k)


def test_argument_checks():
    _, dev = _device_mesh([[0, 1, 2]], _positions(3, 0))
    comps = geometry.mesh_components(dev)
    with pytest.raises(ValueError):
        geometry.filter_mesh(dev, torch.ones(2, dtype=torch.bool, device=DEV), comps)            # C is 1
    with pytest.raises(ValueError):
        geometry.filter_mesh(dev, torch.ones(1, dtype=torch.uint8, device=DEV), comps)
    with pytest.raises(RuntimeError):
        geometry.filter_mesh(dev, torch.ones(1, dtype=torch.bool), comps)
    with pytest.raises(ValueError):
        geometry.mesh_components(dict(dev, triangles=dev["triangles"].long()))
    with pytest.raises(ValueError):
        geometry.mesh_components(dict(dev, vertices=dev["vertices"].t().contiguous().t()))
    with pytest.raises(ValueError):
        geometry.clean_mesh(dev, box=((0, 0), (1, 1)))
    assert geometry.clean_mesh(dev) is dev


def test_box_rejects_a_component_without_bounds():
    """A component with no finite coordinate on an axis keeps +inf / -inf there; those compare as 'inside' any box
    (+inf >= lo, -inf <= hi), and clean_mesh must not take them so."""
    pos = np.zeros((9, 3), dtype=np.float32)
    pos[3:6, 1] = np.nan                                                    # the second triangle: no finite y
    pos[6:9] = 5.0                                                          # the third: outside the box
    host, dev = _device_mesh([[0, 1, 2], [3, 4, 5], [6, 7, 8]], pos)
    comps = geometry.mesh_components(dev)
    assert comps["bounds"][1, :, 1].tolist() == [np.inf, -np.inf]
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    assert mr.clean_keep(comps["triangles"].cpu().numpy(), comps["bounds"].cpu().numpy(), box=box).tolist() == [True, False, False]
    got = geometry.clean_mesh(dev, box=box)
    exp = mr.compact(comps["component"].cpu().numpy(), np.array([True, False, False]), host)
    for k in exp:
        _same(got[k], exp[k].reshape(-1, 3), k)


def test_emit_checks_what_it_reads():
    """nfl_mesh_compact_emit is owed the arguments and the scratch of the count call.  Given other triangles, some with
    indices outside [0, V), it skips those rows: they stay as they were, and nothing is read or written out of range."""
    V, guard = 70, 64
    good = np.arange(60, dtype=np.int32).reshape(20, 3)
    other = good.copy()
    other[3], other[7], other[11] = (0, 1, V), (-1, 4, 5), (2 ** 31 - 1, 6, 7)
    _, dev = _device_mesh(good, _positions(V, 5), colors=False)
    comps = geometry.mesh_components(dev)
    lib, n = _lib.lib(), comps["n_components"]
    keep = torch.ones(n, dtype=torch.uint8, device=DEV)
    nbytes = lib.nfl_mesh_compact_bytes(V, 20)
    scratch = torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=DEV)
    totals = torch.empty(2, dtype=torch.int64, device=DEV)
    out_v = torch.full((V + 2 * guard, 3), -7.0, dtype=torch.float32, device=DEV)
    out_t = torch.full((20 + 2 * guard, 3), -7, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = _lib.MeshCompactArgs()
    a.d_component, a.d_keep, a.d_triangles = comps["component"].data_ptr(), keep.data_ptr(), dev["triangles"].data_ptr()
    a.n_vertices, a.n_triangles, a.n_components = V, 20, n
    a.d_scratch, a.scratch_bytes, a.d_totals = scratch.data_ptr(), nbytes, totals.data_ptr()
    _lib.check(lib.nfl_mesh_compact_count(C.byref(a), stream), "nfl_mesh_compact_count")
    assert totals.tolist() == [V, 20]
    bad = torch.from_numpy(other).to(DEV)
    a.d_triangles, a.n_kept_vertices, a.n_kept_triangles = bad.data_ptr(), V, 20
    a.d_vertices, a.d_out_vertices, a.d_out_triangles = dev["vertices"].data_ptr(), out_v[guard:].data_ptr(), out_t[guard:].data_ptr()
    _lib.check(lib.nfl_mesh_compact_emit(C.byref(a), stream), "nfl_mesh_compact_emit")
    torch.cuda.synchronize()
    exp = np.full((20 + 2 * guard, 3), -7, dtype=np.int32)
    exp[guard:guard + 20] = good
    exp[[guard + 3, guard + 7, guard + 11]] = -7
    _same(out_t, exp, "triangles")
    _same(out_v[guard:guard + V], dev["vertices"], "vertices")
    assert (out_v[:guard] == -7).all() and (out_v[guard + V:] == -7).all()


# ---- chains: long parent paths, hooks that cross waves and workgroups

@pytest.mark.parametrize("V", [63, 64, 65, 257, 5000])
def test_permuted_path(V):
    p = np.random.default_rng(V).permutation(V)
    got = _check(np.stack([p[:-2], p[1:-1], p[2:]], axis=1), V, f"path {V}", seed=V)
    assert got["n_components"] == 1 and got["vertices"].tolist() == [V] and got["triangles"].tolist() == [V - 2]


def test_two_permuted_paths_and_specks():
    """Several components whose vertices interleave, so that ids, table rows and the compaction's remapping all differ
    from the identity."""
    V = 3001
    p = np.random.default_rng(8).permutation(V)
    a, b = p[:1400], p[1400:2900]                                           # 101 vertices stay on their own
    tri = np.concatenate([np.stack([q[:-2], q[1:-1], q[2:]], axis=1) for q in (a, b)])
    got = _check(tri, V, "two paths", seed=9)
    assert got["n_components"] == 103


# ---- scale: closed forms, computed on the device

def _isolated(T):
    tri = torch.arange(3 * T, dtype=torch.int32, device=DEV).view(T, 3)
    v = torch.arange(3 * T, dtype=torch.float32, device=DEV)               # exact: 3 T < 2^24
    pos = torch.stack([v, -(v + 1), v % 7], dim=1).contiguous()
    return {"vertices": pos, "normals": (pos + 0.5).contiguous(), "triangles": tri}


@pytest.fixture(scope="module")
def isolated():
    assert 3 * T_SCALE < 2 ** 24
    mesh = _isolated(T_SCALE)
    return mesh, geometry.mesh_components(mesh)


def test_isolated_triangles(isolated):
    """Triangle i = (3 i, 3 i + 1, 3 i + 2) has id i."""
    mesh, got = isolated
    T = T_SCALE
    assert got["n_components"] == T
    assert torch.equal(got["component"], torch.arange(3 * T, device=DEV, dtype=torch.int32) // 3)
    assert (got["vertices"] == 3).all() and (got["triangles"] == 1).all()
    rows = mesh["vertices"].view(T, 3, 3)
    assert torch.equal(got["bounds"][:, 0], rows.amin(dim=1)) and torch.equal(got["bounds"][:, 1], rows.amax(dim=1))


def test_keeping_odd_components(isolated):
    mesh, comps = isolated
    T = T_SCALE
    keep = torch.arange(T, device=DEV) % 2 == 1
    out = geometry.filter_mesh(mesh, keep, comps)
    Tk = T // 2
    assert out["triangles"].shape == (Tk, 3) and out["vertices"].shape == (3 * Tk, 3) and "colors" not in out
    assert torch.equal(out["triangles"], torch.arange(3 * Tk, dtype=torch.int32, device=DEV).view(Tk, 3))
    for k in ("vertices", "normals"):
        assert torch.equal(out[k], mesh[k].view(T, 9)[1::2].reshape(-1, 3)), k


def test_fan_joins_the_first_half():
    """The isolated triangles plus the fan (0, 3 i, 3 i + 1), i = 1 .. H - 1: the first H triangles become one component
    (every hook ends at vertex 0, every table update of half the mesh goes to row 0), the others move down by H - 1."""
    T, H = T_SCALE, T_SCALE // 2
    mesh = _isolated(T)
    i = torch.arange(1, H, dtype=torch.int32, device=DEV)
    fan = torch.stack([torch.zeros_like(i), 3 * i, 3 * i + 1], dim=1)
    mesh["triangles"] = torch.cat([mesh["triangles"], fan]).contiguous()
    got = geometry.mesh_components(mesh)
    C_exp = T - H + 1
    assert got["n_components"] == C_exp
    v = torch.arange(3 * T, device=DEV, dtype=torch.int32)
    assert torch.equal(got["component"], torch.where(v < 3 * H, torch.zeros_like(v), v // 3 - (H - 1)))
    assert got["vertices"][0].item() == 3 * H and (got["vertices"][1:] == 3).all()
    assert got["triangles"][0].item() == 2 * H - 1 and (got["triangles"][1:] == 1).all()
    first = mesh["vertices"][:3 * H]
    assert torch.equal(got["bounds"][0, 0], first.amin(dim=0)) and torch.equal(got["bounds"][0, 1], first.amax(dim=0))
    rows = mesh["vertices"][3 * H:].view(T - H, 3, 3)
    assert torch.equal(got["bounds"][1:, 0], rows.amin(dim=1)) and torch.equal(got["bounds"][1:, 1], rows.amax(dim=1))
    # dropping the giant leaves the second half, re-indexed from 0
    keep = torch.ones(C_exp, dtype=torch.bool, device=DEV)
    keep[0] = False
    out = geometry.filter_mesh(mesh, keep, got)
    assert torch.equal(out["triangles"], torch.arange(3 * (T - H), dtype=torch.int32, device=DEV).view(T - H, 3))
    assert torch.equal(out["vertices"], mesh["vertices"][3 * H:])


# ---- invariance

def test_triangle_order_does_not_matter_and_runs_repeat():
    V = 3001
    rng = np.random.default_rng(21)
    p = rng.permutation(V)
    tri = np.concatenate([np.stack([q[:-2], q[1:-1], q[2:]], axis=1) for q in (p[:900], p[900:2500], p[2500:2990])])
    pos = _positions(V, 22)
    _, a = _device_mesh(tri, pos)
    _, b = _device_mesh(tri[rng.permutation(len(tri))], pos)
    one, again, shuffled = geometry.mesh_components(a), geometry.mesh_components(a), geometry.mesh_components(b)
    assert one["n_components"] == again["n_components"] == shuffled["n_components"] == 3 + 11
    for k in ("component", "vertices", "triangles", "bounds"):
        _same(again[k], _bits(one[k]), k)                                   # two runs: identical bits
        _same(shuffled[k], _bits(one[k]), k)                                # rows permuted: the same ids and table
    keep = torch.arange(one["n_components"], device=DEV) % 3 != 0
    f1, f2 = geometry.filter_mesh(a, keep, one), geometry.filter_mesh(a, keep, again)
    for k in f1:
        _same(f2[k], _bits(f1[k]), k)


# ---- end to end

@pytest.fixture(scope="module")
def balls():
    lat, lo, hi, sp, xx = mr.three_balls()
    mesh = geometry.extract_surface(torch.from_numpy(lat).to(DEV), 0.0, lo, hi)
    return lat, lo, hi, sp, xx, mesh


def test_three_balls_components(balls):
    lat, lo, hi, sp, xx, mesh = balls
    assert mesh["vertices"].shape == (4480, 3) and mesh["triangles"].shape == (8948, 3)
    got = geometry.mesh_components(mesh)
    assert got["n_components"] == 3
    assert got["vertices"].tolist() == [3346, 158, 976] and got["triangles"].tolist() == [6688, 312, 1948]
    host = {k: v.cpu().numpy() for k, v in mesh.items()}
    comp, n, _ = mr.label(host["triangles"], 4480)
    _same(got["component"], comp, "ids")
    _same(got["bounds"], mr.stats(comp, n, host["vertices"], host["triangles"])[2], "bounds")


def test_three_balls_largest_is_the_big_ball_alone(balls):
    lat, lo, hi, sp, xx, mesh = balls
    got = geometry.clean_mesh(mesh, largest=1)
    alone = lat.copy()
    alone[xx >= 0.1] = -1.0
    exp = geometry.extract_surface(torch.from_numpy(alone).to(DEV), 0.0, lo, hi)
    assert set(got) == {"vertices", "normals", "triangles"}
    assert got["vertices"].shape == (3346, 3) and got["triangles"].shape == (6688, 3)
    for k in exp:
        _same(got[k], _bits(exp[k]), k)                                     # bit for bit


def test_three_balls_by_size_and_by_box(balls):
    lat, lo, hi, sp, xx, mesh = balls
    host = {k: v.cpu().numpy() for k, v in mesh.items()}
    comp, n, _ = mr.label(host["triangles"], 4480)
    for kw, kept in ((dict(min_triangles=313), [True, False, True]), (dict(min_triangles=312), [True, True, True]),
                     (dict(box=((0.2, -0.2, -0.3), (0.8, 0.4, 0.3))), [False, False, True]),
                     (dict(largest=2, min_triangles=2000), [True, False, False]), (dict(largest=0), [False] * 3)):
        got = geometry.clean_mesh(mesh, **kw)
        exp = mr.compact(comp, np.array(kept), host)
        for k in exp:
            _same(got[k], exp[k].reshape(-1, 3), (kw, k))


def test_sized_calls_read_the_device_once(balls, monkeypatch):
    """The host synchronisations of the sized calls, counted: one each, as their docstrings say, two for clean_mesh, and
    none for the empty mesh, which launches no counting half either.  Reads of device values (tolist, item, cpu) are
    counted and let through; torch's synchronisation check raises on any other.  The entry points called are recorded from
    the status check every launch goes through."""
    lat, lo, hi, sp, xx, mesh = balls
    reads, calls = [], []
    for name in ("tolist", "item", "cpu"):
        def counted(self, *args, _real=getattr(torch.Tensor, name), _name=name, **kwargs):
            if not self.is_cuda:
                return _real(self, *args, **kwargs)
            reads.append(_name)
            torch.cuda.set_sync_debug_mode("default")
            try:
                return _real(self, *args, **kwargs)
            finally:
                torch.cuda.set_sync_debug_mode("error")
        monkeypatch.setattr(torch.Tensor, name, counted)
    real_check = _lib.check
    monkeypatch.setattr(_lib, "check", lambda code, what: (calls.append(what), real_check(code, what))[1])

    def counts(fn):
        del reads[:], calls[:]
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            out = fn()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        return out, len(reads), list(calls)

    d_lat = torch.from_numpy(lat).to(DEV)
    comps = geometry.mesh_components(mesh)
    keep = torch.arange(comps["n_components"], device=DEV) != 1
    _, empty = _device_mesh(np.zeros((0, 3)), _positions(0, 0))
    none = {"component": torch.empty(0, dtype=torch.int32, device=DEV), "n_components": 0}
    no_keep = torch.ones(0, dtype=torch.bool, device=DEV)
    try:
        for what, fn, n_reads, entries in (
                ("extract_surface", lambda: geometry.extract_surface(d_lat, 0.0, lo, hi), 1, ["nfl_surface_count", "nfl_surface_emit"]),
                ("extract_surface, no crossing", lambda: geometry.extract_surface(d_lat, 1e9, lo, hi), 1,
                 ["nfl_surface_count", "nfl_surface_emit"]),
                ("mesh_components", lambda: geometry.mesh_components(mesh), 1, ["nfl_mesh_label", "nfl_mesh_stats"]),
                ("filter_mesh", lambda: geometry.filter_mesh(mesh, keep, components=comps), 1,
                 ["nfl_mesh_compact_count", "nfl_mesh_compact_emit"]),
                ("simplify_mesh", lambda: geometry.simplify_mesh(mesh, 0.1), 1, ["nfl_mesh_simplify_count", "nfl_mesh_simplify_emit"]),
                ("mesh_adjacency", lambda: geometry.mesh_adjacency(mesh), 1, ["nfl_mesh_adjacency_count", "nfl_mesh_adjacency_emit"]),
                ("clean_mesh", lambda: geometry.clean_mesh(mesh, min_triangles=1), 2,
                 ["nfl_mesh_label", "nfl_mesh_stats", "nfl_mesh_compact_count", "nfl_mesh_compact_emit"]),
                # the empty mesh: nothing is read back, no counting half runs (nfl_mesh_stats of no component sizes nothing)
                ("empty mesh_components", lambda: geometry.mesh_components(empty), 0, ["nfl_mesh_stats"]),
                ("empty filter_mesh", lambda: geometry.filter_mesh(empty, no_keep, components=none), 0, []),
                ("empty simplify_mesh", lambda: geometry.simplify_mesh(empty, 0.1), 0, []),
                ("empty mesh_adjacency", lambda: geometry.mesh_adjacency(empty), 0, []),
                ("empty clean_mesh", lambda: geometry.clean_mesh(empty, min_triangles=1), 0, ["nfl_mesh_stats"])):
            out, got_reads, got_entries = counts(fn)
            print(f"{what}: {got_reads} host reads, entry points {got_entries}")
            assert (got_reads, got_entries) == (n_reads, entries), what
    finally:
        monkeypatch.undo()
    assert geometry.extract_surface(d_lat, 1e9, lo, hi)["vertices"].shape == (0, 3)
    assert geometry.mesh_adjacency(empty)["offsets"].tolist() == [0]


def test_extract_mesh_filters_before_colouring():
    nerf_fl_amd.set_precision("f16x3")
    try:
        rendering.check_status(DEV)
    except FloatingPointError:
        pass
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(DEV)
    emb = make_embeddings(10, False)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (16, 16, 16)
    with torch.no_grad():
        lattice = geometry.density_lattice(model, emb, lo, hi, res)
        iso = lattice.median().item()
        plain = geometry.extract_surface(lattice, iso, lo, hi)
        plain["colors"] = geometry.surface_colors(model, emb, plain["vertices"], plain["normals"])
        default = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso)
        assert set(default) == set(plain)
        for k in plain:
            _same(default[k], _bits(plain[k]), k)                           # the defaults do what they did
        comps = geometry.mesh_components(plain)
        assert comps["n_components"] > 1                                    # else the filter has nothing to drop
        cleaned = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, largest=1)
        exp = geometry.clean_mesh({k: plain[k] for k in ("vertices", "normals", "triangles")}, largest=1)
        Vk = int(comps["vertices"][comps["triangles"].to(torch.int64).argmax()].item())
        assert 0 < Vk < plain["vertices"].shape[0] and cleaned["colors"].shape == (Vk, 3)
        for k in exp:
            _same(cleaned[k], _bits(exp[k]), k)
        _same(cleaned["colors"], _bits(geometry.surface_colors(model, emb, exp["vertices"], exp["normals"])), "colors")
        by_size = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, min_triangles=10 ** 9)
        assert by_size["vertices"].shape == by_size["colors"].shape == (0, 3) and by_size["triangles"].shape == (0, 3)
    rendering.check_status(DEV)
