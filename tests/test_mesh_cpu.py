"""CPU-side checks of the mesh cleaning (nerf_fl_amd.geometry.mesh_components / filter_mesh / clean_mesh,
csrc/nfl_mesh.hip): the numpy restatement (tests/mesh_ref.py), which the GPU tests hold the kernels to, on hand-written
cases and on the three-ball lattice; everything the C entry points refuse before a launch (their structs and signatures
are held to the header in tests/test_abi_cpu.py).  No kernel is launched."""
import ctypes as C

import numpy as np
import pytest

import geometry_ref as gr
import mesh_ref as mr
from abi_probe import L  # noqa: F401  (a fixture)

EINVAL, ESMALL = -1, -4


# ---- the restatement

def test_hand_written_components():
    comp, n, ignored = mr.label(np.zeros((0, 3), int), 0)
    assert comp.shape == (0,) and (n, ignored) == (0, 0)
    comp, n, ignored = mr.label(np.zeros((0, 3), int), 4)                  # V > 0, T = 0: every vertex on its own
    assert comp.tolist() == [0, 1, 2, 3] and (n, ignored) == (4, 0)
    comp, n, ignored = mr.label([[2, 0, 1]], 3)                            # one triangle
    assert comp.tolist() == [0, 0, 0] and (n, ignored) == (1, 0)
    comp, n, ignored = mr.label([[0, 1, 2], [2, 3, 4]], 6)                 # bow-tie: one shared vertex is enough
    assert comp.tolist() == [0, 0, 0, 0, 0, 1] and (n, ignored) == (2, 0)
    comp, n, ignored = mr.label([[3, 3, 5], [1, 1, 1]], 6)                 # repeated indices
    assert comp.tolist() == [0, 1, 2, 3, 4, 3] and (n, ignored) == (5, 0)
    comp, n, ignored = mr.label([[6, 2, 4], [5, 1, 1]], 7)                 # unreferenced 0, 3 between referenced ones
    assert comp.tolist() == [0, 1, 2, 3, 2, 1, 2] and (n, ignored) == (4, 0)
    comp, n, ignored = mr.label([[0, 1, 2], [1, 2, 7], [-1, 0, 3], [3, 4, 5]], 7)      # two triangles out of range
    assert comp.tolist() == [0, 0, 0, 1, 1, 1, 2] and (n, ignored) == (3, 2)


@pytest.mark.parametrize("V", [63, 64, 65, 257, 5000])
def test_permuted_path_is_one_component(V):
    p = np.random.default_rng(V).permutation(V)
    tri = np.stack([p[:-2], p[1:-1], p[2:]], axis=1)
    comp, n, ignored = mr.label(tri, V)
    assert (comp == 0).all() and (n, ignored) == (1, 0)


def test_hand_written_table_and_compaction():
    tri = np.array([[0, 1, 2], [2, 1, 0], [5, 4, 6], [9, 9, 9], [4, 5, 12]], dtype=np.int32)    # the last is ignored
    pos = np.array([[0, 0, 0], [1, -2, 0], [np.nan, 3, np.inf], [7, 7, 7], [-0.0, 1, 1], [0.0, 2, 1], [-1, 1, 1],
                    [5, 5, 5], [6, 6, 6], [np.nan, np.nan, -np.inf]], dtype=np.float32)
    comp, n, ignored = mr.label(tri, 10)
    assert comp.tolist() == [0, 0, 0, 1, 2, 2, 2, 3, 4, 5] and (n, ignored) == (6, 1)
    n_ver, n_tri, bounds = mr.stats(comp, n, pos, tri)
    assert n_ver.tolist() == [3, 1, 3, 1, 1, 1] and n_tri.tolist() == [2, 0, 1, 0, 0, 1]
    assert bounds.dtype == np.float32 and bounds.shape == (6, 2, 3)
    assert bounds[0].tolist() == [[0, -2, 0], [1, 3, 0]]                   # NaN and inf coordinates are skipped
    assert bounds[2].tolist() == [[-1, 1, 1], [0, 2, 1]]
    assert np.signbit(bounds[2, 0, 0]) and not np.signbit(bounds[2, 1, 0])
    assert bounds[5].tolist() == [[np.inf] * 3, [-np.inf] * 3]             # no finite coordinate at all
    mesh = {"vertices": pos, "normals": -pos, "colors": pos + 1, "triangles": tri}
    out = mr.compact(comp, [True, False, True, False, True, False], mesh)
    kept = [0, 1, 2, 4, 5, 6, 8]
    for k, v in (("vertices", pos), ("normals", -pos), ("colors", pos + 1)):
        assert np.array_equal(out[k].view(np.int32), v[kept].view(np.int32)), k
    assert out["triangles"].dtype == np.int32
    assert out["triangles"].tolist() == [[0, 1, 2], [2, 1, 0], [4, 3, 5]]
    none = mr.compact(comp, np.zeros(6, bool), mesh)
    assert none["vertices"].shape == (0, 3) and none["triangles"].shape == (0, 3)


def test_clean_keep_criteria():
    n_tri = np.array([5, 9, 9, 2, 0])
    bounds = np.zeros((5, 2, 3), np.float32)
    bounds[:, 1] = np.arange(5, dtype=np.float32)[:, None]
    assert mr.clean_keep(n_tri, bounds, largest=1).tolist() == [False, True, False, False, False]      # the tie: lower id
    assert mr.clean_keep(n_tri, bounds, largest=3).tolist() == [True, True, True, False, False]
    assert mr.clean_keep(n_tri, bounds, min_triangles=5).tolist() == [True, True, True, False, False]
    assert mr.clean_keep(n_tri, bounds, box=((0, 0, 0), (2, 2, 2))).tolist() == [True, True, True, False, False]
    assert mr.clean_keep(n_tri, bounds, largest=2, box=((0, 0, 0), (1, 1, 1))).tolist() == [False, True, False, False, False]
    bounds[1, :, 2] = np.inf, -np.inf                                       # no finite z: no bounds, inside no box
    assert mr.clean_keep(n_tri, bounds, box=((0, 0, 0), (2, 2, 2))).tolist() == [True, False, True, False, False]


def _edges(tri):
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)


def test_three_balls_on_the_restatements():
    lat, lo, hi, sp, xx = mr.three_balls()
    assert lat.shape == (22, 24, 40)
    mesh = gr.extract(lat, 0.0, lo, sp)
    V, T = len(mesh["vertices"]), len(mesh["triangles"])
    assert (V, T) == (4480, 8948)
    comp, n, ignored = mr.label(mesh["triangles"], V)
    assert (n, ignored) == (3, 0)
    n_ver, n_tri, bounds = mr.stats(comp, n, mesh["vertices"], mesh["triangles"])
    assert n_ver.tolist() == [3346, 158, 976] and n_tri.tolist() == [6688, 312, 1948]
    for c in range(3):                                                     # each closed, Euler characteristic 2
        tri = mesh["triangles"][comp[mesh["triangles"][:, 0]] == c]
        und, cnt = np.unique(np.sort(_edges(tri), axis=1), axis=0, return_counts=True)
        assert (cnt == 2).all() and n_ver[c] - len(und) + len(tri) == 2
        for k in range(3):
            assert bounds[c, 0, k] == mesh["vertices"][comp == c, k].min()
            assert bounds[c, 1, k] == mesh["vertices"][comp == c, k].max()
    # keeping the largest equals, bit for bit, extracting the lattice without the two small balls
    got = mr.compact(comp, mr.clean_keep(n_tri, bounds, largest=1), mesh)
    alone = lat.copy()
    alone[xx >= 0.1] = -1.0
    exp = gr.extract(alone, 0.0, lo, sp)
    for k in ("vertices", "normals", "triangles"):
        assert got[k].shape == exp[k].shape and np.array_equal(got[k].view(np.int32), exp[k].view(np.int32)), k
    assert mr.clean_keep(n_tri, bounds, min_triangles=313).tolist() == [True, False, True]
    assert mr.clean_keep(n_tri, bounds, min_triangles=312).tolist() == [True, True, True]
    assert mr.clean_keep(n_tri, bounds, box=((0.2, -0.2, -0.3), (0.8, 0.4, 0.3))).tolist() == [False, False, True]


# ---- the C ABI, without a GPU

def test_mesh_symbols_bound_and_exported():
    """The stages are exported by the geometry package (the C symbols under them: tests/test_abi_cpu.py)."""
    from nerf_fl_amd import geometry
    for name in ("mesh_components", "filter_mesh", "clean_mesh"):
        assert name in geometry.__all__ and callable(getattr(geometry, name))


def _tiles(n, tile=2048):
    """8 B per tile sum of every scan level above the elements, padded to 16 B."""
    entries, m = 0, -(-n // tile)
    while m > 1:
        entries, m = entries + m, -(-m // tile)
    return -(-entries * 8 // 16) * 16


def test_mesh_scratch_sizes(L):
    pad = lambda b: -(-b // 16) * 16
    for fn in (L.nfl_mesh_label_bytes, L.nfl_mesh_compact_bytes):
        assert fn(-1, 0) == 0 and fn(0, -1) == 0
        assert fn(2 ** 31, 0) == 0 and fn(0, (2 ** 31 - 1) // 3 + 1) == 0
        assert fn(2 ** 31 - 1, (2 ** 31 - 1) // 3) > 0
    assert L.nfl_mesh_label_bytes(0, 0) == 0 and L.nfl_mesh_compact_bytes(0, 0) == 0
    for V, T in ((1, 0), (3, 1), (2048, 7), (2049, 5000), (5_000_000, 9_000_000)):
        assert L.nfl_mesh_label_bytes(V, T) == 2 * pad(4 * V) + pad(8 * V) + _tiles(V)
        assert L.nfl_mesh_compact_bytes(V, T) == pad(4 * V) + pad(8 * V) + pad(4 * T) + pad(8 * T) + max(_tiles(V), _tiles(T))
    assert _tiles(2048) == 0 and _tiles(2049) == 16 and _tiles(2048 * 2048 + 1) == pad(8 * (2049 + 2))


def test_mesh_calls_validate_arguments(L):
    from nerf_fl_amd import _lib
    P = 64                                                                 # never dereferenced: every call below is refused
    big_t = (2 ** 31 - 1) // 3 + 1

    def label(**kw):
        a = _lib.MeshLabelArgs(d_triangles=P, n_vertices=10, n_triangles=4, d_scratch=P,
                               scratch_bytes=L.nfl_mesh_label_bytes(10, 4), d_component=P, d_totals=P)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.nfl_mesh_label(C.byref(a), None)

    assert L.nfl_mesh_label(None, None) == EINVAL
    for bad in (dict(d_triangles=None), dict(d_scratch=None), dict(d_scratch=68), dict(d_component=None), dict(d_totals=None),
                dict(n_vertices=-1), dict(n_triangles=-1), dict(n_vertices=2 ** 31), dict(n_triangles=big_t)):
        assert label(**bad) == EINVAL, bad
    assert label(scratch_bytes=L.nfl_mesh_label_bytes(10, 4) - 1) == ESMALL and label(scratch_bytes=0) == ESMALL
    assert label(n_vertices=0, d_scratch=None, d_component=None, scratch_bytes=0) == 0            # nothing to label
    assert label(n_vertices=0, n_triangles=0, d_triangles=None, d_scratch=None, d_component=None) == 0

    def stats(**kw):
        a = _lib.MeshStatsArgs(d_component=P, d_positions=P, d_triangles=P, n_vertices=10, n_triangles=4, n_components=3,
                               d_n_vertices=P, d_n_triangles=P, d_bounds=P)
        for k, v in kw.items():
            setattr(a, k, v)
        return L.nfl_mesh_stats(C.byref(a), None)

    assert L.nfl_mesh_stats(None, None) == EINVAL
    for bad in (dict(d_component=None), dict(d_positions=None), dict(d_triangles=None), dict(d_n_vertices=None),
                dict(d_n_triangles=None), dict(d_bounds=None), dict(n_vertices=-1), dict(n_triangles=big_t),
                dict(n_components=-1), dict(n_components=11)):
        assert stats(**bad) == EINVAL, bad
    assert stats(n_components=0, d_bounds=None) == 0                       # an empty table: no launch

    def compact(fn, **kw):
        a = _lib.MeshCompactArgs(d_component=P, d_keep=P, d_triangles=P, n_vertices=10, n_triangles=4, n_components=3,
                                 d_scratch=P, scratch_bytes=L.nfl_mesh_compact_bytes(10, 4), d_totals=P,
                                 n_kept_vertices=5, n_kept_triangles=2, d_vertices=P, d_normals=P, d_colors=None,
                                 d_out_vertices=P, d_out_normals=P, d_out_colors=None, d_out_triangles=P)
        for k, v in kw.items():
            setattr(a, k, v)
        return fn(C.byref(a), None)

    for fn in (L.nfl_mesh_compact_count, L.nfl_mesh_compact_emit):
        assert fn(None, None) == EINVAL
        for bad in (dict(d_component=None), dict(d_keep=None), dict(d_triangles=None), dict(d_scratch=None), dict(d_scratch=68),
                    dict(n_vertices=-1), dict(n_vertices=2 ** 31), dict(n_triangles=big_t), dict(n_components=-1),
                    dict(n_components=11)):
            assert compact(fn, **bad) == EINVAL, bad
        assert compact(fn, scratch_bytes=L.nfl_mesh_compact_bytes(10, 4) - 1) == ESMALL
    assert compact(L.nfl_mesh_compact_count, d_totals=None) == EINVAL
    emit = L.nfl_mesh_compact_emit
    for bad in (dict(n_kept_vertices=-1), dict(n_kept_triangles=-1), dict(n_kept_vertices=11), dict(n_kept_triangles=5),
                dict(d_out_vertices=None), dict(d_out_normals=None), dict(d_out_triangles=None),
                dict(d_colors=P, d_out_colors=None)):
        assert compact(emit, **bad) == EINVAL, bad
    assert compact(emit, n_kept_vertices=0, n_kept_triangles=0, d_out_vertices=None, d_out_normals=None,
                   d_out_triangles=None) == 0                              # totals of 0: no launch


def test_mesh_functions_reject_host_inputs():
    import torch
    from nerf_fl_amd import geometry
    mesh = {"vertices": torch.zeros(3, 3), "normals": torch.zeros(3, 3), "triangles": torch.zeros(1, 3, dtype=torch.int32)}
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.mesh_components(mesh)
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.filter_mesh(mesh, torch.ones(1, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="no CPU path"):
        geometry.clean_mesh(mesh, largest=1)
    with pytest.raises(ValueError):
        geometry.mesh_components({"vertices": torch.zeros(3, 3)})
    assert geometry.clean_mesh(mesh) is mesh                               # no criterion: the input, unchanged
