"""CPU-side checks of the mesh edges (nerf_fl_amd.topology, csrc/nfl_meshedge.hip): the new symbols and constants are in _lib's
tables and the header, which gains no struct; every C entry point refuses bad arguments before any launch; the module stands
beside solid.py; the numpy restatement (tests/meshedge_ref.py), which the GPU tests hold the kernels to, is checked on hand
cases whose tables are written out, under permutations of the triangles, and on closed surfaces whose genus is known; filling
the holes punched into a ball closes it again.  No kernel is launched."""
import os
import re

import numpy as np
import pytest

import meshedge_ref as eref
import meshsmooth_ref as sref
from abi_probe import HEADER, L, declared, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf_fl_amd", "csrc")
F = np.float32
EINVAL, ESMALL = -1, -4
I, B, X, N = eref.INTERIOR, eref.BOUNDARY, eref.FLIPPED, eref.NONMANIFOLD
NEW = ("nfl_mesh_edges_bytes", "nfl_mesh_edges_count", "nfl_mesh_edges_emit", "nfl_mesh_loops_bytes", "nfl_mesh_loops_count",
       "nfl_mesh_loops_emit", "nfl_mesh_fill_bytes", "nfl_mesh_fill_count", "nfl_mesh_fill_emit")


# ---- tables and sources ---------------------------------------------------------------------------------------------------------

def test_the_tables_and_the_header_name_the_new_entry_points_and_no_new_struct():
    names = [s[0] for s in _lib.SYMBOLS]
    assert set(NEW) <= set(names) and set(NEW) <= set(declared()["functions"])
    assert len(declared()["structs"]) == 42 == len(_lib.STRUCTS)
    text = open(HEADER).read()
    assert "#define NFL_ABI_VERSION 10\n" in text and _lib.NFL_ABI_VERSION == 10
    assert text.index("---- mesh solid:") < text.index("/* ---- mesh edges:") < text.index("---- hierarchical sampling")
    section = text[text.index("/* ---- mesh edges:"):text.index("---- hierarchical sampling")]
    for word in ("HALF-EDGE", "EDGE:", "KIND", "TWIN", "SUCCESSOR", "LOOP:", "THE TABLE", "FILL.", "NFL_EINVAL", "NFL_ESMALL"):
        assert word in section, word


def test_the_constants_are_the_header_s():
    c = probe()["constants"]
    assert _lib.EDGE_KINDS == {"interior": I, "boundary": B, "flipped": X, "nonmanifold": N}
    assert [c["NFL_EDGE_INTERIOR"], c["NFL_EDGE_BOUNDARY"], c["NFL_EDGE_FLIPPED"], c["NFL_EDGE_NONMANIFOLD"]] == [I, B, X, N]
    assert c["NFL_EDGE_SHORT_ROW"] == _lib.EDGE_SHORT_ROW == 8
    assert (c["NFL_EDGE_TOTALS"], c["NFL_LOOP_TOTALS"], c["NFL_FILL_TOTALS"]) == (7, 3, 3) == (_lib.EDGE_TOTALS, _lib.LOOP_TOTALS, _lib.FILL_TOTALS)
    for name in ("NFL_EDGE_INTERIOR", "NFL_EDGE_BOUNDARY", "NFL_EDGE_FLIPPED", "NFL_EDGE_NONMANIFOLD", "NFL_EDGE_SHORT_ROW",
                 "NFL_EDGE_TOTALS", "NFL_LOOP_TOTALS", "NFL_FILL_TOTALS"):
        assert name in _lib.CONSTANTS


def test_the_unit_is_built_by_the_common_rule_and_stands_apart_from_the_render_path():
    make = open(os.path.join(CSRC, "Makefile")).read()
    objs = re.search(r"^OBJS = (.*?)\n\n", make, flags=re.S | re.M).group(1)
    assert "nfl_meshedge.o" in objs.split() or "nfl_meshedge.o" in objs.replace("\\", " ").split()
    assert re.search(r"^nfl_meshedge\.o:.*\bnfl_geom\.h nfl_geom_layout\.h$", make, flags=re.M) or \
        re.search(r"^nfl_surface\.o .*nfl_meshedge\.o.*: nfl_geom\.h nfl_geom_layout\.h$", make, flags=re.M)
    assert not re.search(r"^nfl_meshedge\.o:.*\n\t", make, flags=re.M)       # no recipe of its own
    assert "%.o: %.hip" in make and "-ffp-contract=off" in make
    unit = open(os.path.join(CSRC, "nfl_meshedge.hip")).read()
    includes = re.findall(r'^#include [<"]([^>"]+)[>"]', unit, flags=re.M)
    assert "nfl_geom.h" in includes
    for banned in ("nfl_mlp.h", "nfl_render_impl.h", "nfl_math.h", "nfl_plan.h", "nfl_trigrid.h"):
        assert banned not in includes, banned
    assert "hipDeviceGetAttribute" not in unit and "hipFuncSetAttribute" not in unit and "hipMemsetAsync" not in unit
    assert "solid" not in "nfl_meshedge.hip"
    for name in NEW:
        assert f'extern "C" {"size_t" if name.endswith("_bytes") else "int"} {name}(' in unit, name
    layout = open(os.path.join(CSRC, "nfl_geom_layout.h")).read()
    assert "ne_layout" in layout and "nl_layout" in layout and "nf_layout" in layout
    assert "hip" not in re.sub(r"//.*", "", layout).lower()                   # plain C++


def test_the_module_stands_beside_solid():
    source = open(os.path.join(ROOT, "nerf_fl_amd", "topology.py")).read()
    assert "_lib.check(" not in source and "C.byref(" not in source and "ctypes" not in source and "numpy" not in source
    assert ".item()" not in source and ".cpu()" not in source
    assert source.count(".tolist()") == 1 and "THE host read" in source.split(".tolist()")[1].split("\n")[0]
    code = re.sub(r'""".*?"""', "", source, flags=re.S)
    assert code.count(".tolist()") == 1 and code.split(".tolist()")[0].rsplit("\ndef ", 1)[1].startswith("_totals(")
    for helper in ("_call", "_is", "_mesh_tensors", "_on_device", "_ptr", "_scratch", "_refuse_outside"):
        assert re.search(rf"^from \.geometry\._call import .*\b{helper}\b", source, flags=re.M), helper
    from nerf_fl_amd import geometry, topology
    assert topology.__all__ == ["mesh_edges", "mesh_topology", "boundary_loops", "fill_holes"]
    assert len(geometry.__all__) == 24
    assert sorted(n for n in os.listdir(os.path.join(ROOT, "nerf_fl_amd", "geometry")) if n.endswith(".py")) == sorted(
        ["__init__.py", "_call.py", "atlas.py", "image.py", "io.py", "lattice.py", "mesh.py"]) or \
        len([n for n in os.listdir(os.path.join(ROOT, "nerf_fl_amd", "geometry")) if n.endswith(".py")]) == 7


# ---- C refusals: every pointer is a made-up address, so a launch would fault and a refusal can only come from the host check ----

BIG_T = (2 ** 31 - 1) // 3 + 1


def _edges_count_args():
    return dict(d_triangles=0x1000, V=30, T=10, d_offsets=0x2000, d_neighbors=0x3000, N=40, d_scratch=0x4000, scratch_bytes=1 << 30,
                d_totals=0x5000)


def _edges_emit_args():
    return dict(d_triangles=0x1000, V=30, T=10, d_scratch=0x4000, scratch_bytes=1 << 30, E=20, H=30, d_edges=0x5000, d_half_edge=0x6000,
                d_edge_offsets=0x7000, d_edge_halves=0x8000, d_kind=0x9001, d_twin=0xA000)


def _loops_count_args():
    return dict(d_vertices=0x1000, d_triangles=0x2000, V=30, T=10, d_half_edge=0x3000, d_twin=0x4000, d_kind=0x5001, E=20, n_boundary=6,
                d_scratch=0x6000, scratch_bytes=1 << 30, d_totals=0x7000)


def _loops_emit_args():
    return dict(T=10, d_scratch=0x6000, scratch_bytes=1 << 30, L=2, Bp=6, d_loop_offsets=0x1000, d_loop_halves=0x2000, d_loop_of=0x3000,
                d_length=0x4000, d_perimeter=0x5000, d_centroid=0x7000)


def _fill_count_args():
    return dict(L=2, d_length=0x1000, d_perimeter=0x2000, d_keep=0x3001, max_edges=8, max_perimeter=1.0, d_scratch=0x4000,
                scratch_bytes=1 << 30, d_totals=0x5000)


def _fill_emit_args():
    return dict(d_vertices=0x1000, d_normals=0x2000, d_colors=0x3000, d_triangles=0x4000, V=30, T=10, d_loop_offsets=0x5000,
                d_loop_halves=0x6000, d_loop_of=0x7000, d_centroid=0x8000, L=2, Bp=6, d_scratch=0x9000, scratch_bytes=1 << 30, nv=1, nt=6,
                d_out_vertices=0xA000, d_out_normals=0xB000, d_out_colors=0xC000, d_out_triangles=0xD000, d_new_vertices=0xE001,
                d_new_triangles=0xF001)


def _refuse(call, args, bad, empty, scratch_bytes):
    for field, value in bad:
        a = args()
        a[field] = value
        assert call(a) == EINVAL, (field, value)
    for fields in empty:                                    # nothing to do: NFL_OK without a launch
        a = args()
        a.update(fields)
        assert call(a) == 0, fields
    a = args()                                              # a scratch one byte short, then a misaligned and a missing one
    a["scratch_bytes"] = scratch_bytes - 1
    assert call(a) == ESMALL
    a["scratch_bytes"] = 0
    assert call(a) == ESMALL
    a = args()
    a["d_scratch"] += 4
    assert call(a) == EINVAL
    a["d_scratch"] = None
    assert call(a) == EINVAL


SIZES = (("V", -1), ("T", -1), ("V", 1 << 31), ("T", BIG_T))


def test_edges_count_and_emit_refuse_before_any_launch(L):
    need = L.nfl_mesh_edges_bytes(30, 10)
    assert need > 0 and need % 16 == 0 and L.nfl_mesh_edges_bytes(-1, 1) == 0 == L.nfl_mesh_edges_bytes(1, BIG_T)
    assert L.nfl_mesh_edges_bytes(0, 0) == 16                                 # the two raw totals alone
    bad = SIZES + (("N", -1), ("N", 61), ("d_triangles", None), ("d_triangles", 0x1002), ("d_offsets", None), ("d_offsets", 0x2004),
                   ("d_neighbors", None), ("d_neighbors", 0x3002), ("d_totals", None), ("d_totals", 0x5004))
    _refuse(lambda a: L.nfl_mesh_edges_count(*a.values(), None), _edges_count_args, bad, (dict(V=0), dict(T=0, N=0)), need)
    bad = SIZES + (("E", -1), ("E", 31), ("H", -1), ("H", 31), ("d_triangles", None), ("d_triangles", 0x1002), ("d_edges", None),
                   ("d_edges", 0x5002), ("d_half_edge", None), ("d_half_edge", 0x6002), ("d_edge_offsets", None),
                   ("d_edge_offsets", 0x7004), ("d_edge_halves", None), ("d_edge_halves", 0x8002), ("d_kind", None), ("d_twin", None),
                   ("d_twin", 0xA002))
    _refuse(lambda a: L.nfl_mesh_edges_emit(*a.values(), None), _edges_emit_args, bad, (dict(V=0), dict(T=0, E=0, H=0)), need)


def test_loops_count_and_emit_refuse_before_any_launch(L):
    need = L.nfl_mesh_loops_bytes(10)
    assert need > 0 and need % 16 == 0 and L.nfl_mesh_loops_bytes(-1) == 0 == L.nfl_mesh_loops_bytes(BIG_T)
    bad = SIZES + (("E", -1), ("E", 31), ("n_boundary", -1), ("n_boundary", 31), ("d_vertices", None), ("d_vertices", 0x1002),
                   ("d_triangles", None), ("d_triangles", 0x2002), ("d_half_edge", None), ("d_half_edge", 0x3002), ("d_twin", None),
                   ("d_twin", 0x4002), ("d_kind", None), ("d_totals", None), ("d_totals", 0x7004))
    _refuse(lambda a: L.nfl_mesh_loops_count(*a.values(), None), _loops_count_args, bad, (dict(V=0), dict(T=0, E=0, n_boundary=0)), need)
    bad = (("T", -1), ("T", BIG_T), ("L", -1), ("L", 11), ("Bp", -1), ("Bp", 31), ("d_loop_offsets", None), ("d_loop_offsets", 0x1004),
           ("d_loop_halves", None), ("d_loop_halves", 0x2002), ("d_loop_of", None), ("d_loop_of", 0x3002), ("d_length", None),
           ("d_length", 0x4002), ("d_perimeter", None), ("d_perimeter", 0x5002), ("d_centroid", None), ("d_centroid", 0x7002))
    _refuse(lambda a: L.nfl_mesh_loops_emit(*a.values(), None), _loops_emit_args, bad, (dict(T=0, L=0, Bp=0),), need)


def test_fill_count_and_emit_refuse_before_any_launch(L):
    need = L.nfl_mesh_fill_bytes(2)
    assert need > 0 and need % 16 == 0 and L.nfl_mesh_fill_bytes(-1) == 0 == L.nfl_mesh_fill_bytes(BIG_T) and L.nfl_mesh_fill_bytes(0) == 0
    bad = (("L", -1), ("L", BIG_T), ("max_edges", 2), ("max_edges", 0), ("max_edges", -1), ("max_perimeter", 0.0), ("max_perimeter", -1.0),
           ("max_perimeter", np.nan), ("d_length", None), ("d_length", 0x1002), ("d_perimeter", None), ("d_perimeter", 0x2002),
           ("d_totals", None), ("d_totals", 0x5004))
    call = lambda a: L.nfl_mesh_fill_count(*a.values(), None)
    _refuse(call, _fill_count_args, bad, (dict(L=0),), need)
    a = _fill_count_args()
    a.update(L=0, d_keep=None, max_perimeter=np.inf, max_edges=2 ** 62)       # no mask, no limits
    assert call(a) == 0
    pointers = [k for k in _fill_emit_args() if k.startswith("d_") and k not in ("d_scratch", "d_new_vertices", "d_new_triangles")]
    bad = SIZES + (("L", -1), ("L", 11), ("Bp", -1), ("Bp", 31), ("nv", -1), ("nv", 3), ("nt", -1), ("nt", 7), ("d_colors", None),
                   ("d_out_colors", None)) + tuple((k, None) for k in pointers if "colors" not in k) + \
        tuple((k, _fill_emit_args()[k] + (4 if k == "d_loop_offsets" else 2)) for k in pointers)
    call = lambda a: L.nfl_mesh_fill_emit(*a.values(), None)
    _refuse(call, _fill_emit_args, bad, (dict(V=0), dict(T=0, L=0, Bp=0, nv=0, nt=0), dict(L=0, Bp=0, nv=0, nt=0)), need)
    a = _fill_emit_args()
    a.update(L=0, Bp=0, nv=0, nt=0, d_colors=None, d_out_colors=None, d_new_vertices=None, d_new_triangles=None)   # all three optional
    assert call(a) == 0


def test_bad_python_arguments_are_refused_before_any_tensor_is_looked_at():
    from nerf_fl_amd import topology
    for bad in (2, 0, -1, 3.0, True, "3"):
        with pytest.raises(ValueError, match="max_edges"):
            topology.fill_holes(None, max_edges=bad)
    for bad in (0.0, -1.0, np.nan, 1e-60):
        with pytest.raises(ValueError, match="max_perimeter"):
            topology.fill_holes(None, max_perimeter=bad)
    for call in (lambda: topology.mesh_edges(None), lambda: topology.boundary_loops(None), lambda: topology.mesh_topology(None),
                 lambda: topology.fill_holes(None), lambda: topology.mesh_edges({"vertices": 0}),
                 lambda: topology.fill_holes(None, max_edges=3, max_perimeter=1.0, keep=0, loops=0, edges=0)):
        with pytest.raises(ValueError):
            call()


# ---- the restatement: hand cases, every table written out -----------------------------------------------------------------------

def _tables(mesh):
    V = len(mesh["vertices"])
    ed = eref.edges(mesh["triangles"], V)
    return ed, eref.loops(mesh["vertices"], mesh["triangles"], ed)


def _is(ed, lp, **want):
    for k, v in want.items():
        got = ed[k] if k in ed else lp[k]
        got = got.tolist() if hasattr(got, "tolist") else got
        assert got == v, (k, got, v)


CASES = sref.hand_cases()


def test_one_triangle():
    ed, lp = _tables(CASES["one_triangle"])
    _is(ed, lp, edges=[[0, 1], [0, 2], [1, 2]], half_edge=[0, 2, 1], edge_offsets=[0, 1, 2, 3], edge_halves=[0, 2, 1], kind=[B, B, B],
        twin=[-1, -1, -1], totals=[3, 3, 3, 0, 0, 0, 0], loop_offsets=[0, 3], loop_halves=[0, 1, 2], loop_of=[0, 0, 0], length=[3],
        n_loops=1, n_open=0)
    assert eref.successor(ed).tolist() == [1, 2, 0]
    assert lp["perimeter"].dtype == F and lp["perimeter"][0] == F(2.0 + np.sqrt(2.0)) and lp["centroid"].tolist() == [[F(1 / 3), F(1 / 3), 0.0]]
    out, info = eref.fill(CASES["one_triangle"], lp)
    assert out["triangles"].tolist() == [[0, 1, 2], [1, 0, 2]] and len(out["vertices"]) == 3        # ONE triangle (b, a, c), no vertex
    assert (info["n_filled"], info["n_new_vertices"], info["n_new_triangles"]) == (1, 0, 1) and info["new_triangles"].tolist() == [False, True]
    topo = eref.topology(out)
    assert topo["closed"] and topo["manifold"] and topo["oriented"] and topo["euler"].tolist() == [2] and topo["genus"].tolist() == [0]


def test_a_tetrahedron_is_closed_with_euler_2_and_genus_0():
    ed, lp = _tables(CASES["tetrahedron"])
    _is(ed, lp, edges=[[0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]], half_edge=[0, 3, 1, 2, 4, 0, 1, 5, 2, 4, 5, 3],
        edge_offsets=[0, 2, 4, 6, 8, 10, 12], edge_halves=[0, 5, 2, 6, 3, 8, 1, 11, 4, 9, 7, 10], kind=[I] * 6,
        twin=[5, 11, 6, 8, 9, 0, 2, 10, 3, 4, 7, 1], totals=[6, 12, 0, 0, 0, 0, 0], loop_offsets=[0], loop_halves=[], loop_of=[-1] * 12,
        n_loops=0, n_open=0)
    topo = eref.topology(CASES["tetrahedron"], ed, lp)
    assert topo["closed"] and topo["manifold"] and topo["oriented"]
    assert (topo["vertices"].tolist(), topo["edges"].tolist(), topo["triangles"].tolist()) == ([4], [6], [4])
    assert topo["euler"].tolist() == [2] and topo["genus"].tolist() == [0] and topo["loops"].tolist() == [0]


def test_a_square_of_two_triangles_has_one_loop_of_4_and_its_fan():
    ed, lp = _tables(CASES["square"])
    _is(ed, lp, edges=[[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]], half_edge=[0, 3, 1, 1, 4, 2], edge_offsets=[0, 1, 3, 4, 5, 6],
        edge_halves=[0, 2, 3, 5, 1, 4], kind=[B, I, B, B, B], twin=[-1, -1, 3, 2, -1, -1], totals=[5, 6, 4, 0, 0, 0, 0],
        loop_offsets=[0, 4], loop_halves=[0, 1, 4, 5], loop_of=[0, 0, -1, -1, 0, 0], length=[4], perimeter=[4.0], centroid=[[0.5, 0.5, 0.0]],
        n_loops=1, n_open=0)
    assert eref.successor(ed).tolist() == [1, 4, -2, -2, 5, 0]                # through the twin at vertices 2 and 0
    out, info = eref.fill(CASES["square"], lp)
    assert out["triangles"][2:].tolist() == [[1, 0, 4], [2, 1, 4], [3, 2, 4], [0, 3, 4]]
    assert out["vertices"][4].tolist() == [0.5, 0.5, 0.0] and out["normals"][4].tolist() == [0.0, 0.0, -1.0]   # against the input's +z
    assert out["vertices"][:4].tobytes() == CASES["square"]["vertices"].tobytes() and info["new_vertices"].tolist() == [False] * 4 + [True]
    topo = eref.topology(out)
    assert topo["closed"] and topo["oriented"] and topo["manifold"] and topo["euler"].tolist() == [2]


def test_three_triangles_on_one_edge_are_nonmanifold_and_their_boundary_is_open_chains():
    ed, lp = _tables(CASES["three_on_an_edge"])
    _is(ed, lp, edges=[[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4]], half_edge=[0, 4, 1, 0, 5, 2, 0, 6, 3],
        edge_offsets=[0, 3, 4, 5, 6, 7, 8, 9], edge_halves=[0, 3, 6, 2, 5, 8, 1, 4, 7], kind=[N, B, B, B, B, B, B], twin=[-1] * 9,
        totals=[7, 9, 6, 0, 1, 0, 0], loop_offsets=[0], loop_halves=[], loop_of=[-1] * 9, n_loops=0, n_open=6)
    assert eref.successor(ed).tolist() == [-2, 2, -1, -2, 5, -1, -2, 8, -1]
    out, info = eref.fill(CASES["three_on_an_edge"], lp)
    assert info["n_filled"] == 0 and out["triangles"].tobytes() == CASES["three_on_an_edge"]["triangles"].tobytes()
    topo = eref.topology(CASES["three_on_an_edge"], ed, lp)
    assert not topo["manifold"] and not topo["closed"] and topo["oriented"] and topo["genus"].tolist() == [-1]


def test_the_rotation_does_not_cross_at_the_pinch_of_a_bow_tie():
    ed, lp = _tables(CASES["bow_tie"])
    _is(ed, lp, edges=[[0, 1], [0, 2], [0, 3], [0, 4], [1, 2], [3, 4]], half_edge=[0, 4, 1, 2, 5, 3], kind=[B] * 6, twin=[-1] * 6,
        edge_offsets=[0, 1, 2, 3, 4, 5, 6], edge_halves=[0, 2, 3, 5, 1, 4], totals=[6, 6, 6, 0, 0, 0, 0], loop_offsets=[0, 3, 6],
        loop_halves=[0, 1, 2, 3, 4, 5], loop_of=[0, 0, 0, 1, 1, 1], length=[3, 3], n_loops=2, n_open=0)
    assert lp["centroid"].tolist() == [[F(2 / 3), 0.0, 0.0], [F(-2 / 3), 0.0, 0.0]]
    out, _ = eref.fill(CASES["bow_tie"], lp)
    assert out["triangles"][2:].tolist() == [[1, 0, 2], [3, 0, 4]]


def test_a_tetrahedron_with_one_face_reversed_has_3_flipped_edges():
    mesh = dict(CASES["tetrahedron"], triangles=np.int32([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 2, 3]]))
    ed, lp = _tables(mesh)
    _is(ed, lp, kind=[I, I, I, X, X, X], twin=[5, -1, 6, 8, -1, 0, 2, -1, 3, -1, -1, -1], totals=[6, 12, 0, 3, 0, 0, 0], n_loops=0, n_open=0,
        edge_halves=[0, 5, 2, 6, 3, 8, 1, 9, 4, 11, 7, 10])
    topo = eref.topology(mesh, ed, lp)
    assert topo["closed"] and topo["manifold"] and not topo["oriented"] and topo["genus"].tolist() == [-1]


def test_a_moebius_strip_is_not_oriented_however_it_is_wound():
    """Manifold, with one boundary curve, and not orientable: every winding leaves a FLIPPED edge, `oriented` is false and the
    genus -1.  (Under the definitions the rotation stops at that edge, so the boundary curve shows as open chains there.)"""
    mesh = eref.moebius()
    rng = np.random.default_rng(0)
    for trial in range(20):
        tri = mesh["triangles"].copy()
        if trial:
            flip = rng.random(len(tri)) < 0.5
            tri[flip] = tri[flip][:, [0, 2, 1]]
        m = dict(mesh, triangles=tri)
        ed, lp = _tables(m)
        topo = eref.topology(m, ed, lp)
        assert ed["totals"][3] >= 1 and ed["totals"][4] == 0 and ed["totals"][2] == 16
        assert topo["manifold"] and not topo["oriented"] and not topo["closed"] and topo["genus"].tolist() == [-1]
        assert topo["euler"].tolist() == [0] and lp["n_open"] + int(lp["length"].sum()) == 16


def test_a_degenerate_half_edge_an_isolated_vertex_an_index_out_of_range_and_a_nan_vertex():
    ed, lp = _tables(CASES["repeated_index"])                                # the triangle (0, 0, 1)
    _is(ed, lp, edges=[[0, 1], [0, 2], [1, 2]], half_edge=[-1, 0, 0, 0, 2, 1], edge_offsets=[0, 3, 4, 5], edge_halves=[1, 2, 3, 5, 4],
        kind=[N, B, B], twin=[-1] * 6, totals=[3, 5, 2, 0, 1, 1, 0], n_loops=0, n_open=2)
    ed, lp = _tables(CASES["isolated_vertex"])
    _is(ed, lp, edges=[[0, 1], [0, 2], [0, 3], [1, 2], [2, 3]], loop_halves=[0, 1, 4, 5], totals=[5, 6, 4, 0, 0, 0, 0])
    topo = eref.topology(CASES["isolated_vertex"], ed, lp)
    assert topo["n_components"] == 2 and topo["euler"].tolist() == [1, 1] and topo["genus"].tolist() == [0, -1]
    assert eref.fill(CASES["isolated_vertex"], lp)[0]["triangles"][2:].tolist() == [[1, 0, 5], [2, 1, 5], [3, 2, 5], [0, 3, 5]]
    ed, lp = _tables(CASES["out_of_range"])                                   # two of the four triangles take part in nothing
    _is(ed, lp, half_edge=[0, 3, 1, -1, -1, -1, -1, -1, -1, 1, 4, 2], twin=[-1, -1, 9, -1, -1, -1, -1, -1, -1, 2, -1, -1],
        edge_halves=[0, 2, 9, 11, 1, 10], totals=[5, 6, 4, 0, 0, 0, 2], loop_halves=[0, 1, 10, 11], length=[4])
    ed, lp = _tables(CASES["nan_vertex"])
    _is(ed, lp, kind=[B, I, B, I, B, B, B], loop_halves=[0, 6, 7, 4, 5], length=[5], centroid=[[0.0, 0.0, 0.0]], n_open=0)
    assert np.isposinf(lp["perimeter"]).all() and eref.fill(CASES["nan_vertex"], lp)[1]["n_filled"] == 0      # never filled


def test_a_grid_patch_has_one_rim_loop_and_a_fan_its_hub_and_rim():
    ed, lp = _tables(sref.grid_patch(5))
    assert lp["length"].tolist() == [16] and lp["n_open"] == 0 and ed["totals"][2:5] == [16, 0, 0]
    fan = sref.fan(4096)
    ed, lp = _tables(fan)
    assert sorted(lp["length"].tolist()) == [300, 4096] and lp["n_open"] == 0
    book = eref.book(300)
    ed, lp = _tables(book)
    assert ed["kind"][0] == N and np.diff(ed["edge_offsets"])[0] == 300 and ed["totals"][4] == 1 and lp["n_loops"] == 0


# ---- conditions for exactness ----------------------------------------------------------------------------------------------------

def _shuffled(mesh, rng):
    """The same mesh with its triangles permuted and their corners rotated, and where every old half-edge went."""
    tri = mesh["triangles"]
    T = len(tri)
    perm, rot = rng.permutation(T), rng.integers(0, 3, T)
    new = tri[perm[:, None], (np.arange(3)[None, :] + rot[perm, None]) % 3]
    where = np.empty(T, dtype=np.int64)
    where[perm] = np.arange(T)
    old = np.arange(3 * T)
    moved = 3 * where[old // 3] + (old % 3 - rot[old // 3]) % 3
    return dict(mesh, triangles=np.ascontiguousarray(new, dtype=np.int32)), moved


def _cycles(lp, moved=None):
    rows = []
    for l in range(lp["n_loops"]):
        row = lp["loop_halves"][lp["loop_offsets"][l]:lp["loop_offsets"][l + 1]].astype(np.int64)
        row = row if moved is None else moved[row]
        k = int(row.argmin())
        rows.append(np.roll(row, -k).tolist())
    return sorted(rows)


@pytest.mark.parametrize("name", ["grid", "soup", "punched"])
def test_the_tables_do_not_depend_on_the_order_of_the_triangles(name, punched):
    """20 seeded permutations.  edges and kind are identical; half_edge, twin and the loops are identical after mapping the
    half-edge ids.  The start of a loop moves with the ids, so the fp64 folds run in a rotated order.  THE BOUND, from the fold and
    not from a measurement: a sequential fp64 sum of n terms is within (n - 1) 2^-53 sum|x| of the exact sum, so two orders are
    within 2 (n - 1) 2^-53 sum|x| of each other, and the one rounding to fp32 adds at most half an ulp of fp32 to each: the two
    fp32 results differ by at most one fp32 ulp of the larger plus that fp64 term (for the centroid, per component, over n)."""
    mesh = {"grid": sref.grid_patch(5), "soup": sref.soup(65, 200, 3), "punched": punched[0]}[name]
    V = len(mesh["vertices"])
    ed, lp = _tables(mesh)
    rng = np.random.default_rng(11)
    v64 = np.nan_to_num(np.abs(mesh["vertices"].astype(np.float64)), nan=0.0, posinf=0.0, neginf=0.0)
    for _ in range(20):
        m2, moved = _shuffled(mesh, rng)
        ed2, lp2 = _tables(m2)
        assert np.array_equal(ed2["edges"], ed["edges"]) and np.array_equal(ed2["kind"], ed["kind"]) and ed2["totals"] == ed["totals"]
        assert np.array_equal(ed2["half_edge"][moved], ed["half_edge"])
        assert np.array_equal(ed2["twin"][moved], np.where(ed["twin"] >= 0, moved[np.maximum(ed["twin"], 0)], -1))
        assert _cycles(lp2) == _cycles(lp, moved) and lp2["n_open"] == lp["n_open"]
        first = lambda p, mv: {int((p["loop_halves"][p["loop_offsets"][l]:p["loop_offsets"][l + 1]] if mv is None else
                                    mv[p["loop_halves"][p["loop_offsets"][l]:p["loop_offsets"][l + 1]].astype(np.int64)]).min()): l
                               for l in range(p["n_loops"])}
        a, b = first(lp, moved), first(lp2, None)
        for key, l in a.items():
            l2 = b[key]
            n = int(lp["length"][l])
            p, p2 = float(lp["perimeter"][l]), float(lp2["perimeter"][l2])
            if np.isinf(p):
                assert np.isinf(p2)
                continue
            slack = 2.0 * (n - 1) * 2.0 ** -53
            assert abs(p - p2) <= 2.0 ** -23 * max(abs(p), abs(p2)) + slack * 2.0 * max(p, p2)
            row = lp["loop_halves"][lp["loop_offsets"][l]:lp["loop_offsets"][l + 1]].astype(np.int64)
            total = v64[mesh["triangles"].reshape(-1)[row]].sum(axis=0)
            c, c2 = lp["centroid"][l].astype(np.float64), lp2["centroid"][l2].astype(np.float64)
            assert (np.abs(c - c2) <= 2.0 ** -23 * np.maximum(np.abs(c), np.abs(c2)) + slack * total / n + 2.0 ** -149).all()


@pytest.mark.parametrize("shape,euler,genus", [("ball", 2, 0), ("torus", 0, 1)])
def test_a_ball_and_a_torus_off_the_lattice_are_closed_manifold_and_oriented(shape, euler, genus):
    mesh = eref.lattice_mesh(17, shape)
    topo = eref.topology(mesh)
    assert len(mesh["triangles"]) > 2000 and topo["n_components"] == 1
    assert topo["closed"] and topo["manifold"] and topo["oriented"] and topo["n_loops"] == 0 == topo["n_open"]
    assert topo["euler"].tolist() == [euler] and topo["genus"].tolist() == [genus]


# ---- fill on the 17^3 ball -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def punched():
    ball = eref.lattice_mesh(17, "ball")
    ball["colors"] = np.random.default_rng(2).uniform(0, 1, ball["vertices"].shape).astype(F)
    for seed in range(50):                                  # the first seed whose five valences are not all the same
        mesh, chosen, valence = eref.punch(ball, 5, seed)
        if len(chosen) == 5 and min(valence) < max(valence):
            return mesh, chosen, valence, ball
    raise AssertionError("no seed gives five one-rings of differing valence")


def test_five_one_rings_removed_leave_five_loops_of_their_valences(punched):
    mesh, chosen, valence, ball = punched
    ed, lp = _tables(mesh)
    assert len(mesh["triangles"]) == len(ball["triangles"]) - sum(valence)
    assert lp["n_loops"] == 5 and lp["n_open"] == 0 and sorted(lp["length"].tolist()) == sorted(valence)
    topo = eref.topology(mesh, ed, lp)
    assert not topo["closed"] and topo["manifold"] and topo["oriented"] and topo["loops"][0] == 5
    assert topo["euler"][0] == 2 - 5 and topo["genus"][0] == 0               # a sphere with five discs removed


def test_filling_closes_the_ball_again_and_keeps_every_input_row(punched):
    mesh, chosen, valence, ball = punched
    ed, lp = _tables(mesh)
    out, info = eref.fill(mesh, lp)
    V, T = len(mesh["vertices"]), len(mesh["triangles"])
    assert (info["n_filled"], info["n_new_vertices"], info["n_new_triangles"]) == (5, 5, sum(valence))
    for k in ("vertices", "normals", "colors", "triangles"):
        assert out[k][:len(mesh[k])].tobytes() == mesh[k].tobytes() and out[k].dtype == mesh[k].dtype, k
    assert info["new_vertices"].tolist() == [False] * V + [True] * 5 and info["new_triangles"].sum() == sum(valence)
    topo = eref.topology(out)
    assert topo["closed"] and topo["manifold"] and topo["oriented"] and topo["euler"][0] == 2 and topo["genus"][0] == 0
    at, start = T, mesh["triangles"].reshape(-1)
    for l in range(5):                                      # the stated order: loop order, then walk order
        row = lp["loop_halves"][lp["loop_offsets"][l]:lp["loop_offsets"][l + 1]].astype(np.int64)
        assert out["vertices"][V + l].tobytes() == lp["centroid"][l].tobytes()
        for h in row:
            assert out["triangles"][at].tolist() == [start[h - h % 3 + (h % 3 + 1) % 3], start[h], V + l]
            at += 1
        mean = mesh["colors"][start[row]].astype(np.float64).mean(axis=0)
        assert np.abs(out["colors"][V + l] - mean).max() < 1e-6
        outward = out["vertices"][V + l].astype(np.float64)
        assert np.dot(out["normals"][V + l], outward / np.linalg.norm(outward)) > 0.9      # the cap of a ball wound outward faces outward
    assert at == len(out["triangles"])


def test_max_edges_leaves_exactly_the_larger_loops_open_and_a_mask_the_others(punched):
    mesh, chosen, valence, ball = punched
    ed, lp = _tables(mesh)
    limit = max(valence) - 1
    out, info = eref.fill(mesh, lp, max_edges=limit)
    assert 0 < info["n_filled"] == sum(v <= limit for v in valence) < 5
    _, lp2 = _tables(out)
    assert sorted(lp2["length"].tolist()) == sorted(v for v in valence if v > limit)
    keep = np.array([True, False, True, False, False])
    out, info = eref.fill(mesh, lp, keep=keep)
    _, lp3 = _tables(out)
    assert info["n_filled"] == 2 and sorted(lp3["length"].tolist()) == sorted(lp["length"][~keep].tolist())
    out, info = eref.fill(mesh, lp, max_perimeter=float(np.sort(lp["perimeter"])[1]))
    assert info["n_filled"] == 2
    assert eref.fill(mesh, lp, max_perimeter=1e-3)[1]["n_filled"] == 0


def test_a_loop_of_3_gets_one_triangle_and_no_vertex():
    ball = eref.lattice_mesh(17, "ball")
    mesh = dict(ball, triangles=np.delete(ball["triangles"], 100, axis=0))
    ed, lp = _tables(mesh)
    assert lp["length"].tolist() == [3]
    out, info = eref.fill(mesh, lp)
    assert (info["n_new_vertices"], info["n_new_triangles"]) == (0, 1) and len(out["vertices"]) == len(ball["vertices"])
    assert sorted(out["triangles"][-1].tolist()) == sorted(ball["triangles"][100].tolist())
    assert eref.topology(out)["closed"] and eref.topology(out)["oriented"]
