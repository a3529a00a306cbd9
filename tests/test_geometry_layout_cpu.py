"""The layout of nerf_fl_amd/geometry/ (DESIGN.md section 31), held by a search of its sources: the package is cut by
stage, and the launch line, the counting half of a sized call and the out-of-range refusal each exist once, in _call.py.
The two host-side helpers of _call.py are run on the cases their callers' refusal tests use."""
import ast
import inspect
import os
import re

import numpy as np
import pytest
import torch

import meshcolor_ref as mref
from nerf_fl_amd import geometry
from nerf_fl_amd.geometry import _call, lattice, mesh as mesh_stage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "nerf_fl_amd", "geometry")
NAMES = ["density_lattice", "extract_surface", "surface_colors", "write_ply", "extract_mesh", "lattice_points",
         "mesh_components", "filter_mesh", "clean_mesh", "simplify_mesh", "mesh_adjacency", "smooth_mesh",
         "vertex_normals", "OccupancyGrid", "occupancy_grid", "clip_rays",
         "mesh_depth", "color_mesh_from_images", "mesh_visibility", "render_mesh", "atlas_layout", "atlas_uv",
         "bake_texture", "write_obj"]
SOURCES = {n: open(os.path.join(PKG, n)).read() for n in sorted(os.listdir(PKG)) if n.endswith(".py")}


def _where(text):
    return [n for n, s in SOURCES.items() if text in s]


def test_the_public_names_are_the_same_24():
    assert geometry.__all__ == NAMES and len(NAMES) == 24
    for name in NAMES:
        assert callable(getattr(geometry, name)) or inspect.isclass(getattr(geometry, name)), name
    assert "extract_surface" in geometry.__doc__ and "Conventions:" in geometry.__doc__
    assert sorted(SOURCES) == ["__init__.py", "_call.py", "files.py", "images.py", "lattice.py", "mesh.py", "occupancy.py"]


def test_every_public_name_is_defined_in_one_module():
    defined = {}
    for n, s in SOURCES.items():
        for node in ast.parse(s).body:
            if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
                defined.setdefault(node.name, []).append(n)
    assert {k: v for k, v in defined.items() if len(v) != 1} == {}             # private helpers included
    assert all(name in defined for name in NAMES)
    assert defined["extract_mesh"] == ["__init__.py"] and defined["write_obj"] == ["files.py"]
    assert defined["_run_depth"] == defined["_run_visibility"] == defined["_atlas_of"] == ["images.py"]
    assert defined["_box"] == ["lattice.py"]
    # __init__ re-exports the public names; of the private ones it holds only the three checkers extract_mesh itself calls
    private = sorted(n for n in vars(geometry) if n.startswith("_") and not n.startswith("__") and inspect.isfunction(getattr(geometry, n)))
    assert private == ["_box", "_simplify_arguments", "_smooth_arguments"]


def test_one_launch_line_one_host_read_one_refusal():
    # nfl_render_pass goes through the launch helper too (it takes the plan pointers ahead of the struct): no exception
    assert _where("_lib.check(") == ["_call.py"] and _where("C.byref(") == ["_call.py"]
    # the launch line in its two forms, side by side: _launch for a struct, _call for plain arguments
    assert SOURCES["_call.py"].count("_lib.check(") == 2 and SOURCES["_call.py"].count("C.byref(") == 1
    assert SOURCES["_call.py"].count("rendering._stream()") == 2
    assert _where("rendering._stream()") == ["_call.py"]
    # .tolist(): the totals of a sized call, once.  files.py is the one other place that spells it, on numpy arrays it has
    # already brought to the host (the OBJ writer's numbers); nothing in its source names the library or a launch, and torch
    # only where read_ply, handed a device, uploads what it read
    assert _where(".tolist()") == ["_call.py", "files.py"] and SOURCES["_call.py"].count(".tolist()") == 1
    assert not re.search(r"_lib|rendering|_launch|_count", SOURCES["files.py"])
    reader = SOURCES["files.py"].split("def read_ply(")[1].split("\ndef ")[0]
    assert SOURCES["files.py"].count("torch") == 2 == reader.count("torch") and "    import torch" in reader
    assert not re.search(r"^(import|from) .*torch", SOURCES["files.py"], flags=re.M)
    assert _where("triangles have an index outside") == ["_call.py"]
    assert SOURCES["_call.py"].count("triangles have an index outside") == 1
    for struct in ("MeshDepthArgs", "MeshVisibilityArgs", "MeshShadeArgs", "MeshShadeAtlasArgs"):
        assert _where(struct + "()") == ["images.py"]
    assert _where("a.d_table, a.n_images, a.first, a.count") == ["_call.py"]    # the camera-run prefix, filled once


def test_three_numbers():
    assert _call._three((1, 2.5, "3"), "m") == [1.0, 2.5, 3.0] and _call._three(np.arange(3), "m", int) == [0, 1, 2]
    assert _call._three(torch.tensor([1.0, 2.0, 3.0]), "m") == [1.0, 2.0, 3.0]
    # the origins test_simplify_mesh_refuses_before_a_launch refuses, those that are not 3 numbers at all
    for bad in ((0, 0), (0, 0, 0, 0), 1.0, ("a", "b", "c"), None):
        with pytest.raises(ValueError, match="^origin: 3 finite numbers"):
            _call._three(bad, "origin: 3 finite numbers, in (x, y, z) order")
    # ... and the caller's own rule stays with the caller: a NaN is three numbers
    assert _call._three((0, float("nan"), 0), "m")[0] == 0.0
    for bad in ((0, float("nan"), 0), (0, 0, float("inf"))):
        with pytest.raises(ValueError, match="origin"):
            mesh_stage._simplify_arguments(0.5, bad, "mean")
    # a string float() refuses gets the argument's own text, everywhere (some callers let float's text through before)
    for call in (lambda: lattice._box(("a", 0, 0), (1, 1, 1), (4, 4, 4)), lambda: lattice._box((0, 0, 0), (1, 1, 1), (4, "b", 4))):
        with pytest.raises(ValueError, match="^lo, hi and res are 3 numbers each"):
            call()
    with pytest.raises(ValueError, match="^background: 3 numbers$"):
        _call._three(("white", 1, 1), "background: 3 numbers")
    # the boxes test_geometry_rejects_host_inputs refuses and accepts
    for lo, hi, res in (((0, 0, 0), (1, 1, 1), (4, 1, 4)), ((0, 0, 0), (1, 0, 1), (4, 4, 4)), ((0, 0), (1, 1, 1), (4, 4, 4)),
                        (0, (1, 1, 1), (4, 4, 4))):
        with pytest.raises(ValueError):
            lattice._box(lo, hi, res)
    assert lattice._box((-1, 0, 1), (1, 3, 2), (5, 4, 3)) == ([-1.0, 0.0, 1.0], [0.5, 1.0, 0.5], [5, 4, 3])


def test_host_mesh():
    ver, tri = mref.soup(4, 3)
    mesh = {"vertices": ver, "normals": ver, "triangles": tri}
    for m in (mesh, {k: torch.from_numpy(v) for k, v in mesh.items()}, dict(mesh, vertices=ver.tolist())):
        got = _call._host_mesh(m)
        assert all(isinstance(g, np.ndarray) for g in got)
        assert np.array_equal(got[0], ver) and np.array_equal(got[1], ver) and np.array_equal(got[2], tri)
    empty = _call._host_mesh({"vertices": np.zeros((0, 3)), "normals": np.zeros((0, 3)), "triangles": np.zeros((0, 3), np.int32)})
    assert [g.shape for g in empty] == [(0, 3)] * 3
    # what test_write_obj_refusals refuses of a mesh
    bad_tri = tri.copy()
    bad_tri[2, 1] = 12
    for bad in (dict(mesh, triangles=bad_tri), dict(mesh, triangles=-tri), dict(mesh, normals=ver[:5]),
                dict(mesh, vertices=ver[:, :2]), dict(mesh, triangles=tri.reshape(-1))):
        with pytest.raises(ValueError, match="^mesh: "):
            _call._host_mesh(bad)
