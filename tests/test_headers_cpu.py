"""The layering of the device headers (file map): nfl_math.h is a leaf, nfl_mlp.h the MLP engine on top of it,
nfl_render_impl.h the forward kernel on top of that.  Every header compiles from a one-line includer, and no translation
unit reaches above the layer it needs.  The geometry layer stands beside them: nfl_geom_layout.h (plain C++) under
nfl_geom.h, which its five translation units include and which takes nothing from the render path.  nfl_launch.h (plain C++,
the launchers' host side) sits under the render kernel and the dgrad unit, nfl_compose.h (plain C++, the composition's task
lists) under the weight-gradient launcher and the compose unit; the two runtime queries a launcher makes are written once,
in nfl_dev.h."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nerf_fl_amd", "csrc")
HIPCC = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def includes(name):
    with open(os.path.join(CSRC, name)) as f:
        return set(re.findall(r'^\s*#\s*include\s*"([^"]+)"', f.read(), re.M))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")
@pytest.mark.parametrize("header", ["nfl_math.h", "nfl_dev.h", "nfl_pixel.h", "nfl_mlp.h", "nfl_render_impl.h",
                                    "nfl_geom_layout.h", "nfl_geom.h", "nfl_reduce.h", "nfl_launch.h", "nfl_compose.h"])
def test_header_compiles_on_its_own(header, tmp_path):
    src = tmp_path / "includer.hip"
    src.write_text('#include "%s"\n' % header)
    r = subprocess.run([HIPCC, "-fsyntax-only", "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-I", CSRC, str(src)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_math_header_is_a_leaf():
    assert not includes("nfl_math.h") & {"nfl_plan.h", "nfl_prods.h", "nfl_diag.h", "nfl_mlp.h", "nfl_render_impl.h"}
    assert not includes("nfl_macros.h")          # what nfl_math.h does include pulls in nothing of the project either


@pytest.mark.parametrize("unit", ["nfl_posenc.hip", "nfl_genrays.hip", "nfl_gather.hip"])
def test_small_kernels_take_the_math_only(unit):
    assert "nfl_math.h" in includes(unit)
    assert not includes(unit) & {"nfl_mlp.h", "nfl_render_impl.h"}


def test_dgrad_takes_the_engine_without_the_render_kernel():
    assert "nfl_mlp.h" in includes("nfl_dgrad.hip")
    assert "nfl_render_impl.h" not in includes("nfl_dgrad.hip")


GEOMETRY_UNITS = ["nfl_surface.hip", "nfl_mesh.hip", "nfl_occupancy.hip", "nfl_simplify.hip", "nfl_mesh_scan.hip"]


@pytest.mark.parametrize("unit", GEOMETRY_UNITS)
def test_geometry_units_take_the_shared_header_only(unit):
    assert "nfl_geom.h" in includes(unit)
    assert not includes(unit) & {"nfl_mlp.h", "nfl_render_impl.h", "nfl_math.h", "nfl_plan.h"}


def test_geometry_headers_stand_beside_the_render_path():
    assert includes("nfl_geom.h") == {"nfl_geom_layout.h"}
    assert includes("nfl_geom_layout.h") == {"../../include/nerf_fl_amd.h"}
    with open(os.path.join(CSRC, "nfl_geom_layout.h")) as f:
        assert "hip" not in re.sub(r"//.*", "", f.read())                   # host arithmetic: g++ builds it


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_layout_header_is_plain_cpp(tmp_path):
    src = tmp_path / "includer.cpp"
    src.write_text('#include "nfl_geom_layout.h"\nint main() { return (int)ng_bytes(nm_label_layout(0)); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_launch_header_sits_under_the_kernels():
    assert includes("nfl_launch.h") == {"../../include/nerf_fl_amd.h", "nfl_plan.h"}
    assert includes("nfl_launch.cpp") == {"nfl_launch.h"}
    for user in ("nfl_render_impl.h", "nfl_dgrad.hip", "nfl_capi.hip", "nfl_appearance.hip"):
        assert "nfl_launch.h" in includes(user)
    for name in ("nfl_launch.h", "nfl_launch.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip" not in re.sub(r"//.*", "", f.read())                   # host arithmetic: g++ builds it


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_launch_header_is_plain_cpp(tmp_path):
    src = tmp_path / "includer.cpp"
    src.write_text('#include "nfl_launch.h"\nint main() { return (int)sizeof(RenderArgs) + (int)sizeof(DgradArgs); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_compose_header_sits_under_the_two_units_that_launch_it():
    """nfl_compose.h (plain C++: the composition's task records and their builders) takes the public header and the
    weight-gradient plan only; the unit with the kernel and the weight-gradient launcher include it."""
    assert includes("nfl_compose.h") == {"../../include/nerf_fl_amd.h", "nfl_wgrad_plan.h"}
    assert includes("nfl_wgrad_plan.h") == {"../../include/nerf_fl_amd.h", "nfl_plan.h"}
    assert includes("nfl_compose.cpp") == {"nfl_compose.h"}
    for user in ("nfl_wgrad.hip", "nfl_compose.hip"):
        assert "nfl_compose.h" in includes(user)
    for name in ("nfl_compose.h", "nfl_compose.cpp"):
        with open(os.path.join(CSRC, name)) as f:
            assert "hip" not in re.sub(r"//.*", "", f.read())                   # host arithmetic: g++ builds it


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_compose_header_is_plain_cpp(tmp_path):
    src = tmp_path / "includer.cpp"
    src.write_text('#include "nfl_compose.h"\nint main() { return (int)sizeof(WgCompose) + (int)sizeof(WgTensors); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", CSRC, str(src)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]


def test_runtime_queries_are_written_once():
    """The CU count and the dynamic-LDS attribute go through nfl_device() / nfl_lds_attr() of nfl_dev.h: no other source
    names the runtime calls."""
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h", ".cpp")):
            continue
        with open(os.path.join(CSRC, name)) as f:
            text = f.read()
        for call in ("hipDeviceGetAttribute", "hipFuncSetAttribute"):
            assert text.count(call) == (1 if name == "nfl_dev.h" else 0), (name, call)
