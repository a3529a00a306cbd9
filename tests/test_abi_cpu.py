"""The whole ctypes mirror (nerf_fl_amd/_lib.py: STRUCTS, SYMBOLS, CONSTANTS) against include/nerf_fl_amd.h, in one place:
the two sides name the same structs and functions; every struct has the header's fields in the header's order, each at the
compiled offset, with the compiled size and type; every argtypes list follows its prototype; every constant has the compiled
value.  A new struct or entry point is checked here as soon as it is in the header and in _lib's tables: no new test code.
The header is compiled once (tests/abi_probe.py).  No kernel is launched."""
import ctypes as C

import pytest

from abi_probe import HEADER, L, declared, probe  # noqa: F401  (L is a fixture)
from nerf_fl_amd import _lib

# A deliberate change of the ABI shows up as a diff of this table.
SIZES = {
    "nfl_field_desc": 32, "nfl_field_params": 304, "nfl_pack_job": 48, "nfl_camera": 88, "nfl_pass_args": 328,
    "nfl_compbwd_args": 144, "nfl_dgrad_args": 120, "nfl_field_grads": 304, "nfl_adam_tensors": 2304,
    "nfl_optim_tensors": 2816, "nfl_loss_args": 128, "nfl_pose_args": 112, "nfl_appfit_args": 152, "nfl_image_rec": 104,
    "nfl_gather_args": 80, "nfl_metrics_args": 128, "nfl_depth_args": 64, "nfl_bounds_args": 56, "nfl_surface_args": 112,
    "nfl_mesh_label_args": 56, "nfl_mesh_stats_args": 72, "nfl_mesh_compact_args": 144, "nfl_mesh_simplify_args": 168,
    "nfl_mesh_adjacency_args": 104, "nfl_mesh_smooth_args": 96, "nfl_mesh_normals_args": 80, "nfl_occ_build_args": 56,
    "nfl_occ_clip_args": 80, "nfl_mesh_depth_args": 72, "nfl_mesh_blend_args": 120, "nfl_mesh_visibility_args": 72,
    "nfl_mesh_shade_args": 128, "nfl_atlas_points_args": 88, "nfl_atlas_resolve_args": 128,
    "nfl_mesh_shade_atlas_args": 152, "nfl_tsdf_fuse_args": 112, "nfl_tsdf_resolve_args": 56, "nfl_tsdf_support_args": 72,
    "nfl_trigrid_args": 112, "nfl_mesh_closest_args": 152, "nfl_mesh_sample_args": 104, "nfl_meshdist_reduce_args": 88,
}

# ctypes keeps one class per C type (c_int32 is c_int, c_size_t is c_uint64 here), so `is` compares types, not spellings
SCALARS = {"int": C.c_int, "float": C.c_float, "double": C.c_double, "int32_t": C.c_int32, "uint32_t": C.c_uint32,
           "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t}
KINDS = {C.c_float: "float", C.c_double: "double", C.c_int32: "int32_t", C.c_uint32: "uint32_t", C.c_int64: "int64_t",
         C.c_uint64: "uint64_t", C.c_size_t: "uint64_t", C.c_void_p: "pointer"}


def _kind(ctype):
    """(kind, count) of a ctypes field type, in the probe's terms."""
    if issubclass(ctype, C.Array):
        return _kind(ctype._type_)[0], ctype._length_
    return ("pointer" if issubclass(ctype, C._Pointer) else KINDS[ctype]), None


def test_both_sides_name_the_same_structs():
    ours, theirs = set(_lib.STRUCTS), set(declared()["structs"])
    assert ours == theirs, f"only in _lib.STRUCTS: {sorted(ours - theirs)}; only in the header: {sorted(theirs - ours)}"
    assert set(SIZES) == theirs, f"SIZES and the header differ in {sorted(set(SIZES) ^ theirs)}"
    classes = {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure)}
    assert classes == set(_lib.STRUCTS.values()), "a ctypes.Structure of _lib is missing from STRUCTS, or listed twice"


@pytest.mark.parametrize("name", sorted(set(_lib.STRUCTS) | set(declared()["structs"])))
def test_layout(name):
    assert name in _lib.STRUCTS, f"{name} is in the header and not in _lib.STRUCTS"
    assert name in declared()["structs"], f"{name} is in _lib.STRUCTS and not in the header"
    cls, compiled = _lib.STRUCTS[name], probe()["structs"][name]
    ours, theirs = [f for f, _ in cls._fields_], [f for f, _, _ in declared()["structs"][name]]
    assert ours == theirs, (f"{name}: fields only in ctypes {[f for f in ours if f not in theirs]}, only in the header "
                            f"{[f for f in theirs if f not in ours]}; ctypes order {ours}, header order {theirs}")
    for field, ctype in cls._fields_:
        got = (getattr(cls, field).offset, getattr(cls, field).size) + _kind(ctype)
        want = compiled["fields"][field]
        assert got == want, f"{name}.{field}: ctypes (offset, size, kind, count) {got}, header {want}"
    assert C.sizeof(cls) == compiled["size"] == SIZES[name], name


def test_both_sides_name_the_same_functions(L):
    ours, theirs = [s[0] for s in _lib.SYMBOLS], set(declared()["functions"])
    assert len(ours) == len(set(ours)), "a name is listed twice in _lib.SYMBOLS"
    assert set(ours) == theirs, (f"only in _lib.SYMBOLS: {sorted(set(ours) - theirs)}; "
                                 f"only in the header: {sorted(theirs - set(ours))}")
    for name in ours:
        getattr(L, name)                       # exported by the built library


def _agrees(ctype, param):
    """One argtypes entry against one parameter type of the prototype."""
    if param in SCALARS:
        return ctype is SCALARS[param]
    assert param.endswith("*"), param
    pointee = param[:-1].replace("const ", "")
    if pointee in _lib.STRUCTS:                # the library reads its argument structs and never writes them
        return param.startswith("const ") and ctype is C.POINTER(_lib.STRUCTS[pointee])
    if pointee in SCALARS:
        return ctype is C.c_void_p or ctype is C.POINTER(SCALARS[pointee])
    return pointee in ("void", "char") and ctype is C.c_void_p


@pytest.mark.parametrize("name,restype,argtypes", _lib.SYMBOLS, ids=[s[0] for s in _lib.SYMBOLS])
def test_signature(name, restype, argtypes):
    assert name in declared()["functions"], f"{name} is in _lib.SYMBOLS and not in the header"
    ret, params = declared()["functions"][name]
    want = {"int": C.c_int, "size_t": C.c_size_t, "const char*": C.c_char_p}[ret]
    assert restype is want, f"{name}: restype {restype.__name__}, the header returns {ret}"
    assert len(argtypes) == len(params), f"{name}: {len(argtypes)} argtypes, {len(params)} parameters in the header: {params}"
    for k, (ctype, param) in enumerate(zip(argtypes, params)):
        assert _agrees(ctype, param), f"{name}: argument {k} is {ctype.__name__}, the header has {param}"


@pytest.mark.parametrize("name", sorted(_lib.CONSTANTS))
def test_constant(name):
    ours, theirs = _lib.CONSTANTS[name], probe()["constants"][name]
    assert ours == theirs, f"{name}: {ours} in _lib, {theirs} in the header"


def test_the_small_dicts_hold_what_the_header_defines():
    """Every member of a dict is a constant of the header, under the dict's prefix."""
    for prefix, table in (("NFL_SIMPLIFY_", _lib.SIMPLIFY_PLACEMENTS), ("NFL_NORMALS_", _lib.NORMAL_WEIGHTINGS),
                          ("NFL_BLEND_", _lib.BLEND_WEIGHTINGS), ("NFL_SHADE_", _lib.SHADE_MODES)):
        assert {prefix + k.upper(): v for k, v in table.items()}.items() <= _lib.CONSTANTS.items(), prefix


def test_abi_version_is_pinned_in_three_places(L):
    assert _lib.NFL_ABI_VERSION == L.nfl_abi_version() == 10
    assert "#define NFL_ABI_VERSION 10\n" in open(HEADER).read()
