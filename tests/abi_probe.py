"""What include/nerf_fl_amd.h says, for the tests that hold nerf_fl_amd/_lib.py (and the numpy restatements) to it:

  declared()  the header's text: its structs with their fields in order, and its function prototypes;
  probe()     the header compiled: sizeof every struct of _lib.STRUCTS, offset / size / kind of every field, and the value
              of every constant of _lib.CONSTANTS -- one C file, compiled once per process;
  L           the fixture of the CPU test modules that call the built library (`from abi_probe import L`)."""
import functools
import os
import re
import subprocess
import tempfile

import pytest

from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "nerf_fl_amd.h")


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return _lib.lib()


def _fields(body):
    """`const float* a[3], b;` -> (name, type, is_array) per declarator, in order."""
    out = []
    for statement in filter(None, (s.strip() for s in body.split(";"))):
        first, *rest = (d.strip() for d in statement.split(","))
        ctype, name, dim = re.fullmatch(r"(.*?)(\w+)\s*(\[[^\]]*\])?", first, flags=re.S).groups()
        ctype = re.sub(r"\s+", " ", ctype).replace(" *", "*").strip()
        out.append((name, ctype, dim is not None))
        for d in rest:
            name, dim = re.fullmatch(r"(\w+)\s*(\[[^\]]*\])?", d).groups()
            out.append((name, ctype, dim is not None))
    return out


@functools.lru_cache(maxsize=None)
def declared():
    """{"structs": {name: [(field, type, is_array), ...]}, "functions": {name: (return type, [parameter type, ...])}}"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    structs = {m.group(1): _fields(m.group(2))
               for m in re.finditer(r"typedef\s+struct\s+(nfl_\w+)\s*\{(.*?)\}\s*\1\s*;", text, flags=re.S)}
    functions = {}
    for ret, name, params in re.findall(r"^\s*(int|size_t|const char\*)\s+(nfl_\w+)\s*\(([^)]*)\)\s*;", text, flags=re.M):
        params = [re.sub(r"\s+", " ", p).strip() for p in params.split(",")]
        types = [] if params == ["void"] else [re.fullmatch(r"(.*?)\s*\w+", p).group(1).replace(" *", "*") for p in params]
        functions[name] = (ret, types)
    return {"structs": structs, "functions": functions}


# the one type of a scalar (of an array's element); every pointer, and whatever else, is the default
KIND = ('_Generic((x), float: "float", double: "double", int32_t: "int32_t", uint32_t: "uint32_t", int64_t: "int64_t", '
        'uint64_t: "uint64_t", default: "pointer")')


@functools.lru_cache(maxsize=None)
def probe():
    """{"structs": {name: {"size": n, "fields": {field: (offset, size, kind, count)}}}, "constants": {name: value}}: count is
    None for a scalar and the number of elements for an array, whose kind is its element's.  Only what both sides name is
    probed (a struct or a field that ctypes has and the header lacks would not compile); test_abi_cpu.py compares the names."""
    header = declared()["structs"]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "nerf_fl_amd.h"', f"#define KIND(x) {KIND}",
             "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        if name not in header:
            continue
        lines.append(f'  printf("S {name} %zu\\n", sizeof({name}));')
        arrays = {f: is_array for f, _, is_array in header[name]}
        for f, _ in cls._fields_:
            if f not in arrays:
                continue
            m = f"(({name}*)0)->{f}"
            elem, count = (f"{m}[0]", f"sizeof({m}) / sizeof({m}[0])") if arrays[f] else (m, "(size_t)0")
            lines.append(f'  printf("F {name} {f} %zu %zu %s %zu\\n", offsetof({name}, {f}), sizeof({m}), KIND({elem}), {count});')
    for name in _lib.CONSTANTS:
        lines.append(f'  printf("C {name} %.17g\\n", (double)({name}));')
    lines += ["  return 0;", "}", ""]
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "abi_probe.c"), os.path.join(tmp, "abi_probe")
        open(src, "w").write("\n".join(lines))
        subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), src, "-o", exe], check=True)
        out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    structs, constants = {}, {}
    for tag, name, *rest in (line.split() for line in out.splitlines()):
        if tag == "S":
            structs[name] = {"size": int(rest[0]), "fields": {}}
        elif tag == "F":
            field, offset, size, kind, count = rest
            structs[name]["fields"][field] = (int(offset), int(size), kind, int(count) or None)
        else:
            constants[name] = float(rest[0])
    return {"structs": structs, "constants": constants}

