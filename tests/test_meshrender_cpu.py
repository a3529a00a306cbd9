"""CPU-side checks of mesh render (nerf_fl_amd.geometry.mesh_visibility / render_mesh, csrc/nfl_meshrender.hip): the C entry
points refuse bad arguments before any launch (their structs and signatures are held to the header in
tests/test_abi_cpu.py); the numpy restatement (tests/meshrender_ref.py),
which the GPU tests hold the kernels to bit for bit, is itself checked on hand cases whose expected numbers are written out
and, independent of its own fp32 arithmetic, against the same algorithm in fp64 on the seeded triangle soup.  No kernel is
launched."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import meshcolor_ref as mref
import meshrender_ref as rref
from abi_probe import L  # noqa: F401  (a fixture)
from nerf_fl_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
EINVAL = -1
INF = np.inf


# ---- sources and validation ------------------------------------------------------------------------------------------------

def test_shade_modes_and_the_header_s_sections():
    assert _lib.SHADE_MODES == {"color": 0, "normal": 1, "facing": 2}      # held to the header's enum in test_abi_cpu.py
    header = open(os.path.join(ROOT, "include", "nerf_fl_amd.h")).read()
    assert header.index("---- mesh colour") < header.index("---- mesh render") < header.index("---- hierarchical sampling")


def test_the_ray_test_exists_once(tmp_path):
    """nfl_meshray.h compiles from a one-line includer, both rasters include it, and neither defines the ray test itself."""
    import shutil
    csrc = os.path.join(ROOT, "nerf_fl_amd", "csrc")
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    text = {n: open(os.path.join(csrc, n)).read() for n in ("nfl_meshray.h", "nfl_meshcolor.hip", "nfl_meshrender.hip")}
    for fn in ("nmc_dot", "nmc_to_camera", "nmc_setup", "nmc_test", "nmc_ray"):
        defined = [n for n, t in text.items() if re.search(r"NFL_DEV \w+ %s\(" % fn, t)]
        assert defined == ["nfl_meshray.h"], (fn, defined)
    # the finite test of the cull is the geometry layer's, defined there once for float and used by the raster
    text["nfl_geom.h"] = open(os.path.join(csrc, "nfl_geom.h")).read()
    defined = [n for n, t in text.items() if re.search(r"bool ng_is_finite\(float", t)]
    assert defined == ["nfl_geom.h"] and "ng_is_finite(q[k][0])" in text["nfl_meshray.h"], defined
    assert not any(re.search(r"bool \w*finite\w*\(", text[n]) for n in ("nfl_meshray.h", "nfl_meshcolor.hip", "nfl_meshrender.hip"))
    del text["nfl_geom.h"]
    assert [n for n, t in text.items() if "struct NmcTri" in t] == ["nfl_meshray.h"]
    for unit in ("nfl_meshcolor.hip", "nfl_meshrender.hip"):
        assert '#include "nfl_meshray.h"' in text[unit] and '#include "nfl_geom.h"' in text[unit]
    if os.path.exists(hipcc):
        src = tmp_path / "includer.hip"
        src.write_text('#include "nfl_meshray.h"\n')
        r = subprocess.run([hipcc, "-fsyntax-only", "--offload-arch=gfx950", "-std=c++17", "-x", "hip", "-I", csrc, str(src)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]


def _vis_args():
    a = _lib.MeshVisibilityArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 0x2000, 30, 10
    a.d_table, a.n_images, a.first, a.count, a.d_vis, a.n_vis = 0x3000, 4, 1, 2, 0x4000, 100
    return a


def test_visibility_refuses_before_any_launch(L):
    """Every pointer below is a made-up address: a launch would fault, so a refusal can only come from the host check."""
    assert L.nfl_mesh_visibility(None, None) == EINVAL
    for field in ("d_vertices", "d_triangles", "d_table", "d_vis"):
        a = _vis_args()
        setattr(a, field, None)
        assert L.nfl_mesh_visibility(C.byref(a), None) == EINVAL, field
    for field, addr in (("d_vertices", 0x1002), ("d_triangles", 0x2001), ("d_table", 0x3004), ("d_vis", 0x4004), ("d_vis", 0x4001)):
        a = _vis_args()
        setattr(a, field, addr)
        assert L.nfl_mesh_visibility(C.byref(a), None) == EINVAL, (field, addr)
    for field, bad in (("n_vertices", -1), ("n_vertices", 1 << 31), ("n_triangles", -1), ("n_triangles", (1 << 31) // 3 + 1),
                       ("n_images", 0), ("first", -1), ("count", -1), ("first", 3), ("count", 4), ("first", 5),
                       ("n_vis", -1), ("n_vis", (1 << 38) + 1)):
        a = _vis_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_visibility(C.byref(a), None) == EINVAL, (field, bad)
    a = _vis_args()                                                  # 2^31 workgroups of (triangle, image) pairs
    a.n_triangles, a.n_images, a.first, a.count = (1 << 31) // 3, 1 << 20, 0, 1 << 20
    assert L.nfl_mesh_visibility(C.byref(a), None) == EINVAL


def _shade_args(mode=0):
    a = _lib.MeshShadeArgs()
    a.d_vertices, a.d_triangles, a.n_vertices, a.n_triangles = 0x1000, 0x2000, 30, 10
    a.d_table, a.n_images, a.first, a.count, a.mode, a.d_vis, a.n_vis = 0x3000, 4, 1, 2, mode, 0x4000, 100
    a.d_attr, a.d_rgb, a.d_rgb_u8, a.d_depth, a.d_triangle = 0x5000, 0x6000, 0x7001, 0x8000, 0x9000
    return a


def test_shade_refuses_before_any_launch(L):
    assert L.nfl_mesh_shade(None, None) == EINVAL
    for field in ("d_vertices", "d_triangles", "d_table", "d_vis", "d_attr"):
        a = _shade_args()
        setattr(a, field, None)
        assert L.nfl_mesh_shade(C.byref(a), None) == EINVAL, field
    a = _shade_args(1)                                               # normals are attributes too
    a.d_attr = None
    assert L.nfl_mesh_shade(C.byref(a), None) == EINVAL
    for field, addr in (("d_vertices", 0x1002), ("d_triangles", 0x2001), ("d_table", 0x3004), ("d_vis", 0x4004),
                        ("d_attr", 0x5002), ("d_rgb", 0x6001), ("d_depth", 0x8002), ("d_triangle", 0x9003)):
        a = _shade_args()
        setattr(a, field, addr)
        assert L.nfl_mesh_shade(C.byref(a), None) == EINVAL, field
    for field, bad in (("n_vertices", -1), ("n_vertices", 1 << 31), ("n_triangles", -1), ("n_triangles", (1 << 31) // 3 + 1),
                       ("n_images", 0), ("first", -1), ("count", -1), ("first", 3), ("count", 4), ("first", 5),
                       ("mode", 3), ("mode", -1), ("n_vis", -1), ("n_vis", (1 << 38) + 1)):
        a = _shade_args()
        setattr(a, field, bad)
        assert L.nfl_mesh_shade(C.byref(a), None) == EINVAL, (field, bad)
    # nothing to do: NFL_OK without a launch, whatever the pointers
    for mode in (0, 1, 2):
        a = _shade_args(mode)
        a.n_vis = 0
        assert L.nfl_mesh_shade(C.byref(a), None) == 0
    a = _shade_args(2)                                               # the headlight reads no attributes
    a.d_attr, a.n_vis = None, 0
    assert L.nfl_mesh_shade(C.byref(a), None) == 0


# ---- hand cases.  9 x 9 pixels, fx = fy = 8, cx = cy = 4: the ray of pixel (i, j) is ((i - 4) / 8, -(j - 4) / 8, -1), exact in
# fp32, and it meets the plane z = -3 at 3 * that

CAM = dict(width=9, height=9, fx=8.0, fy=8.0, cx=4.0, cy=4.0)
# square-on at distance 3, its corners on the rays of pixels (1, 7), (7, 7) and (4, 1): the centroid lies on pixel (4, 5)
TRI = [[-1.125, -1.125, -3], [1.125, -1.125, -3], [0, 1.125, -3]]
COL = np.array([[0.9, 0.1, 0.2], [0.2, 0.8, 0.1], [0.1, 0.3, 0.7]], dtype=F)
BG = (0.25, 0.5, 0.75)


def _render(ver, tri, attr=None, mode="color", cam=None):
    ver = np.array(ver, dtype=F).reshape(-1, 3)
    out = rref.render(ver, np.array(tri, dtype=np.int32).reshape(-1, 3), mref.camera(**(cam or CAM)), mode, attr, BG)
    H, W = (cam or CAM)["height"], (cam or CAM)["width"]
    return {k: v.reshape((H, W) + v.shape[1:]) for k, v in out.items()}


def _word(d, tr):
    return (np.uint64(np.array(d, dtype=F).view(np.uint32)) << np.uint64(32)) | np.uint64(tr)


def test_square_on_triangle_at_distance_3():
    r = _render(TRI, [[0, 1, 2]], COL)
    assert r["words"].dtype == np.uint64 and r["rgb"].dtype == F and r["rgb_u8"].dtype == np.uint8
    assert r["depth"].dtype == F and r["triangle"].dtype == np.int32
    cov = r["triangle"] >= 0
    assert np.array_equal(cov, np.isfinite(r["depth"])) and np.array_equal(cov, r["words"] != rref.EMPTY)
    assert cov.sum() == 7 + 5 + 5 + 3 + 3 + 1 + 1                    # rows 7 .. 1: an edge pixel lost each side every 2 rows
    assert np.array_equal(r["depth"], mref.depth_map(np.array(TRI, dtype=F), np.array([[0, 1, 2]]), mref.camera(**CAM)))
    assert r["depth"][5, 4] == F(3.0) * np.sqrt(F(1.0) + F(1.0 / 64))          # the centroid: the ray (0, -1 / 8, -1)
    assert r["words"][5, 4] == _word(F(3.0) * np.sqrt(F(1.0) + F(1.0 / 64)), 0)
    assert r["rgb"][5, 4] == pytest.approx(COL.astype(np.float64).mean(axis=0), abs=1e-6)       # (0.4, 0.4, 1 / 3)
    assert r["rgb"][5, 4] == pytest.approx([0.4, 0.4, 1.0 / 3], abs=1e-6)
    for (i, j), k in (((1, 7), 0), ((7, 7), 1), ((4, 1), 2)):        # a vertex pixel gets that vertex's colour
        assert cov[j, i] and r["rgb"][j, i] == pytest.approx(COL[k], abs=1e-6), (i, j)
    assert r["rgb"][7, 4] == pytest.approx((COL[0].astype(np.float64) + COL[1]) / 2, abs=1e-6)   # the midpoint of the edge 0-1
    # uncovered pixels: the background, +inf, -1, and the background's bytes
    assert not cov[0, 0] and np.array_equal(r["rgb"][0, 0], np.array(BG, dtype=F))
    assert r["depth"][0, 0] == INF and r["triangle"][0, 0] == -1
    assert r["rgb_u8"][0, 0].tolist() == [63, 127, 191]              # 63.75, 127.5, 191.25 truncated
    assert r["rgb_u8"][7, 1].tolist() == [int(F(c) * F(255.0)) for c in r["rgb"][7, 1]]
    # the other winding is the same picture
    r2 = _render(TRI, [[0, 2, 1]], COL)
    assert np.array_equal(r2["triangle"], r["triangle"]) and np.abs(r2["rgb"] - r["rgb"]).max() <= 1e-6


def test_midpoint_of_a_slanted_edge_is_the_mean_of_its_ends():
    # corners on pixels (0, 8), (8, 8), (4, 0): the edge from (8, 8) to (4, 0) passes pixel (6, 4) at its midpoint
    tri = [[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]]
    r = _render(tri, [[0, 1, 2]], COL)
    assert r["triangle"][4, 6] == 0 and r["triangle"][4, 2] == 0
    assert r["rgb"][4, 6] == pytest.approx((COL[1].astype(np.float64) + COL[2]) / 2, abs=1e-6)
    assert r["rgb"][4, 2] == pytest.approx((COL[0].astype(np.float64) + COL[2]) / 2, abs=1e-6)


def test_ties_and_order():
    a = [[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]]
    # two coincident triangles: the lower index wins, whichever way round they stand
    r = _render(a + a, [[0, 1, 2], [3, 4, 5]], np.concatenate([COL, COL[::-1]]))
    assert set(np.unique(r["triangle"])) == {-1, 0}
    r = _render(a + a, [[3, 4, 5], [0, 1, 2]], np.concatenate([COL, COL[::-1]]))
    assert set(np.unique(r["triangle"])) == {-1, 0}
    assert r["rgb"][8, 0] == pytest.approx(COL[2], abs=1e-6)         # triangle 0 is now the one with the reversed colours
    # two triangles sharing the edge x = 0 through the column of pixel centres i = 4: both hit it at the same distance
    quad = [[-1.5, -1.5, -3], [0, -1.5, -3], [0, 1.5, -3], [1.5, -1.5, -3]]
    r = _render(quad, [[0, 1, 2], [1, 3, 2]], np.array([[1, 0, 0]] * 4, dtype=F))
    assert (r["triangle"][1:, 4] == 0).all() and r["triangle"][8, 3] == 0 and r["triangle"][8, 5] == 1
    r = _render(quad, [[1, 3, 2], [0, 1, 2]], np.array([[1, 0, 0]] * 4, dtype=F))
    assert (r["triangle"][1:, 4] == 0).all() and r["triangle"][8, 3] == 1 and r["triangle"][8, 5] == 0
    # a nearer triangle with a higher index still wins
    near = [[-0.5, -0.5, -2], [0.5, -0.5, -2], [0, 0.5, -2]]          # pixels 2 .. 6 of rows 2 .. 6
    r = _render(a + near, [[0, 1, 2], [3, 4, 5]], np.zeros((6, 3), dtype=F))
    assert r["triangle"][4, 4] == 1 and r["depth"][4, 4] == 2.0 and r["words"][4, 4] == _word(2.0, 1)
    assert r["triangle"][8, 0] == 0                                  # beside the nearer one the farther shows


def test_triangles_that_cover_nothing():
    tri = [[0, 1, 2]]
    none = lambda r: (r["triangle"] == -1).all() and (r["words"] == rref.EMPTY).all() and (r["depth"] == INF).all()
    assert none(_render([[-1.5, -1.5, 3], [1.5, -1.5, 3], [0, 1.5, 3]], tri, COL))                 # behind the camera
    assert none(_render([[-1.5, -1.5, -3], [np.nan, -1.5, -3], [0, 1.5, -3]], tri, COL))           # a NaN vertex
    assert none(_render([[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]], [[0, 1, 3]], COL))      # an index out of range
    assert none(_render([[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]], [[-1, 1, 2]], COL))
    assert none(_render(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3))))
    # one straddling the camera plane is seen where it lies in front (test_meshcolor_cpu.py has the picture) ...
    r = _render([[-1, -1, -3], [1, -1, -3], [0, 1, 1]], tri, COL)
    assert (r["triangle"][:7, 4] == 0).all() and (r["triangle"][7:, 4] == -1).all()
    assert np.array_equal(np.isfinite(r["depth"]), r["triangle"] == 0)
    # ... and a culled triangle keeps its number: the one after it is still number 1
    ver = [[-1.5, -1.5, 3], [1.5, -1.5, 3], [0, 1.5, 3]] + TRI
    r = _render(ver, [[0, 1, 2], [3, 4, 5]], np.concatenate([COL, COL]))
    assert set(np.unique(r["triangle"])) == {-1, 1}


def test_words_that_are_not_the_rasters():
    """The buffer is the caller's: a triangle number >= T, or a triangle with an index out of range, is uncovered."""
    ver, cam = np.array(TRI, dtype=F), mref.camera(**CAM)
    words = np.full(81, rref.EMPTY, dtype=np.uint64)
    words[39] = _word(3.0, 1)                                        # T == 1
    words[41] = _word(3.0, 0xFFFFFFFE)
    words[40] = _word(123.0, 0)                                      # the centre pixel; the distance is recomputed, not believed
    r = rref.shade(ver, np.array([[0, 1, 2]]), cam, words, "color", COL, BG)
    assert r["triangle"][39] == -1 and r["triangle"][41] == -1 and r["depth"][39] == INF and r["depth"][41] == INF
    assert np.array_equal(r["rgb"][39], np.array(BG, dtype=F)) and r["rgb_u8"][41].tolist() == [63, 127, 191]
    full = rref.render(ver, np.array([[0, 1, 2]]), cam, "color", COL, BG)
    assert r["triangle"][40] == 0 and r["depth"][40] == full["depth"][40] == 3.0 and np.array_equal(r["rgb"][40], full["rgb"][40])
    r = rref.shade(ver, np.array([[0, 1, 7]]), cam, np.full(81, _word(3.0, 0), dtype=np.uint64), "color", COL, BG)
    assert (r["triangle"] == -1).all()


def test_bytes_clamp_truncate_and_nan():
    col = np.array([[np.nan, 1.5, -0.5]] * 3, dtype=F)
    r = _render(TRI, [[0, 1, 2]], col)
    assert r["triangle"][5, 4] == 0
    assert np.isnan(r["rgb"][5, 4, 0]) and r["rgb"][5, 4, 1] == pytest.approx(1.5, abs=1e-6)      # the floats are not clamped
    assert r["rgb"][5, 4, 2] == pytest.approx(-0.5, abs=1e-6)
    assert r["rgb_u8"][5, 4].tolist() == [0, 255, 0]
    assert rref.to_bytes([0.0, 1.0, 0.999, 0.5, 1.0 / 255, np.inf, -np.inf]).tolist() == [0, 255, 254, 127, 1, 255, 0]


def test_normal_and_facing_modes():
    n = np.array([[0, 0, 2.0]] * 3, dtype=F)                         # any length: the interpolated normal is normalised
    r = _render(TRI, [[0, 1, 2]], n, mode="normal")
    assert r["rgb"][5, 4] == pytest.approx([0.5, 0.5, 1.0], abs=1e-6) and r["rgb_u8"][5, 4].tolist() == [127, 127, 255]
    r = _render(TRI, [[0, 1, 2]], np.zeros((3, 3), dtype=F), mode="normal")       # zero length: grey
    assert np.array_equal(r["rgb"][5, 4], np.array([0.5, 0.5, 0.5], dtype=F))
    r = _render(TRI, [[0, 1, 2]], np.full((3, 3), np.nan, dtype=F), mode="normal")
    assert np.array_equal(r["rgb"][5, 4], np.array([0.5, 0.5, 0.5], dtype=F))
    r = _render([[-1.5, -1.5, -3], [1.5, -1.5, -3], [0, 1.5, -3]], [[0, 1, 2]], mode="facing")
    assert r["rgb"][4, 4] == pytest.approx([1.0] * 3, abs=1e-6)                   # square-on, down the axis
    assert r["rgb"][8, 0] == pytest.approx([1 / np.sqrt(1.5)] * 3, abs=1e-6)      # the ray (-0.5, -0.5, -1) against (0, 0, 1)
    assert np.array_equal(r["rgb"][0, 0], np.array(BG, dtype=F))
    # 45 degrees: the plane z = -3 + x
    r = _render([[-1, -1, -4], [1, -1, -2], [0, 1, -3]], [[0, 1, 2]], mode="facing")
    assert r["rgb"][4, 4] == pytest.approx([np.sqrt(0.5)] * 3, abs=1e-6)


@pytest.mark.parametrize("k", [0, 37, 128, 254])
def test_flat_colour_gives_its_byte_at_every_covered_pixel(k):
    ver, tri = mref.soup(400, 7)
    col = np.full((ver.shape[0], 3), (k + 0.5) / 255, dtype=F)
    r = rref.render(ver, tri, mref.camera(**mref.SOUP_CAMERA), "color", col, BG)
    cov = r["triangle"] >= 0
    assert cov.mean() > 0.5 and (r["rgb_u8"][cov] == k).all()
    assert (r["rgb_u8"][~cov] == np.array([63, 127, 191], dtype=np.uint8)).all()


def test_render_fp32_against_fp64_on_the_soup():
    """The restatement's fp32 against the same algorithm in fp64, on the soup with random vertex colours.  A pixel may be
    left out when its fp64 barycentrics come within 1e-5 of an edge of any triangle, or when its two nearest fp64 hits lie
    within 1e-5 relative of each other; at most 1 % of the pixels.  Elsewhere the winner and the coverage agree exactly and
    the colour to 1e-5 absolute (four times the 2.5e-6 measured: a grazing triangle divides by a small determinant)."""
    ver, tri = mref.soup(400, 7)
    cam = mref.camera(**mref.SOUP_CAMERA)
    col = np.random.default_rng(11).uniform(size=(ver.shape[0], 3)).astype(F)
    d32, w32 = rref.nearest(ver, tri, cam)
    d64, w64 = rref.nearest(ver, tri, cam, dtype=np.float64)
    s32 = rref.shade_at(ver, tri, cam, w32, "color", col, BG)
    s64 = rref.shade_at(ver, tri, cam, w64, "color", col, BG, dtype=np.float64)
    dx, dy = mref.pixel_rays(cam)
    a, b, c = (ver[tri[:, k]] for k in range(3))
    hit, tau, u, v = mref.intersect(a, b, c, dx, dy, np.float64)
    e = 1e-5
    with np.errstate(all="ignore"):
        near = ((np.abs(u) < e) | (np.abs(v) < e) | (np.abs(1.0 - u - v) < e)) & (u > -e) & (v > -e) & (u + v < 1 + e) & (tau > 0)
        two = np.sort(np.where(hit, tau, np.inf), axis=0)[:2]
        close = np.isfinite(two[1]) & (two[1] - two[0] <= e * two[0])
    edge = near.any(axis=0)
    left_out = edge | close
    keep = ~left_out
    covered = w64 >= 0
    both = covered & keep
    worst_rgb = np.abs(s32["rgb"][both].astype(np.float64) - s64["rgb"][both]).max()
    worst_uv = max(np.abs(s32["u"][both] - s64["u"][both]).max(), np.abs(s32["v"][both] - s64["v"][both]).max())
    print(f"soup: {covered.mean():.3f} covered, {edge.mean():.4f} left out by the edge rule, {close.mean():.4f} by the tie rule, "
          f"{int((w32 != w64)[keep].sum())} winners differ, worst colour difference {worst_rgb:.3e}, worst u / v {worst_uv:.3e}")
    assert 0.5 < covered.mean() < 0.75
    assert left_out.mean() <= 0.01
    assert np.array_equal(w32[keep], w64[keep])
    assert np.array_equal(s32["triangle"][keep], s64["triangle"][keep])
    assert worst_rgb <= 1e-5
