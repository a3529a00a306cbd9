"""GPU checks of nerf_fl_amd.geometry: the extraction kernels (csrc/nfl_surface.hip) against the numpy restatement of
tests/geometry_ref.py, density_lattice against field_forward on the same points, extract_mesh end to end.

Tolerance of positions and normals against the fp32 restatement.  Both sides evaluate the same fp32 formulae with every
operation rounded on its own (the library is built with -ffp-contract=off; division and square root are correctly
rounded on both), so they can differ only where a compiler contracts or reorders.  MEASURED worst deviation over all the
cases below on an MI355X: positions 0.0, normals 0.0 (bit-identical).  Allowed: 4 x the measured value, but at least
1 ulp of the lattice extent (positions: of the largest coordinate of the box; normals: of 1)."""
import numpy as np
import pytest
import torch

import geometry_ref as gr
import nerf_fl_amd
from gpu_util import DEV, make_embeddings
from nerf_fl_amd import NeRF, geometry, rendering, synth

pytestmark = pytest.mark.gpu

MEASURED_POS, MEASURED_NRM = 0.0, 0.0           # see the module docstring
SIGMA_TOL = 1e-4                                 # the project's forward bar, relative to max(1, |sigma|)


def _ulp(x):
    return float(np.spacing(np.float32(x)))


def _run(lat, iso, lo, hi):
    lat = np.ascontiguousarray(lat, dtype=np.float32)
    got = geometry.extract_surface(torch.from_numpy(lat).to(DEV), iso, lo, hi)
    nz, ny, nx = lat.shape
    sp = [np.float32((h - l) / (n - 1)) for l, h, n in zip(lo, hi, (nx, ny, nz))]
    exp = gr.extract(lat, iso, lo, sp)
    return {k: v.cpu().numpy() for k, v in got.items()}, exp


def _close(a, b, tol):
    with np.errstate(invalid="ignore"):
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
    same = (a == b) | (np.isnan(a) & np.isnan(b))           # equal infinities and NaN on both sides count as equal
    d = np.where(same, 0.0, d)
    worst = float(np.nan_to_num(d, nan=np.inf).max()) if d.size else 0.0
    return worst, worst <= tol


def _check(lat, iso, lo, hi, what):
    got, exp = _run(lat, iso, lo, hi)
    assert got["vertices"].shape == exp["vertices"].shape, what            # V
    assert got["triangles"].shape == exp["triangles"].shape, what          # T
    assert got["triangles"].dtype == np.int32 and np.array_equal(got["triangles"], exp["triangles"]), what
    extent = max(abs(float(v)) for v in tuple(lo) + tuple(hi))
    dp, ok_p = _close(got["vertices"], exp["vertices"], max(4 * MEASURED_POS, _ulp(extent)))
    dn, ok_n = _close(got["normals"], exp["normals"], max(4 * MEASURED_NRM, _ulp(1.0)))
    print(f"{what}: V={len(exp['vertices'])} T={len(exp['triangles'])} worst position dev {dp:.3e} normal dev {dn:.3e}")
    assert ok_p and ok_n, (what, dp, dn)
    return got


def test_all_corner_patterns():
    """2 x 2 x 2, each of the 256 inside / outside patterns: every tetrahedron case and every edge type."""
    for pattern in range(256):
        lat = np.array([1.0 if (pattern >> c) & 1 else -1.0 for c in range(8)], dtype=np.float32).reshape(2, 2, 2)
        got = _check(lat, 0.0, (0.0, 1.0, -1.0), (1.0, 3.0, -0.5), f"pattern {pattern}")
        if pattern in (0, 255):
            assert len(got["vertices"]) == 0 and len(got["triangles"]) == 0


def test_centre_inside_is_closed():
    lat = -np.ones((3, 3, 3), dtype=np.float32)
    lat[1, 1, 1] = 2.0
    got = _check(lat, 0.0, (-1, -1, -1), (1, 1, 1), "3x3x3 centre")
    tri = got["triangles"].astype(np.int64)
    e = np.sort(np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]), axis=1)
    und, cnt = np.unique(e, axis=0, return_counts=True)
    assert (cnt == 2).all() and len(got["vertices"]) - len(und) + len(tri) == 2
    assert len(got["vertices"]) == 14                                        # one crossing per edge that leaves the centre


@pytest.mark.parametrize("shape", [(3, 4, 5), (7, 9, 33), (2, 3, 65), (5, 6, 300), (67, 62, 3), (91, 91, 3)])
def test_random_lattices(shape):
    """(nz, ny, nx): distinct sizes so that strides are not interchangeable; 33 and 65 cross wave boundaries, 300 the
    256-point slab of a workgroup.  The two thin ones have 4154 and 8281 slabs: nfl_surface_scan_kernel takes 4096 a round,
    so it carries its sums over a full and a ragged round, and over three."""
    rng = np.random.default_rng(sum(shape))
    lat = rng.standard_normal(shape).astype(np.float32)
    _check(lat, 0.25, (-1.0, 0.5, 2.0), (2.0, 1.5, 2.75), f"random {shape}")


def test_values_equal_to_iso():
    rng = np.random.default_rng(5)
    lat = rng.integers(-1, 2, size=(6, 5, 7)).astype(np.float32)           # a third of the points exactly at iso
    _check(lat, 0.0, (0, 0, 0), (6, 4, 5), "values at iso")
    _check(np.zeros((3, 3, 3), np.float32), 0.0, (0, 0, 0), (1, 1, 1), "all at iso")


def test_nan_and_inf_values():
    rng = np.random.default_rng(6)
    lat = rng.standard_normal((5, 6, 9)).astype(np.float32)
    flat = lat.reshape(-1)
    flat[rng.choice(flat.size, 40, replace=False)] = np.nan
    flat[rng.choice(flat.size, 10, replace=False)] = np.inf
    flat[rng.choice(flat.size, 10, replace=False)] = -np.inf
    _check(lat, 0.0, (-1, -1, -1), (1, 1, 1), "NaN and inf")
    _check(np.full((3, 3, 3), np.nan, np.float32), 0.0, (0, 0, 0), (1, 1, 1), "all NaN")


def test_all_outside():
    got = _check(-np.ones((4, 5, 6), np.float32), 0.0, (0, 0, 0), (1, 1, 1), "all outside")
    assert got["vertices"].shape == (0, 3) and got["normals"].shape == (0, 3) and got["triangles"].shape == (0, 3)


def test_sphere_and_reproducibility():
    lat, lo, sp = gr.sphere_lattice(24)
    _check(lat, 0.0, (-1, -1, -1), (1, 1, 1), "sphere 24^3")
    d = torch.from_numpy(lat).to(DEV)
    a = geometry.extract_surface(d, 0.0, (-1, -1, -1), (1, 1, 1))
    b = geometry.extract_surface(d, 0.0, (-1, -1, -1), (1, 1, 1))
    for k in a:
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k      # bit-identical


def test_extract_surface_rejects_bad_inputs():
    x = torch.zeros(4, 4, 4, device=DEV)
    with pytest.raises(ValueError):
        geometry.extract_surface(x.double(), 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        geometry.extract_surface(x[:, :, ::2], 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        geometry.extract_surface(x[0], 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        geometry.extract_surface(x[:1], 0.0, (0, 0, 0), (1, 1, 1))
    with pytest.raises(ValueError):
        geometry.extract_surface(x, 0.0, (0, 0, 0), (1, 0, 1))


# ---- the field on a lattice

def _model(kind):
    kw = dict(encode_appearance=True, encode_transient=True) if kind == "nerfw" else {}
    m = NeRF("fine", **kw)
    m.load_state_dict(synth.make_field_params(12 if kind == "base" else 13, "sharp", typ="fine", **kw))
    return m.to(DEV)


@pytest.fixture(scope="module", params=["base", "nerfw"])
def field(request):
    nerf_fl_amd.set_precision("f16x3")
    try:
        rendering.check_status(DEV)          # start from a clean status word, whatever ran before
    except FloatingPointError:
        pass
    return request.param, _model(request.param), make_embeddings(10, False)


@pytest.mark.parametrize("res", [(70, 3, 2), (8, 4, 4), (300, 2, 2)])
def test_density_lattice_matches_field_forward(field, res):
    """Against field_forward on the same points encoded with nfl_posenc.  70 is no multiple of the kernel's 32-sample
    segment (the tail mask); 300 is cut into two pieces of 160 (the dropped samples past the row's end); a chunk of 200
    points forces several passes.  MEASURED worst relative error on an MI355X: 0.0 (bit-identical) for both models (base,
    nerfw) at each of (70, 3, 2), (8, 4, 4) and (300, 2, 2): both routes run the same fused kernel on the same fp32
    positions.  The bar stays the project's forward bar."""
    kind, model, emb = field
    lo, hi = (-1.1, -0.9, -0.4), (1.2, 0.8, 0.5)
    with torch.no_grad():
        got = geometry.density_lattice(model, emb, lo, hi, res, chunk=200 if res[0] == 70 else 1 << 20)
        pts = geometry.lattice_points(lo, hi, res, DEV)
        exp = rendering.field_forward(model, rendering.posenc(pts.reshape(-1, 3), 10), sigma_only=True)
    assert got.shape == (res[2], res[1], res[0]) and got.dtype == torch.float32 and got.is_contiguous()
    exp = exp.reshape(got.shape)
    err = ((got - exp).abs() / exp.abs().clamp(min=1.0)).max().item()
    print(f"density_lattice {kind} {res}: worst relative error {err:.3e}, sigma in [{exp.min().item():.3g}, {exp.max().item():.3g}]")
    assert err <= SIGMA_TOL
    rendering.check_status(DEV)


def test_density_lattice_with_colour(field):
    kind, model, emb = field
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (40, 3, 2)
    a_emb = torch.linspace(-1, 1, 48, device=DEV) if kind == "nerfw" else None
    view = torch.tensor([0.0, 0.6, -0.8], device=DEV)
    with torch.no_grad():
        sigma, rgb = geometry.density_lattice(model, emb, lo, hi, res, a_embedded=a_emb, view_dir=view)
        pts = geometry.lattice_points(lo, hi, res, DEV).reshape(-1, 3)
        cols = [rendering.posenc(pts, 10), rendering.posenc(view.expand(len(pts), 3), 4)]
        if a_emb is not None:
            cols.append(a_emb.expand(len(pts), 48))
        exp = rendering.field_forward(model, torch.cat(cols, 1), output_transient=False)
    assert rgb.shape == (2, 3, 40, 3)
    assert ((sigma.reshape(-1) - exp[:, 3]).abs() / exp[:, 3].abs().clamp(min=1.0)).max().item() <= SIGMA_TOL
    assert (rgb.reshape(-1, 3) - exp[:, :3]).abs().max().item() <= SIGMA_TOL
    if kind == "nerfw":
        with pytest.raises(ValueError):
            geometry.density_lattice(model, emb, lo, hi, res, view_dir=view)          # appearance code missing


def test_extract_mesh_end_to_end(field, tmp_path):
    kind, model, emb = field
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (16, 16, 16)
    a_emb = torch.linspace(-1, 1, 48, device=DEV) if kind == "nerfw" else None
    with torch.no_grad():
        iso = geometry.density_lattice(model, emb, lo, hi, res).median().item()
        path = str(tmp_path / "mesh.ply")
        mesh = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, a_embedded=a_emb, path=path)
    V, T = mesh["vertices"].shape[0], mesh["triangles"].shape[0]
    assert V > 0 and T > 0
    assert mesh["vertices"].shape == mesh["normals"].shape == mesh["colors"].shape == (V, 3)
    assert mesh["triangles"].dtype == torch.int32 and 0 <= mesh["triangles"].min() and mesh["triangles"].max() == V - 1
    assert mesh["vertices"].abs().max().item() <= 1 + 1e-6            # inside the box (its far corner is lo + 15 s in fp32)
    assert (mesh["colors"] >= 0).all() and (mesh["colors"] <= 1).all()
    length = mesh["normals"].norm(dim=1)
    assert (((length - 1).abs() <= 1e-5) | (length == 0)).all()
    rendering.check_status(DEV)                                              # the status word is clean
    raw = open(path, "rb").read()
    assert raw.startswith(b"ply\n") and f"element vertex {V}\n".encode() in raw and f"element face {T}\n".encode() in raw
