"""GPU checks of the mesh smoothing (csrc/nfl_meshsmooth.hip through nerf_fl_amd.geometry.mesh_adjacency / smooth_mesh /
vertex_normals) against the numpy restatement of tests/meshsmooth_ref.py.

What is compared how.  The offsets, the neighbour and incident rows, the boundary flags and the totals are integers: EXACT.
The smoothed positions are a sequential fp64 sum in the order of a sorted row, a division, three fp64 operations and one
rounding to fp32, none of which the device is free to reorder or fuse: EXACT on the bits.  Normals go through an fp64
square root and a division per triangle ("uniform") and per vertex: 1e-6 absolute, the bar tests/test_simplify_gpu.py
sets for the same two operations; a row taken from the fallback is equal bit for bit.

Sizes.  Kernels run 256 threads (4 waves) a workgroup: 63 / 64 / 65 cross a wave, 257 a workgroup.  The scan works on
tiles of 2048: the soup of 70 000 vertices and 150 000 triangles crosses 35 of them (two levels).  A row of up to 24
incident entries is sorted by its thread, a longer one by its workgroup: the dense soups (5 vertices with rows of about
240, 40 with rows of 15 to 32) and the fan (a hub of 4096 triangles beside 4396 rows of a few) take both paths in one launch;
a long row of up to 8192 words is sorted in LDS (the hub's 4096 entries and 8192 candidates just fit), a longer one by a
rank sort through tiles of 12 288 words, so `test_a_row_longer_than_the_lds` has hubs of 5000 and 8200 triangles."""
import ctypes as C

import numpy as np
import pytest
import torch

import meshsmooth_ref as mr
import nerf_fl_amd
from geom_gpu_util import bits as _bits, same as _same, to_dev as _to_dev
from gpu_util import DEV, make_embeddings
from nerf_fl_amd import NeRF, _lib, geometry, rendering, synth

pytestmark = pytest.mark.gpu

ADJ_KEYS = ("offsets", "neighbors", "boundary", "tri_offsets", "incident")


def _normals_close(got, exp, what):
    """Within 1e-6 absolute; a row copied bit for bit (a fallback may carry anything) is equal.  Returns the worst."""
    got, exp = got.cpu().numpy() if torch.is_tensor(got) else got, np.asarray(exp)
    assert got.dtype == np.float32 and got.shape == exp.shape, what
    with np.errstate(invalid="ignore"):
        diff = np.where(_bits(got) == _bits(exp), 0.0, np.abs(got.astype(np.float64) - exp.astype(np.float64)))
    worst = float(diff.max()) if diff.size else 0.0
    print(f"normals, {what}: worst {worst:.3e} against the restatement")
    assert worst <= 1e-6, (what, "normals")                                  # a NaN difference fails the comparison
    return worst


def _check_adjacency(mesh, what, dev=None):
    V = len(mesh["vertices"])
    exp = mr.adjacency(mesh["triangles"], V)
    got = geometry.mesh_adjacency(dev if dev is not None else _to_dev(mesh))
    assert set(got) == set(ADJ_KEYS) | {"n_boundary"}, what
    for k in ADJ_KEYS:
        _same(got[k], exp[k], (what, k))
    assert [got["incident"].shape[0], got["neighbors"].shape[0], got["n_boundary"]] == [exp["totals"][0], exp["totals"][1], exp["totals"][3]]
    return got, exp


def _check_all(mesh, what, dev=None, iterations=2):
    """Adjacency, Taubin and Laplacian steps with both boundary rules, both normal weightings."""
    dev = dev if dev is not None else _to_dev(mesh)
    adj, exp_adj = _check_adjacency(mesh, what, dev)
    for boundary, mu in (("fixed", -0.53), ("free", -0.53), ("free", None)):
        got = geometry.smooth_mesh(dev, iterations, mu=mu, boundary=boundary, adjacency=adj, normals=None)
        exp = mr.smooth(mesh["vertices"], exp_adj, mr.factors(iterations, 0.5, mu), fix_boundary=boundary == "fixed")
        _same(got["vertices"], exp, (what, boundary, mu, "vertices"))
        assert got["normals"] is dev["normals"] and got["triangles"] is dev["triangles"]
    for weighting in (mr.AREA, mr.UNIFORM):
        got = geometry.vertex_normals(dev, weighting=weighting, adjacency=adj, fallback=dev["normals"])
        _normals_close(got, mr.normals(mesh["vertices"], mesh["triangles"], exp_adj, weighting, mesh["normals"]), f"{what}, {weighting}")
    return adj, exp_adj


# ---- small cases

@pytest.mark.parametrize("name", sorted(set(mr.hand_cases()) - {"out_of_range"}))
def test_hand_cases(name):
    _check_all(mr.hand_cases()[name], name)


def test_grid_patch_fixed_and_free():
    mesh = mr.grid_patch(5)
    adj, _ = _check_all(mesh, "grid patch", iterations=3)
    assert adj["n_boundary"] == 16
    dev = _to_dev(mesh)
    fixed = geometry.smooth_mesh(dev, 3)["vertices"]
    rim = adj["boundary"]
    _same(fixed[rim], mesh["vertices"][rim.cpu().numpy()], "the rim stays")
    assert (geometry.smooth_mesh(dev, 3, boundary="free")["vertices"][rim] != dev["vertices"][rim]).any(dim=1).all()


def test_empty_mesh_launches_nothing():
    mesh = _to_dev(mr._mesh(np.zeros((0, 3)), np.zeros((0, 3))))
    adj = geometry.mesh_adjacency(mesh)
    assert adj["offsets"].tolist() == [0] and adj["tri_offsets"].tolist() == [0] and adj["n_boundary"] == 0
    assert adj["neighbors"].shape == adj["incident"].shape == adj["boundary"].shape == (0,)
    out = geometry.smooth_mesh(mesh)
    assert out["vertices"].shape == out["normals"].shape == (0, 3) and out["normals"] is not mesh["normals"]
    assert geometry.vertex_normals(mesh).shape == (0, 3)


@pytest.mark.parametrize("V", [1, 63, 64, 65, 257])
def test_small_soups(V):
    _check_all(mr.soup(V, 3 * V + 1, seed=V), f"V = {V}")


@pytest.mark.parametrize("V,T", [(5, 400), (40, 300), (2, 30)])
def test_dense_soups_take_the_workgroup_path(V, T):
    mesh = mr.soup(V, T, seed=V + T)
    _, exp = _check_all(mesh, f"V = {V}, T = {T}")
    longest = int(np.diff(exp["tri_offsets"]).max())
    assert longest > _lib.ADJ_SHORT_ROW
    if V == 40:
        assert int(np.diff(exp["tri_offsets"]).min()) <= _lib.ADJ_SHORT_ROW      # both paths in one workgroup


# ---- the soup that crosses scan tiles

@pytest.fixture(scope="module")
def big_soup():
    mesh = mr.soup(70_000, 150_000, seed=1)
    return mesh, _to_dev(mesh)


def test_big_soup(big_soup):
    mesh, dev = big_soup
    adj, exp = _check_all(mesh, "soup", dev)
    assert exp["totals"][0] == 450_000                                          # two scan levels
    again = geometry.mesh_adjacency(dev)                                        # two runs: identical bits
    for k in ADJ_KEYS:
        _same(again[k], _bits(adj[k]), k)
    one, two = geometry.smooth_mesh(dev, 2, normals="uniform"), geometry.smooth_mesh(dev, 2, normals="uniform")
    for k in ("vertices", "normals"):
        _same(one[k], _bits(two[k]), k)


# ---- long rows

def test_fan_hub_beside_ordinary_rows():
    mesh = mr.fan(4096, 300, seed=0)
    dev = _to_dev(mesh)
    adj, exp = _check_all(mesh, "fan", dev)
    rows = np.diff(exp["offsets"])
    assert rows[0] == 4096 and np.diff(exp["tri_offsets"])[0] == 4096 and (rows[1:] <= 4).all() and len(rows) == 4397
    assert not exp["boundary"][0] and exp["boundary"][1:].all()                 # the rim's outer edges have one triangle
    again = geometry.mesh_adjacency(dev)
    for k in ADJ_KEYS:
        _same(again[k], _bits(adj[k]), k)


@pytest.mark.parametrize("hub", [5000, 8200])
def test_a_row_longer_than_the_lds(hub):
    """Past 8192 words a long row is rank-sorted through tiles of 12 288: the 10 000 candidates of 5000 triangles (their
    entries still sort in LDS), the 8200 entries and 16 400 candidates (two tiles) of 8200."""
    mesh = mr.fan(hub, 20, seed=1)
    mesh["triangles"][5] = mesh["triangles"][6]                                 # a duplicate: multiplicities of 3
    _check_all(mesh, f"fan of {hub}")


# ---- a real surface

def test_noisy_ball_through_ten_taubin_iterations():
    clean, noisy = mr.noisy_ball(33)
    dev = _to_dev(noisy)
    adj, exp_adj = _check_adjacency(noisy, "ball", dev)
    assert adj["n_boundary"] == 0 and exp_adj["totals"][2] == 0
    exp = mr.smooth_mesh(noisy, 10)
    got = geometry.smooth_mesh(dev, 10)
    _same(got["vertices"], exp["vertices"], "vertices")
    _normals_close(got["normals"], exp["normals"], "ball after 10 Taubin iterations")
    assert got["triangles"] is dev["triangles"] and "colors" not in got
    r = got["vertices"].double().norm(dim=1)
    r0 = dev["vertices"].double().norm(dim=1)
    assert (r - r.mean()).pow(2).mean().sqrt().item() < 0.5 * (r0 - r0.mean()).pow(2).mean().sqrt().item()
    with_adj = geometry.smooth_mesh(dict(dev, colors=dev["normals"]), 10, adjacency=adj)
    for k in ("vertices", "normals"):
        _same(with_adj[k], _bits(got[k]), k)                                    # the adjacency handed in = the one built
    assert with_adj["colors"] is dev["normals"]
    n = geometry.vertex_normals(_to_dev(clean))
    assert ((n * torch.from_numpy(clean["normals"]).to(DEV)).sum(dim=1) > 0).all()


# ---- the C ABI: step parities, pins, bounded reads, nothing outside the outputs

GUARD = 64


def _framed(n, dtype, tail=()):
    fill = -7 if dtype != torch.uint8 else 249
    return torch.full((n + 2 * GUARD,) + tail, fill, dtype=dtype, device=DEV)


def _frame_intact(buf, n):
    fill = -7 if buf.dtype != torch.uint8 else 249
    return bool((buf[:GUARD] == fill).all() and (buf[GUARD + n:] == fill).all())


def _smooth_abi(ver, off, nbr, steps, boundary=None, pinned=None, fix=0):
    """nfl_mesh_smooth on device tensors with every buffer framed -> (V, 3) fp32 tensor."""
    lib = _lib.lib()
    V = ver.shape[0]
    nbytes = lib.nfl_mesh_smooth_bytes(V)
    assert nbytes % 8 == 0
    scratch, out = _framed(nbytes // 8, torch.int64), _framed(V, torch.float32, (3,))
    keep = ver.clone()
    a = _lib.MeshSmoothArgs()
    a.d_vertices, a.d_offsets, a.d_neighbors = ver.data_ptr(), off.data_ptr(), nbr.data_ptr() if nbr.numel() else None
    a.n_vertices, a.n_neighbors = V, nbr.shape[0]
    a.d_boundary = boundary.data_ptr() if boundary is not None else None
    a.d_pinned = pinned.data_ptr() if pinned is not None else None
    a.fix_boundary, a.n_steps = fix, len(steps)
    host = (C.c_double * max(len(steps), 1))(*steps)
    a.factors = host
    a.d_scratch, a.scratch_bytes, a.d_out_vertices = scratch[GUARD:].data_ptr(), nbytes, out[GUARD:].data_ptr()
    _lib.check(lib.nfl_mesh_smooth(C.byref(a), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_mesh_smooth")
    torch.cuda.synchronize()
    assert _frame_intact(scratch, nbytes // 8) and _frame_intact(out, V)
    _same(ver, _bits(keep), "the input is never written")
    return out[GUARD:GUARD + V]


@pytest.mark.parametrize("n_steps", [0, 1, 2, 3])
def test_step_parities_and_the_copy(n_steps):
    mesh = mr.soup(257, 700, seed=3)
    exp_adj = mr.adjacency(mesh["triangles"], 257)
    dev = _to_dev(mesh)
    adj = geometry.mesh_adjacency(dev)
    steps = [0.5, -0.53, 0.25][:n_steps]
    pinned = (torch.arange(257, device=DEV) % 5 == 0).to(torch.uint8)
    got = _smooth_abi(dev["vertices"], adj["offsets"], adj["neighbors"], steps, adj["boundary"].view(torch.uint8), pinned, 1)
    exp = mr.smooth(mesh["vertices"], exp_adj, steps, pinned=pinned.cpu().numpy(), fix_boundary=True)
    _same(got, exp, f"{n_steps} steps")
    assert np.isnan(got[3, 0].item())                                           # a vertex that is not finite stays as it is
    free = _smooth_abi(dev["vertices"], adj["offsets"], adj["neighbors"], steps)                 # no flags, no pins
    _same(free, mr.smooth(mesh["vertices"], exp_adj, steps, fix_boundary=False), f"{n_steps} free steps")
    via_python = geometry.smooth_mesh(dev, n_steps, lam=0.5, mu=None, boundary="free", pinned=pinned.bool(), normals=None)
    _same(via_python["vertices"], mr.smooth(mesh["vertices"], exp_adj, [0.5] * n_steps, pinned=pinned.cpu().numpy(), fix_boundary=False),
          "pinned as bool")


def test_a_foreign_csr_is_read_within_bounds():
    """Offsets that run backwards or past N give an empty row, a neighbour outside [0, V) is skipped: wrong positions,
    never an access out of range (the restatement is given the rows that remain)."""
    V = 65
    mesh = mr.soup(V, 200, seed=8)
    adj = mr.adjacency(mesh["triangles"], V)
    off, nbr = adj["offsets"].copy(), adj["neighbors"].copy()
    nbr[::7], nbr[3::11] = -1, V                                                  # skipped
    off[10], off[20], off[30] = off[12], -5, len(nbr) + 9                          # rows 9 / 10, 19 / 20 and 29 / 30 touched
    valid = np.array([0 <= off[v] <= off[v + 1] <= len(nbr) for v in range(V)])
    rows = [nbr[off[v]:off[v + 1]] if valid[v] else nbr[:0] for v in range(V)]
    rows = [r[(r >= 0) & (r < V)] for r in rows]
    clean = {"offsets": np.concatenate([[0], np.cumsum([len(r) for r in rows])]), "neighbors": np.concatenate(rows),
             "boundary": adj["boundary"]}
    got = _smooth_abi(torch.from_numpy(mesh["vertices"]).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(nbr).to(DEV), [0.5, -0.53])
    _same(got, mr.smooth(mesh["vertices"], clean, [0.5, -0.53], fix_boundary=False), "foreign CSR")


def test_adjacency_and_normals_outputs_are_framed_by_sentinels():
    V, T = 257, 700
    mesh = mr.soup(V, T, seed=3)
    mesh["triangles"][:9] = mesh["triangles"][0, 0]                              # 27 entries: past the thread path's length
    exp = mr.adjacency(mesh["triangles"], V)
    I, N = exp["totals"][:2]
    dev = _to_dev(mesh)
    lib = _lib.lib()
    nbytes = lib.nfl_mesh_adjacency_bytes(V, T)
    assert nbytes % 8 == 0
    scratch, totals = _framed(nbytes // 8, torch.int64), _framed(4, torch.int64)
    toff, off = _framed(V + 1, torch.int64), _framed(V + 1, torch.int64)
    inc, nbr, bnd = _framed(I, torch.int32), _framed(N, torch.int32), _framed(V, torch.uint8)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    a = _lib.MeshAdjacencyArgs()
    a.d_triangles, a.n_vertices, a.n_triangles = dev["triangles"].data_ptr(), V, T
    a.d_scratch, a.scratch_bytes, a.d_totals = scratch[GUARD:].data_ptr(), nbytes, totals[GUARD:].data_ptr()
    _lib.check(lib.nfl_mesh_adjacency_count(C.byref(a), stream), "nfl_mesh_adjacency_count")
    assert totals[GUARD:GUARD + 4].tolist() == exp["totals"]
    a.n_incident, a.n_neighbors = I, N
    a.d_tri_offsets, a.d_incident = toff[GUARD:].data_ptr(), inc[GUARD:].data_ptr()
    a.d_offsets, a.d_neighbors, a.d_boundary = off[GUARD:].data_ptr(), nbr[GUARD:].data_ptr(), bnd[GUARD:].data_ptr()
    _lib.check(lib.nfl_mesh_adjacency_emit(C.byref(a), stream), "nfl_mesh_adjacency_emit")
    normals = _framed(V, torch.float32, (3,))
    n = _lib.MeshNormalsArgs()
    n.d_vertices, n.d_triangles, n.n_vertices, n.n_triangles = dev["vertices"].data_ptr(), dev["triangles"].data_ptr(), V, T
    n.d_tri_offsets, n.d_incident, n.n_incident = toff[GUARD:].data_ptr(), inc[GUARD:].data_ptr(), I
    n.weighting, n.d_fallback_normals, n.d_out_normals = 1, None, normals[GUARD:].data_ptr()
    _lib.check(lib.nfl_mesh_normals(C.byref(n), stream), "nfl_mesh_normals")
    torch.cuda.synchronize()
    for buf, size in ((scratch, nbytes // 8), (totals, 4), (toff, V + 1), (off, V + 1), (inc, I), (nbr, N), (bnd, V), (normals, V)):
        assert _frame_intact(buf, size)                                          # nothing written out of range
    _same(toff[GUARD:GUARD + V + 1], exp["tri_offsets"], "tri_offsets")
    _same(off[GUARD:GUARD + V + 1], exp["offsets"], "offsets")
    _same(inc[GUARD:GUARD + I], exp["incident"], "incident")
    _same(nbr[GUARD:GUARD + N], exp["neighbors"], "neighbors")
    _same(bnd[GUARD:GUARD + V], exp["boundary"].astype(np.uint8), "boundary")
    _normals_close(normals[GUARD:GUARD + V], mr.normals(mesh["vertices"], mesh["triangles"], exp, mr.UNIFORM), "framed, no fallback")


# ---- the Python layer

def test_out_of_range_index_raises_with_the_count():
    with pytest.raises(ValueError, match="2 of 4 triangles"):
        geometry.mesh_adjacency(_to_dev(mr.hand_cases()["out_of_range"]))
    mesh = mr.soup(70, 40, seed=4)
    mesh["triangles"][[3, 17, 29]] = [[0, 1, 70], [-1, 4, 5], [2 ** 31 - 1, 6, 7]]
    for call in (geometry.mesh_adjacency, geometry.smooth_mesh, geometry.vertex_normals):
        with pytest.raises(ValueError, match="3 of 40 triangles"):
            call(_to_dev(mesh))
    empty = _to_dev(mr._mesh(np.zeros((0, 3)), [[0, 1, 2]]))
    with pytest.raises(ValueError, match="1 of 1 triangles"):
        geometry.mesh_adjacency(empty)


def test_argument_checks_on_the_device():
    dev = _to_dev(mr.soup(65, 100, seed=6))
    adj = geometry.mesh_adjacency(dev)
    other = geometry.mesh_adjacency(_to_dev(mr.soup(64, 100, seed=6)))
    for bad in (other, {}, dict(adj, offsets=adj["offsets"].int()), dict(adj, boundary=adj["boundary"].cpu()), 7):
        with pytest.raises((ValueError, RuntimeError)):
            geometry.smooth_mesh(dev, 1, adjacency=bad)
    for pinned in (torch.zeros(64, dtype=torch.bool, device=DEV), torch.zeros(65, dtype=torch.int32, device=DEV),
                   torch.zeros(65, dtype=torch.bool)):
        with pytest.raises((ValueError, RuntimeError)):
            geometry.smooth_mesh(dev, 1, pinned=pinned)
    with pytest.raises(ValueError):
        geometry.vertex_normals(dev, fallback=torch.zeros(64, 3, device=DEV))
    with pytest.raises(ValueError):
        geometry.smooth_mesh(dict(dev, triangles=dev["triangles"].long()))
    out = geometry.smooth_mesh(dict(dev, colors=dev["normals"].abs()), 2, normals=None)
    assert set(out) == {"vertices", "normals", "triangles", "colors"} and out["normals"] is dev["normals"]


def test_extract_mesh_smooths_before_simplifying_and_colouring():
    nerf_fl_amd.set_precision("f16x3")
    try:
        rendering.check_status(DEV)
    except FloatingPointError:
        pass
    model = NeRF("fine")
    model.load_state_dict(synth.make_field_params(12, "sharp", typ="fine"))
    model = model.to(DEV)
    emb = make_embeddings(10, False)
    lo, hi, res = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), (25, 25, 25)
    cell = 2.0 * 2.0 / 24
    with torch.no_grad():
        lattice = geometry.density_lattice(model, emb, lo, hi, res)
        iso = lattice.median().item()
        base = geometry.extract_surface(lattice, iso, lo, hi)
        assert base["vertices"].shape[0] > 0
        # without smooth=: what it did before, on the bits
        plain = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso)
        assert set(plain) == {"vertices", "normals", "triangles", "colors"}
        for k in ("vertices", "normals", "triangles"):
            _same(plain[k], _bits(base[k]), k)
        _same(plain["colors"], _bits(geometry.surface_colors(model, emb, base["vertices"], base["normals"])), "colors")
        # smooth=3: the steps taken by hand
        got = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, smooth=3)
        exp = geometry.smooth_mesh(base, 3)
        for k in ("vertices", "normals", "triangles"):
            _same(got[k], _bits(exp[k]), k)
        assert not torch.equal(got["vertices"], base["vertices"]) and not torch.equal(got["normals"], base["normals"])
        _same(got["colors"], _bits(geometry.surface_colors(model, emb, exp["vertices"], exp["normals"])), "colors")
        # clean -> smooth -> simplify, with the keywords passed on
        kw = dict(lam=0.4, mu=None, boundary="free", normals="uniform")
        got = geometry.extract_mesh({"fine": model}, emb, lo, hi, res, iso, largest=1, smooth=2, smooth_kwargs=kw, simplify=cell)
        exp = geometry.simplify_mesh(geometry.smooth_mesh(geometry.clean_mesh(base, largest=1), 2, **kw), cell, origin=lo)
        assert 0 < exp["vertices"].shape[0] < base["vertices"].shape[0]
        for k in ("vertices", "normals", "triangles"):
            _same(got[k], _bits(exp[k]), k)
        _same(got["colors"], _bits(geometry.surface_colors(model, emb, exp["vertices"], exp["normals"])), "colors")
    rendering.check_status(DEV)
