"""Direct parity of the HIP `nfl_sample_pdf` (C ABI) with the reference's sample_pdf + concat + sort
(models/rendering.py:7-46, 266-272) on the reference's edge cases: completely empty rays, runs of zero-weight
bins, a single spike, weight only in the two dropped columns, u = 0 / 1 / 1 - 2^-24, per-ray depth ranges,
jittered coarse depths.  Fixture: tests/golden/g3b_sample_pdf_coarse.npz, produced by the real reference.

What "equal" means here.  The kernel reproduces the reference's CPU arithmetic operation for operation (ATen's
fp32 summation order, its fp64-accumulated cumsum, separately rounded fp32 elsewhere; see nfl_sample.hip), so on
identical inputs every draw must be BIT-IDENTICAL to the fixture -- that is the assertion.  Beside it the test keeps
a weaker, implementation-independent rule (`_admissible_error`): an ulp in the normalising sum moves every cdf
entry by at most an ulp and a draw by  ulp(1) * (bin width) / (bin probability), and sample_pdf is piecewise -- bin
choice by searchsorted, `denom < eps -> 1` (rendering.py:33-42) -- so a draw within a few ulps of a breakpoint may
fall on either side.  That rule is what end-to-end comparisons can rely on when the coarse weights themselves
differ in their last bits (tests/golden_util.py: sampling_conditioning).

The fixture has one shape (S = 64, I = 64, R = 48).  The shape sweep at the end of this file takes the kernel through its
other branches -- the scalar-sum path, vector counts with and without left-over vectors and tails, the later passes of the
64-bin scan, a last block of three rays, S + I at the 512-entry limit, equal keys in the rank count -- on seeded inputs, bit
for bit against `_kernel_model`, whose sum is written out (`_row_sums`) and held equal to torch.sum and to the oracle on
the CPU, with both outputs inside guarded NaN arenas.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_util as gu

CDF_ULPS = 2.0
ULP1 = 2.0 ** -24
EPS = 1e-5


def _hip_sample(z, w, u, I):
    from nerf_fl_amd import _lib
    dev = "cuda:0"
    R, S = z.shape
    zd, wd = z.to(dev).contiguous(), w.to(dev).contiguous()
    z_fine = torch.empty(R, S + I, device=dev)
    smp = torch.empty(R, I, device=dev)
    if u is None:
        u_row, ud = torch.linspace(0, 1, I, device=dev), None
    else:
        u_row, ud = None, u.to(dev).contiguous()
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    _lib.check(_lib.lib().nfl_sample_pdf(p(zd), p(wd), p(ud), p(u_row), R, S, I, p(z_fine), p(smp),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_sample_pdf")
    torch.cuda.synchronize()
    return z_fine.cpu(), smp.cpu()


def _row_sums(ww, leftover_to=0):
    """fp32 row sums of the (R, M) float32 matrix `ww` in the order nfl_sample.hip adds them, written out so that the
    expectation does not follow the host's vector width as torch.sum's does: 8-lane vectors, vector i into accumulator
    i % 4 while whole groups of four last, the left-over vectors into accumulator 0, ((acc0 + acc1) + acc2) + acc3 lane by
    lane, then the scalar tail and after it the eight partials in order, all into one scalar.  Rows shorter than a vector
    (M < 8): four interleaved scalar accumulators, the tail into the first, ((a0 + a1) + a2) + a3.
    `leftover_to` != 0 is a deliberate defect (tests only)."""
    assert ww.dtype == np.float32
    R, M = ww.shape
    if M < 8:
        acc = np.zeros((R, 4), np.float32)
        nq = M >> 2
        for i in range(nq):
            acc += ww[:, 4 * i:4 * i + 4]
        for j in range(4 * nq, M):
            acc[:, 0] += ww[:, j]
        return ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    nv = M >> 3
    nfull = nv >> 2
    acc = np.zeros((R, 4, 8), np.float32)
    for i in range(nfull):
        for k in range(4):
            acc[:, k] += ww[:, 8 * (4 * i + k):8 * (4 * i + k) + 8]
    for i in range(4 * nfull, nv):
        acc[:, leftover_to] += ww[:, 8 * i:8 * i + 8]
    part = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    fin = np.zeros(R, np.float32)
    for j in range(8 * nv, M):
        fin += ww[:, j]
    for q in range(8):
        fin += part[:, q]
    assert fin.dtype == np.float32
    return fin


def _kernel_model(z, w, u, row_sums=_row_sums):
    """The arithmetic nfl_sample.hip performs, restated with numpy (the sum in ATen's CPU order, written out in _row_sums,
    the scan in fp64 rounded once per entry, everything else fp32 operation by operation).  Used on the CPU to
    check this file's acceptance rule without a GPU, and as the expectation of the shape sweep."""
    z, w, u = z.numpy(), w.numpy(), u.numpy()
    R, S = z.shape
    eps = np.float32(EPS)
    ww = (w[:, 1:-1] + eps).astype(np.float32)
    total = row_sums(ww)                                 # the kernel follows ATen's CPU summation order exactly
    pdf = (ww / total[:, None]).astype(np.float32)
    cdf = np.concatenate([np.zeros((R, 1), np.float32), np.cumsum(pdf.astype(np.float64), 1).astype(np.float32)], 1)
    mids = (np.float32(0.5) * (z[:, :-1] + z[:, 1:])).astype(np.float32)
    M = S - 2
    out = np.zeros_like(u)
    for r in range(R):
        lo = np.searchsorted(cdf[r], u[r], side="right")
        below, above = np.maximum(lo - 1, 0), np.minimum(lo, M)
        c0, c1, b0, b1 = cdf[r][below], cdf[r][above], mids[r][below], mids[r][above]
        den = (c1 - c0).astype(np.float32)
        den[den < eps] = 1
        out[r] = (b0 + ((u[r] - c0) / den).astype(np.float32) * (b1 - b0)).astype(np.float32)
    return torch.from_numpy(out)


def _admissible_error(z, w, u, smp):
    """For every draw: distance of `smp` to the nearest value the reference's algorithm can return when its cdf is
    perturbed by at most CDF_ULPS ulps, divided by that value's own error bound (<= 1 means accepted).
    sample_pdf is piecewise: a draw picks the bin with cdf[j] <= u < cdf[j+1] (searchsorted right=True, then the
    clamps of rendering.py:34-35), and a bin narrower than eps gets denominator 1 (rendering.py:41-42).  A draw within
    a few ulps of a breakpoint, or a bin within a few ulps of eps, may legitimately fall on either side; inside a
    branch the result moves by  delta * width / den  for a cdf error delta (plus the cancellation in den = c1 - c0)."""
    zz, ww = z.double(), (w[:, 1:-1] + EPS).double()
    mids = 0.5 * (zz[:, :-1] + zz[:, 1:])                                    # (R, M+1)
    pdf = ww / ww.sum(1, keepdim=True)
    cdf = torch.cat([torch.zeros_like(pdf[:, :1]), pdf.cumsum(1)], 1)         # (R, M+1)
    M = pdf.shape[1]
    ud, sd = u.double(), smp.double()
    delta = CDF_ULPS * ULP1
    j0 = (torch.searchsorted(cdf.contiguous(), ud.contiguous(), right=True) - 1).clamp(min=0)      # bin of the draw, 0..M
    best = torch.full_like(sd, float("inf"))
    for dj in (-1, 0, 1):
        j = (j0 + dj).clamp(0, M)
        top = j == M                                   # clamped: below = above = M, the sample is the last mid-point
        jn = (j + 1).clamp(max=M)
        c0, c1 = cdf.gather(1, j), cdf.gather(1, jn)
        b0, b1 = mids.gather(1, j), mids.gather(1, jn)
        reach = (ud >= c0 - delta) & ((ud <= c1 + delta) | top)
        den = c1 - c0
        for branch in ("keep", "one"):
            if branch == "keep":
                valid = reach & (den >= EPS - delta) & ~top
                d = den.clamp(min=EPS - delta)
            else:
                valid = reach & ((den < EPS + delta) | top)
                d = torch.ones_like(den)
            cand = b0 + (ud - c0) / d * (b1 - b0)
            # cdf error delta in (u - c0) and 2 * delta in den = c1 - c0 (|u - c0| <= den + delta), then fp32 rounding
            tol = 3 * delta * (b1 - b0).abs() / d + 8 * ULP1 * cand.abs() + 1e-7
            ratio = torch.where(valid, (sd - cand).abs() / tol, torch.full_like(sd, float("inf")))
            best = torch.minimum(best, ratio)
    return best


def _check(z, w, u, smp, exp, label, min_exact=1.0):
    ratio = _admissible_error(z, w, u, smp)
    exact = float((smp == exp).float().mean())
    print(f"sample_pdf[{label}]: {100 * exact:.2f}% of {smp.numel()} draws bit-identical to the reference, "
          f"worst |err| {(smp - exp).abs().max().item():.3e}, worst distance/bound {float(ratio.max()):.3f}")
    assert float(_admissible_error(z, w, u, exp).max()) <= 1.0, "the reference's own output must satisfy the rule"
    bad = (ratio > 1.0).nonzero()
    assert bad.numel() == 0, f"{bad.shape[0]} draws further than {CDF_ULPS} cdf-ulps from the reference, e.g. {bad[:4].tolist()}"
    assert exact >= min_exact, "the kernel follows the reference's CPU arithmetic: the draws must be bit-identical"


def _inputs(mode):
    cfg, a = gu.load("g3b_sample_pdf_coarse")
    I = cfg["n_importance"]
    z, w = a["z_coarse"], a["weights_coarse"]
    u = torch.linspace(0, 1, I).expand(z.shape[0], I).contiguous() if mode == "det" else a["u"]
    return a, I, z, w, u


@pytest.mark.parametrize("mode", ["det", "rnd"])
def test_acceptance_rule_on_kernel_model_cpu(mode):
    """No GPU: the numpy restatement of the kernel's arithmetic passes the same rule the GPU test applies (keeps the
    rule itself honest, and pins what the kernel is meant to compute)."""
    a, I, z, w, u = _inputs(mode)
    _check(z, w, u, _kernel_model(z, w, u), a[mode], "model/" + mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["det", "rnd"])
def test_sample_pdf_edge_cases(mode):
    a, I, z, w, u = _inputs(mode)
    z_fine, smp = _hip_sample(z, w, None if mode == "det" else u, I)
    _check(z, w, u, smp, a[mode], mode)
    model = _kernel_model(z, w, u)
    print(f"   vs the numpy model of the kernel: {100 * float((smp == model).float().mean()):.2f}% bit-identical")
    # concat + sort (rendering.py:272): exactly the sorted multiset of the coarse depths and the kernel's own draws
    assert torch.equal(z_fine, torch.sort(torch.cat([z, smp], 1), 1)[0])
    # rows all of whose draws are bit-identical must give the reference's merged row bit for bit
    same = (smp == a[mode]).all(1)
    assert same.sum() >= 24
    assert torch.equal(z_fine[same], a[f"z_fine_{mode}"][same])


@pytest.mark.gpu
def test_sample_pdf_empty_rays_are_uniform():
    """Rays without any interior weight (rows 8..11 and 16..19 of the fixture): the pdf is uniform, so the
    deterministic draws run evenly from the first to the last mid-point -- a closed form to hold the kernel to."""
    a, I, z, w, u = _inputs("det")
    _, smp = _hip_sample(z, w, None, I)
    for r in list(range(8, 12)) + list(range(16, 20)):
        mids = 0.5 * (z[r, :-1] + z[r, 1:])
        lin = mids[0] + (mids[-1] - mids[0]) * torch.linspace(0, 1, I)
        assert (smp[r] - lin).abs().max().item() <= 2e-5


# ---- the shape sweep: every branch of the kernel, bit for bit ---------------------------------------------------------------
# S: M = S - 2 interior weights.  3, 4, 9: the scalar-sum path (M = 1, 2, 7; 9 with a tail after one group of four); 10: one
# vector, no tail; 34: four vectors (a multiple of four: no left-over vectors), no tail; 41, 42: left-over vector with and
# without a tail; 66: the scan's single pass filled (M = 64); 67: its second pass (M = 65); 131, 258: three and four passes
# (M = 256: 32 vectors, no left-over, no tail).  I = 65, 200: more draws than lanes.  S + I = 512: the LDS limit.
SWEEP_S = (3, 4, 9, 10, 34, 41, 42, 66, 67, 131, 258)
SWEEP_I = (1, 5, 64, 65, 200)
SWEEP = [(S, I) for S in SWEEP_S for I in SWEEP_I if S + I <= 512] + [(258, 254)]
SWEEP_R = 7               # two blocks of four waves: the last has three rays
SPECIAL_U = (0.0, 1.0, 1.0 - 2.0 ** -24)


def _sweep_inputs(S, I):
    """Seeded: jittered, sorted depths; rows 0, 1, 3, 6 random^8 weights, row 2 and row 4 all zero, row 5 a single spike;
    per-ray u with 0, 1 and 1 - 2^-24 in every row (I < 3: one of them per row), and a shared row of u with the same."""
    gen = torch.Generator().manual_seed(1000 * S + I)
    R = SWEEP_R
    step = 4.0 / (S - 1)
    z = torch.sort(torch.linspace(2, 6, S)[None, :] + (torch.rand(R, S, generator=gen) - 0.5) * step, 1)[0].contiguous()
    w = torch.rand(R, S, generator=gen) ** 8
    w[2] = 0
    w[4] = 0
    w[5] = 0
    w[5, 1 + int(torch.randint(0, S - 2, (1,), generator=gen))] = 0.7
    special = torch.tensor(SPECIAL_U, dtype=torch.float32)
    u = torch.rand(R, I, generator=gen)
    u_row = torch.rand(I, generator=gen)
    for r in range(R):
        pos = torch.randperm(I, generator=gen)[:3]
        u[r, pos] = special.roll(r)[:len(pos)]
    pos = torch.randperm(I, generator=gen)[:3]
    u_row[pos] = special.roll(S)[:len(pos)]
    assert float(u.max()) <= 1.0 and float(u_row.max()) <= 1.0
    return z, w, u, u_row


def _tie_inputs():
    """Draws that coincide with coarse depths: no interior weight, so the pdf is uniform, and u on the model's own cdf
    grid, so every draw is a bin mid-point, b0 + 0 / den * (b1 - b0), each value drawn twice; in every ray two neighbouring
    coarse depths are equal, hence equal to their mid-point, which is drawn too: three and four equal keys for the rank
    count to order."""
    S = 12
    gen = torch.Generator().manual_seed(77)
    z = torch.sort(2 + 4 * torch.rand(SWEEP_R, S, generator=gen), 1)[0]
    for r in range(SWEEP_R):
        j = 1 + r % (S - 2)
        z[r, j + 1] = z[r, j]
    w = torch.zeros(SWEEP_R, S)
    ww = np.full((SWEEP_R, S - 2), np.float32(EPS), np.float32)
    pdf = (ww / _row_sums(ww)[:, None]).astype(np.float32)
    cdf = np.concatenate([np.zeros((SWEEP_R, 1), np.float32), np.cumsum(pdf.astype(np.float64), 1).astype(np.float32)], 1)
    u = torch.from_numpy(np.concatenate([cdf, cdf], 1)).contiguous()                   # (R, 2 (S - 1))
    return z.contiguous(), w, u


def _oracle(z, w, u):
    from oracle import nerfw_oracle as orc
    return orc.sample_pdf(0.5 * (z[:, :-1] + z[:, 1:]), w[:, 1:-1], u)


def _torch_sums(ww):
    return torch.from_numpy(ww).sum(1).numpy()


def test_explicit_sum_order_is_torch_sum_and_the_oracle_cpu():
    """No GPU; a guard for other hosts.  Over the whole sweep (and the tie case) the model with the sum written out gives
    the draws of the model with torch.sum and of oracle.sample_pdf, bit for bit, on the per-ray u and on the shared row;
    the oracle's draws satisfy the acceptance rule.  The written-out sum with the left-over vectors added into the wrong
    accumulator does not give the oracle's draws at S = 42 (M = 40: five vectors, one left over)."""
    cases = [(f"S={S} I={I}", z, w, uu) for S, I in SWEEP for z, w, u, u_row in [_sweep_inputs(S, I)]
             for uu in (u, u_row.expand(SWEEP_R, I).contiguous())]
    cases.append(("ties",) + _tie_inputs())
    n = differ = 0
    for label, z, w, u in cases:
        model, ora = _kernel_model(z, w, u), _oracle(z, w, u)
        d = int((model != ora).sum()) + int((model != _kernel_model(z, w, u, _torch_sums)).sum())
        if d:
            print(f"sample_pdf model[{label}]: {d} differences")
        differ += d
        n += model.numel()
        assert bool(torch.isfinite(model).all())
        assert float(_admissible_error(z, w, u, ora).max()) <= 1.0, label
    print(f"sample_pdf model: {n} draws, {differ} differences between the explicit model, torch.sum and the oracle")
    assert n == 2 * SWEEP_R * sum(I for _, I in SWEEP) + SWEEP_R * 22 and differ == 0
    z, w, u, _ = _sweep_inputs(42, 200)
    wrong = _kernel_model(z, w, u, lambda ww: _row_sums(ww, leftover_to=1))
    assert int((wrong != _oracle(z, w, u)).sum()) > 0
    # the tie case is what it says: every draw a mid-point, each coarse pair equal to one
    z, w, u = _tie_inputs()
    smp = _kernel_model(z, w, u)
    mids = 0.5 * (z[:, :-1] + z[:, 1:])
    assert torch.equal(smp, torch.cat([mids, mids], 1))
    keys = torch.cat([z, smp], 1)
    assert all(int((keys[r] == z[r, 1 + r % 10]).sum()) == 4 for r in range(SWEEP_R))


def _hip_sample_guarded(z, w, u, u_row, I, want_samples=True):
    """nfl_sample_pdf with z_fine and samples inside NaN-filled arenas (forward_ref.Arena).  Returns (z_fine, samples or None,
    complaints about guards and left-over NaN)."""
    import forward_ref as fr
    from nerf_fl_amd import _lib
    dev = "cuda:0"
    R, S = z.shape
    on = lambda t: None if t is None else t.to(dev).contiguous()
    zd, wd, ud, rd = on(z), on(w), on(u), on(u_row)
    arenas = {"z_fine": fr.Arena((R, S + I), dev)}
    if want_samples:
        arenas["samples"] = fr.Arena((R, I), dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    _lib.check(_lib.lib().nfl_sample_pdf(p(zd), p(wd), p(ud), p(rd), R, S, I, p(arenas["z_fine"].t),
                                         p(arenas["samples"].t) if want_samples else C.c_void_p(0),
                                         C.c_void_p(torch.cuda.current_stream().cuda_stream)), "nfl_sample_pdf")
    torch.cuda.synchronize()
    bad = [f"wrote outside {k}" for k, a in arenas.items() if not a.guards_ok()]
    bad += [f"NaN left in {k}" for k, a in arenas.items() if bool(torch.isnan(a.t).any())]
    return arenas["z_fine"].t.cpu(), arenas["samples"].t.cpu() if want_samples else None, bad


def _sweep_check(label, z, w, u, z_fine, smp, bad):
    """Every draw bit-identical to the explicit model, z_fine the sorted row of coarse depths and draws, the weaker rule too."""
    model = _kernel_model(z, w, u)
    out = [f"{label}: {b}" for b in bad]
    if smp is not None:
        differ = smp.view(torch.int32) != model.view(torch.int32)
        if bool(differ.any()):
            r, i = differ.nonzero()[0].tolist()
            out.append(f"{label}: {int(differ.sum())} of {smp.numel()} draws differ from the model, first ray {r} draw {i}: "
                       f"{smp[r, i].item()!r} against {model[r, i].item()!r} (u = {u[r, i].item()!r})")
        worst = float(_admissible_error(z, w, u, smp).max())
        if not worst <= 1.0:
            out.append(f"{label}: a draw is {worst:.3f} of the admissible error")
    if not torch.equal(z_fine, torch.sort(torch.cat([z, model], 1), 1)[0]):
        out.append(f"{label}: z_fine is not the sorted row of the coarse depths and the draws")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("S", sorted({S for S, _ in SWEEP}))
def test_sample_pdf_shape_sweep(S):
    """Every (S, I) of the sweep with this S (see SWEEP_S for the branch each S takes), R = 7, through d_u and through
    d_u_row, with d_samples null once per S: every draw bit-identical to the explicit model (which the CPU test above holds
    equal to the oracle), z_fine equal to torch.sort of the coarse depths and the draws, `_admissible_error` <= 1, the
    guards of both buffers intact and no NaN left in either."""
    bad = []
    for I in [I for s, I in SWEEP if s == S]:
        z, w, u, u_row = _sweep_inputs(S, I)
        bad += _sweep_check(f"S={S} I={I} d_u", z, w, u, *_hip_sample_guarded(z, w, u, None, I))
        wide = u_row.expand(SWEEP_R, I).contiguous()
        bad += _sweep_check(f"S={S} I={I} d_u_row", z, w, wide, *_hip_sample_guarded(z, w, None, u_row, I))
    bad += _sweep_check(f"S={S} I={I} d_u, d_samples null", z, w, u, *_hip_sample_guarded(z, w, u, None, I, want_samples=False))
    assert not bad, "\n".join(bad)


@pytest.mark.gpu
def test_sample_pdf_orders_equal_keys():
    """The tie case (_tie_inputs): coarse depths equal to each other and to draws, draws equal to each other.  The rank count
    must give every key a place of its own: a tie broken the same way twice leaves a NaN of the arena in z_fine."""
    z, w, u = _tie_inputs()
    bad = _sweep_check("ties", z, w, u, *_hip_sample_guarded(z, w, u, None, u.shape[1]))
    assert not bad, "\n".join(bad)
