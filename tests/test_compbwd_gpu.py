"""nfl_composite_backward on its own, against float64 autograd through the oracle's compositing (tests/compbwd_ref.py)."""
import functools

import pytest
import torch

import compbwd_ref as cr

pytestmark = pytest.mark.gpu

SENT = -12345.5          # whatever the call does not own must still hold it afterwards
GUARD = 64               # floats before and behind the head gradient
JUNK = 7.0e30            # what d_gmax holds before the call

ALL = cr.UP_NAMES
FUSED = ("rgb", "beta")  # the fused loss leaves seeds for rgb and beta only; go is a device scalar, g_tsig_const != 0

# (R, N, transient, noise, white_back, upstream gradients present, fused-loss scalars)
CASES = []
# every N with everything present: the block carries of both scans (63, 64, 65, 129) and NFL_CB_MAXN; R = 5 leaves three of
# the last workgroup's four waves without a ray
for i, n in enumerate([1, 2, 63, 64, 65, 129, 1024]):
    CASES += [(5, n, True, False, i % 2 == 0, ALL, False), (5, n, False, True, i % 2 == 1, ALL, False)]
# R = 1 and a full workgroup pair, noise off
CASES += [(1, 65, True, False, False, ALL, False), (1, 65, False, False, True, ALL, False),
          (8, 65, True, False, True, ALL, False), (8, 65, False, False, False, ALL, False)]
# each pointer alone (the other seven NULL)
CASES += [(5, 65, True, False, True, (name,), False) for name in ALL]
CASES += [(5, 65, False, True, True, (name,), False) for name in ALL[:4]]
# the fused-loss pattern
CASES += [(5, 129, True, False, True, FUSED, True), (5, 129, False, True, False, ("rgb",), True)]


def case_id(c):
    R, N, tr, noisy, white, present, fused = c
    what = "all" if present == ALL else "fused" if fused else "only_" + present[0]
    return f"R{R}-N{N}-{'transient' if tr else 'static'}{'-noise' if noisy else ''}{'-white' if white else ''}-{what}"


@functools.lru_cache(maxsize=None)
def inputs(R, N, tr, noisy):
    return cr.draw_inputs(R, N, tr, noisy, seed=7 * R + N + 2 * tr + noisy)


def run(f, z, noise, R, N, tr, white, grads, go, g_tsig_const, n_rays=None):
    """The call with `head` inside a sentinel-filled buffer and d_gmax pre-filled with junk.  Returns (head, gmax) on the CPU
    after checking that nothing but the head gradient's R N 9 floats was written."""
    import gpu_util
    from nerf_fl_amd import _lib, rendering as rnd
    dev = gpu_util.DEV
    n = R * N * 9
    buf = torch.full((2 * GUARD + n,), SENT, dtype=torch.float32, device=dev)
    head = buf[GUARD:GUARD + n].view(R * N, 9)
    gmax = torch.full((_lib.NFL_GMAX_SLOTS,), JUNK, dtype=torch.float32, device=dev)
    on = lambda t: None if t is None else t.to(dev)
    rnd._run_compbwd(on(f), on(z), R if n_rays is None else n_rays, N, noise=on(noise), noise_std=1.0 if noise is not None else 0.0,
                     use_t=tr, white_back=white, grads=[on(g) for g in grads],
                     go=None if go is None else torch.tensor(go, dtype=torch.float32, device=dev), g_tsig_const=g_tsig_const,
                     head=head, gmax=gmax)
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == SENT).all()) and bool((host[GUARD + n:] == SENT).all()), "written outside the head gradient"
    return host[GUARD:GUARD + n].view(R * N, 9).clone(), gmax.cpu()


@pytest.mark.parametrize("case", CASES, ids=[case_id(c) for c in CASES])
def test_head_gradient_against_float64_autograd(case):
    """Every element of the (R N, 9) head gradient within
        |got - ref| <= 2^-24 E + floor
    of float64 autograd.  E (compbwd_ref.error_units) is the issue's  c(N) * magnitude  with the count applied term by term,
    not as one constant: a first-order sum over the terms of the derivative, in each of which one factor is replaced by its
    error and the others keep their true absolute values; the j-fold count falls on the transmittance only where T enters,
    the 8 + N / 64 additions of the suffix scan only on the suffix.  It departs from the issue's magnitude
    delta act' (T_{i+1} |g_i| + sum_{j>i} |w_j g_j|) in one respect, which the kernel's (and the reference's) formulation
    forces: alpha = 1 - expf(..) and each factor 1 - alpha_k of T carry an ABSOLUTE error of about 3 u and 5 u, so a thin
    sample's weight (alpha ~ 1e-4) is known to 3e4 u of its value and T behind a saturated sample to u T_k.  Where alpha is
    resolved the bound is 2 .. 3 (N + 40) u of a colour gradient and about 20 (N + 40) u of a density gradient, whose two
    halves partly cancel (tests/test_backward_refs_cpu.py); on thin samples it exceeds the issue's magnitude by up to 3 / alpha.
    floor = 2^-109 of the ray's summed |upstream gradient|: fp32 underflow where float64 still has e^-200.
    Largest |error| / bound as measured on the MI355X (printed per case), everything present, R = 5:
        N            1      2      63     64     65     129    1024
        transient    0.24   0.25   0.36   0.32   0.33   0.44   0.33
        static+noise 0.13   0.19   0.16   0.34   0.29   0.48   0.16
    R = 1 and 8 at N = 65: 0.13 .. 0.43; one upstream pointer alone: 0.05 (depth) .. 0.29; fused-loss pattern: 0.50
    transient, 0.48 static.  The worst elements are colour gradients of thin samples and sigma_t: a few roundings of one sign
    out of the handful the bound counts there.

    Also: channels 4..8 and gated densities exactly 0; nothing written outside `head`; no NaN or Inf on the saturated rays;
    d_gmax (pre-filled with junk: the zeroing kernel must have run) holds in slot r the maximum of ray r, bit for bit,
    and zero in the slots of rays that do not exist."""
    R, N, tr, noisy, white, present, fused = case
    f, z, noise = inputs(R, N, tr, noisy)
    grads = cr.draw_upstream(R, N, tr, present, seed=N + len(present))
    go, gts = (0.37, 1e-3 if tr else 0.0) if fused else (None, 0.0)
    kw = dict(noise=noise, noise_std=1.0 if noisy else 0.0, use_t=tr, white_back=white, grads=grads, go=go, g_tsig_const=gts)
    ref = cr.reference(f, z, **kw)
    E, floor = cr.error_units(f, z, **kw)
    assert float(ref.abs().max()) > 0, "the case tests nothing"

    head, gmax = run(f, z, noise, R, N, tr, white, grads, go, gts)
    assert bool(torch.isfinite(head).all()), "NaN or Inf in the head gradient"
    ratio = cr.error_ratio(head, ref, E, floor)
    worst, where = cr.worst(ratio, N)
    print(f"compbwd {case_id(case)}: largest |error| / bound = {worst:.3e} at {where}")
    assert worst <= 1.0, f"{where}: got {head.flatten()[int(ratio.argmax())].item()!r}, float64 {ref.flatten()[int(ratio.argmax())].item()!r}, {worst:.3g} of the bound"
    if not tr:
        assert not head[:, 4:].any(), "a transient channel of a static pass is not zero"
        pre = f[:, 3] + (noise.flatten() if noisy else 0.0)
        assert not head[:, 3][pre <= 0].any(), "a density at or below zero after its noise has a gradient"

    per_ray = head.abs().view(R, N * 9).max(1)[0]
    assert bool((gmax >= 0).all()) and torch.equal(gmax[:R].view(torch.int32), per_ray.view(torch.int32)), (gmax[:R], per_ray)
    assert not gmax[R:].any(), "a slot of a ray that does not exist is not zero"
    assert torch.equal(gmax.max().view(torch.int32), head.abs().max().view(torch.int32))


def test_gmax_zeroed_without_rays():
    """n_rays = 0: nothing to do but to zero d_gmax; the head gradient is not touched."""
    f, z, _ = inputs(1, 2, True, False)
    head, gmax = run(f, z, None, 1, 2, True, True, cr.draw_upstream(1, 2, True, ALL, 1), None, 0.0, n_rays=0)
    assert not gmax.any() and bool((head == SENT).all())
