"""float64 references for nfl_composite_backward: the head gradient by autograd through the oracle's compositing, and a
first-order bound on what an fp32 evaluation of it may differ by.  A plain helper (no pytest hooks), CPU only.

The kernel's input `field_raw` holds the ACTIVATED head outputs [rgb, sigma, rgb_t, sigma_t, beta] (include/nerf_fl_amd.h);
its output is the gradient w.r.t. the PRE-activations.  `reference` inverts the activations in float64 (logit for the colours,
softplus^-1 for sigma, sigma_t and beta), makes the pre-activations leaves, applies the activations again -- snapping each
value back onto the fp32 input it came from, so that the forward sees exactly the numbers the kernel read and a density
that cancels its noise exactly is an exact zero of the relu here as well -- and differentiates
    go * ( sum_k <output_k, upstream_k>  +  g_tsig_const * sum sigma_t )
through oracle.nerfw_oracle.composite.

`closed_form` is the same derivative written out (the formulas of the header comment of csrc/nfl_compbwd.hip, from
SURVEY.md 8 A9); tests/test_backward_refs_cpu.py holds it to autograd.

`error_units` is the bound, in units of u = 2^-24: |got - ref| <= u E + floor.  It is the issue's  c(N) * magnitude  with the
count applied TERM BY TERM instead of once: E is a sum over the terms of the derivative, each term a product in which ONE
factor is replaced by its error and the others keep their true absolute values (first order), and every operation's
rounding is charged to the value it produces.  The factors' errors, with x = delta * density, e = exp(-x), alpha = 1 - e:

  de      = e (3 x + 3)            product delta * density and the sum of two densities (u x each, amplified by the exponent),
                                   the exponential's own argument scaling (u x) and result (one ulp = 2 u), one to spare
  dalpha  = de + alpha             alpha = 1 - e inherits the ABSOLUTE error of e: a thin sample's alpha ~ 1e-4 is known to
                                   3 u, not to u alpha -- the reference's own formulation, which the kernel follows
  d(1 - alpha) = dalpha + e
  dT_j    = sum_{k<j} d(1 - alpha_k) T_j / e_k + (8 + j / 64) T_j
                                   the transmittance is a product of the factors 1 - alpha_k: each hands on its absolute error
                                   (after a saturated sample k, e_k ~ e^-50, T_j is known to u T_k only), and the product
                                   itself is a 64-wide scan of depth 6 plus one carry per block
  dg      = 6 sum|terms|           the upstream gradient of a weight (go * p, gD * z, the white-background sum, three additions)
  d(1 - c) = 1 - c,   d(1 - exp(-sigma)) = 2 exp(-sigma) + (1 - exp(-sigma))
  suffix  = sum_{j>i} dH_j + (8 + N / 64) sum_{j>=i} |H_j|
                                   the terms' own errors, then the additions: a 64-wide scan of depth 6, one carry per block,
                                   minus the own term, plus the carry

`floor` covers what underflows in fp32.  A factor 1.01 covers the second-order terms (N u < 1e-4).
"""
import math

import torch

from oracle import nerfw_oracle as orc

U = 2.0 ** -24
UP_NAMES = ("weights", "opacity", "rgb", "depth", "transient_sigmas", "beta", "rgb_static", "rgb_transient")


def _sp_inv(y):
    return y + torch.log(-torch.expm1(-y))


def _as64(t):
    return None if t is None else t.detach().double().cpu()


def reference(field_raw, z, *, noise, noise_std, use_t, white_back, grads, go, g_tsig_const, beta_min=0.1):
    """(R N, 9) float64 head gradient.  `grads`: the eight upstream gradients in UP_NAMES order, tensors or None; `go`: a
    number or None."""
    R, N = z.shape
    f = _as64(field_raw).view(R, N, 9)
    z = _as64(z)
    # not torch's softplus: above its threshold of 20 that one is the identity, with derivative 1 where sigmoid(20) = 1 - 2e-9
    sp = lambda x: torch.clamp(x, min=0) + torch.log1p(torch.exp(-x.abs()))
    leaves = [torch.logit(f[..., 0:3]), _sp_inv(f[..., 3]), torch.logit(f[..., 4:7]), _sp_inv(f[..., 7]), _sp_inv(f[..., 8])]
    leaves = [x.clone().requires_grad_(True) for x in leaves]
    acts = [torch.sigmoid, sp, torch.sigmoid, sp, sp]
    vals = [f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7], f[..., 8]]
    rgb, sig, rgb_t, sig_t, beta = [a(x) + (v - a(x)).detach() for a, x, v in zip(acts, leaves, vals)]
    fd = {"sigma": sig, "rgb": rgb}
    if use_t:
        fd.update(sigma_t=sig_t, rgb_t=rgb_t, beta=beta)
    typ = "fine" if use_t else "coarse"
    nz = torch.zeros(R, N, dtype=torch.float64) if noise is None else _as64(noise)
    res = orc.composite(typ, z, fd, noise=nz, noise_std=float(noise_std), white_back=bool(white_back), test_time=False,
                        beta_min=beta_min)
    keys = [f"weights_{typ}", f"opacity_{typ}", f"rgb_{typ}", f"depth_{typ}", "transient_sigmas", "beta", "_rgb_fine_static",
            "_rgb_fine_transient"]
    total = torch.zeros((), dtype=torch.float64)
    for k, g in zip(keys, grads):
        if g is not None and k in res:
            total = total + (res[k] * _as64(g).view_as(res[k])).sum()
    if use_t:
        total = total + float(g_tsig_const) * sig_t.sum()
    total = total * (1.0 if go is None else float(go))
    if total.requires_grad:
        total.backward()
    cols = [x.grad if x.grad is not None else torch.zeros_like(x) for x in leaves]
    return torch.cat([cols[0], cols[1][..., None], cols[2], cols[3][..., None], cols[4][..., None]], -1).reshape(R * N, 9)


def _zero(*shape):
    return torch.zeros(*shape, dtype=torch.float64)


def _pieces(field_raw, z, noise, noise_std, use_t, white_back, grads, go, g_tsig_const, last_delta=1e2):
    """The true (float64) quantities both the derivative and its bound are built from.  Every upstream sum comes twice:
    signed, and as the sum of the absolute values of its terms (suffix `_abs`)."""
    R, N = z.shape
    p = {"R": R, "N": N}
    f = _as64(field_raw).view(R, N, 9)
    z = _as64(z)
    s = 1.0 if go is None else float(go)
    up = [None if g is None else s * _as64(g) for g in grads]
    get = lambda k, *shape: up[k].view(*shape) if up[k] is not None and (use_t or k < 4) else _zero(*shape)
    gw, gW, gC, gD = get(0, R, N), get(1, R, 1), get(2, R, 1, 3), get(3, R, 1)
    p["garr"], p["gB"] = get(4, R, N), get(5, R, 1)
    p["gCs"], p["gCs_abs"] = gC + get(6, R, 1, 3), gC.abs() + get(6, R, 1, 3).abs()
    p["gCt"], p["gCt_abs"] = gC + get(7, R, 1, 3), gC.abs() + get(7, R, 1, 3).abs()
    p["gts"] = s * float(g_tsig_const) if use_t else 0.0
    white = 1.0 if white_back else 0.0
    p["g"] = gw + gW + gD * z - white * p["gCs"].sum(-1)
    p["g_abs"] = gw.abs() + gW.abs() + (gD * z).abs() + white * p["gCs_abs"].sum(-1)
    p["delta"] = torch.cat([z[:, 1:] - z[:, :-1], torch.full((R, 1), last_delta, dtype=torch.float64)], 1)
    p["rgb"], p["sig"], p["rgb_t"], p["sig_t"], p["beta"] = f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7], f[..., 8]
    if use_t:
        p["dens"], p["gate"] = p["sig"] + p["sig_t"], torch.ones(R, N, dtype=torch.float64)
    else:
        pre = p["sig"] + (0.0 if noise is None else _as64(noise) * float(noise_std))
        p["dens"], p["gate"] = torch.relu(pre), (pre > 0).double()
    p["x"] = p["delta"] * p["dens"]
    p["e"] = torch.exp(-p["x"])
    p["T"] = torch.cat([torch.ones(R, 1, dtype=torch.float64), torch.cumprod(p["e"], 1)[:, :-1]], 1)
    p["G"] = (gw.abs().sum(1, keepdim=True) + gW.abs() + gD.abs() * z.abs().max(1, keepdim=True)[0] + p["gCs_abs"].sum(-1)
              + p["gCt_abs"].sum(-1) + p["gB"].abs() + p["garr"].abs().sum(1, keepdim=True) + abs(p["gts"]) * N)
    return p


def _suffix(H, inclusive, block=None):
    """sum over j > i (j >= i when inclusive) along the samples; `block`: starting again at every block of that many."""
    R, N = H.shape
    if block is None:
        inc = torch.flip(torch.cumsum(torch.flip(H, [1]), 1), [1])
    else:
        nb = (N + block - 1) // block
        Hp = torch.cat([H, _zero(R, nb * block - N)], 1).view(R, nb, block)
        inc = torch.flip(torch.cumsum(torch.flip(Hp, [2]), 2), [2]).reshape(R, nb * block)[:, :N]
    return inc if inclusive else inc - H


def closed_form(field_raw, z, *, noise, noise_std, use_t, white_back, grads, go, g_tsig_const, defect=None):
    """The derivative written out: (R N, 9) float64.  `defect` (tests/test_backward_refs_cpu.py): one deliberate mistake,
    "T_i" (T_i where T_{i+1} belongs), "suffix64" (the suffix sum starts again at every 64-sample block) or "last_delta"
    (the last interval 1e10 instead of 1e2) -- what the comparison must be able to reject."""
    p = _pieces(field_raw, z, noise, noise_std, use_t, white_back, grads, go, g_tsig_const,
                last_delta=1e10 if defect == "last_delta" else 1e2)
    R, N, T, delta, g = p["R"], p["N"], p["T"], p["delta"], p["g"]
    ex = (lambda x: torch.ones_like(x)) if defect == "T_i" else (lambda x: torch.exp(-x))     # the factor that makes T_{i+1} of T_i
    after = lambda H: _suffix(H, False, 64 if defect == "suffix64" else None)
    dact = lambda v: 1 - torch.exp(-v)                                        # softplus'(x) = 1 - exp(-softplus(x))
    out = _zero(R, N, 9)
    al = 1 - p["e"]
    if use_t:
        a_s, a_t = 1 - torch.exp(-delta * p["sig"]), 1 - torch.exp(-delta * p["sig_t"])
        gs = (p["gCs"] * p["rgb"]).sum(-1)
        gt = (p["gCt"] * p["rgb_t"]).sum(-1) + p["gB"] * p["beta"]
        ws, wt, w = a_s * T, a_t * T, al * T
        common = ex(p["x"]) * T * g - after(ws * gs + wt * gt + w * g)
        dss = delta * (ex(delta * p["sig"]) * T * gs + common)
        dst = delta * (ex(delta * p["sig_t"]) * T * gt + common) + p["gts"] + p["garr"]
        out[..., 0:3] = ws[..., None] * p["gCs"] * p["rgb"] * (1 - p["rgb"])
        out[..., 3] = dss * dact(p["sig"])
        out[..., 4:7] = wt[..., None] * p["gCt"] * p["rgb_t"] * (1 - p["rgb_t"])
        out[..., 7] = dst * dact(p["sig_t"])
        out[..., 8] = wt * p["gB"] * dact(p["beta"])
    else:
        gg = g + (p["gCs"] * p["rgb"]).sum(-1)
        w = al * T
        ds = p["gate"] * delta * (ex(p["x"]) * T * gg - after(w * gg))
        out[..., 0:3] = w[..., None] * p["gCs"] * p["rgb"] * (1 - p["rgb"])
        out[..., 3] = ds * dact(p["sig"])
    return out.reshape(R * N, 9)


def error_units(field_raw, z, *, noise, noise_std, use_t, white_back, grads, go, g_tsig_const):
    """(E (R N, 9), floor (R N, 1)): |fp32 result - float64 derivative| <= u E + floor, first order, as derived in the
    module's docstring.  floor: an fp32 intermediate that underflows is wrong by at most 2^-126 (flushed or subnormal) where
    float64 still holds e^-200; it reaches an element through delta <= 100 < 2^7, at most 2^10 terms of a suffix and a
    factor <= the ray's summed |upstream gradient| G, so 2^-109 G."""
    p = _pieces(field_raw, z, noise, noise_std, use_t, white_back, grads, go, g_tsig_const)
    R, N, T, delta, e = p["R"], p["N"], p["T"], p["delta"], p["e"]
    n_sum = 8 + math.ceil(N / 64)

    def exp_parts(x):
        """e, de, alpha, dalpha of one exponent."""
        ex = torch.exp(-x)
        de = ex * (3 * x + 3)
        return ex, de, 1 - ex, de + (1 - ex)

    ec, dec, al, dal = exp_parts(p["x"])
    dom = dal + ec
    Q = _zero(R, N)                                        # sum_{k<j} d(1 - alpha_k) T_j / e_k, by its recurrence
    q = _zero(R)
    for j in range(N):
        Q[:, j] = q
        q = q * e[:, j] + T[:, j] * dom[:, j]
    dT = Q + (8 + torch.arange(N, dtype=torch.float64) // 64) * T
    dT[:, 0] = 0.0                                         # T_0 = 1 is exact

    weight = lambda a, da: (a * T, da * T + a * dT + a * T)                                       # w = alpha T and its error
    lead = lambda ex, dex, gx, dgx: (ex * T * gx, (dex * T + ex * dT) * gx.abs() + ex * T * dgx + 2 * (ex * T * gx).abs())
    da_of = lambda v: 2 * torch.exp(-v) + (1 - torch.exp(-v))                                     # d(1 - exp(-v))
    dact = lambda v: 1 - torch.exp(-v)

    def colours(w, dw, G, G_abs, c):
        """error of w G c (1 - c): the weight's, then go * p and the sum of two upstream terms, 1 - c, three products."""
        return (dw[..., None] * G.abs() + 6 * w[..., None] * G_abs) * c * (1 - c)

    g, dg = p["g"], 6 * p["g_abs"]
    E = _zero(R, N, 9)
    if use_t:
        es, des, a_s, da_s = exp_parts(delta * p["sig"])
        et, det, a_t, da_t = exp_parts(delta * p["sig_t"])
        gs, dgs = (p["gCs"] * p["rgb"]).sum(-1), 5 * (p["gCs_abs"] * p["rgb"]).sum(-1)
        gt = (p["gCt"] * p["rgb_t"]).sum(-1) + p["gB"] * p["beta"]
        dgt = 6 * ((p["gCt_abs"] * p["rgb_t"]).sum(-1) + (p["gB"] * p["beta"]).abs())
        (ws, dws), (wt, dwt), (w, dw) = weight(a_s, da_s), weight(a_t, da_t), weight(al, dal)
        terms = [(ws, dws, gs, dgs), (wt, dwt, gt, dgt), (w, dw, g, dg)]
        H_abs = sum((wx * gx).abs() for wx, _, gx, _ in terms)
        dH = sum(dwx * gx.abs() + wx * dgx + (wx * gx).abs() for wx, dwx, gx, dgx in terms) + 2 * H_abs
        dafter = _suffix(dH, False) + n_sum * _suffix(H_abs, True)
        H = sum(wx * gx for wx, _, gx, _ in terms)
        Ac, dAc = lead(ec, dec, g, dg)
        common = Ac - _suffix(H, False)
        dcommon = dAc + dafter + common.abs()
        for ch, (ex, dex, gx, dgx, sg, extra, dextra) in ((3, (es, des, gs, dgs, p["sig"], 0.0, 0.0)),
                                                          (7, (et, det, gt, dgt, p["sig_t"], p["gts"] + p["garr"],
                                                               abs(p["gts"]) + p["garr"].abs()))):
            Ax, dAx = lead(ex, dex, gx, dgx)
            inner = Ax + common
            dinner = dAx + dcommon + inner.abs()
            val = delta * inner + extra
            dval = delta * (dinner + inner.abs()) + dextra + 2 * ((delta * inner).abs() + dextra)
            E[..., ch] = dval * dact(sg) + val.abs() * da_of(sg) + (val * dact(sg)).abs()
        E[..., 0:3] = colours(ws, dws, p["gCs"], p["gCs_abs"], p["rgb"])
        E[..., 4:7] = colours(wt, dwt, p["gCt"], p["gCt_abs"], p["rgb_t"])
        b = p["beta"]
        E[..., 8] = (dwt + 3 * wt) * p["gB"].abs() * dact(b) + wt * p["gB"].abs() * da_of(b)
    else:
        gg = g + (p["gCs"] * p["rgb"]).sum(-1)
        dgg = 9 * (p["g_abs"] + (p["gCs_abs"] * p["rgb"]).sum(-1))
        w, dw = weight(al, dal)
        H = w * gg
        dH = dw * gg.abs() + w * dgg + H.abs()
        dafter = _suffix(dH, False) + n_sum * _suffix(H.abs(), True)
        A, dA = lead(ec, dec, gg, dgg)
        D = A - _suffix(H, False)
        dD = dA + dafter + D.abs()
        ds, dds = p["gate"] * delta * D, p["gate"] * delta * (dD + D.abs())
        E[..., 3] = dds * dact(p["sig"]) + ds.abs() * da_of(p["sig"]) + (ds * dact(p["sig"])).abs()
        E[..., 0:3] = colours(w, dw, p["gCs"], p["gCs_abs"], p["rgb"])
    floor = (2.0 ** -109 * p["G"]).expand(R, N).reshape(R * N, 1)
    return 1.01 * E.reshape(R * N, 9), floor


def error_ratio(got, ref, E, floor):
    """|got - ref| / (u E + floor), per element (float64); an element whose bound is zero must be exact: ratio 0 if it is,
    inf if not; a NaN or Inf in `got` is inf."""
    err = (got.double() - ref).abs()
    bound = U * E + floor
    ratio = err / bound.clamp(min=1e-300)
    ratio = torch.where(bound > 0, ratio, torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return torch.where(torch.isfinite(got.double()), ratio, torch.full_like(ratio, float("inf")))


def worst(ratio, N):
    """(largest ratio, 'ray r sample i channel c') for a failure message."""
    k = int(torch.argmax(ratio))
    row, ch = divmod(k, 9)
    return float(ratio.flatten()[k]), f"ray {row // N} sample {row % N} channel {ch}"


def draw_inputs(R, N, use_t, noisy, seed):
    """Inputs at which nothing is ill-conditioned beyond what the magnitude accounts for.  Depths sorted on a 1/64 grid (the
    intervals are exact in fp32), in every second ray one repeated depth (delta = 0).  Densities such that sigma * delta
    spans 1e-4 .. 50 for a typical interval of 1/32: rays 0, 4, .. are moderate (1e-2 .. 0.5 per sample: every alpha is well
    resolved and T stays alive over a hundred samples, where a misplaced term shows best), rays 1, 5, .. are thin for their
    first half and saturate after it (T underflows mid-ray), rays 2, 6, .. span the whole range everywhere, rays 3, 7, ..
    stay thin (the transmittance survives the longest ray).  Colours strictly inside (0, 1).  `noisy` (static only, noise_std = 1): densities and noise on a 1/64
    grid, so sigma + noise is exact in fp32 and its sign is float64's; every eighth sample cancels exactly (both sides give
    0 there), every eighth ends up 1/64 below zero.  Returns fp32 CPU tensors: field_raw (R N, 9), z (R, N), noise or None."""
    gen = torch.Generator().manual_seed(seed)
    grid = max(256, 2 * N)
    z = torch.stack([torch.sort(torch.randperm(grid, generator=gen)[:N])[0] for _ in range(R)]).double() / 64.0 + 2.0
    if N >= 2:
        i = (N - 1) // 2
        z[1::2, i + 1] = z[1::2, i]

    def density():
        lo, hi = torch.full((R, N), -4.0), torch.full((R, N), 1.7)
        lo[0::4], hi[0::4] = -2.0, -0.3
        hi[1::4, :N // 2] = -2.0
        lo[1::4, N // 2:] = 0.5
        hi[3::4] = -2.0
        t = 10.0 ** (lo + (hi - lo) * torch.rand(R, N, generator=gen))
        return (32.0 * t.double() * 64).round().clamp(min=1.0) / 64.0        # on the grid; at least 1/64

    f = torch.zeros(R, N, 9, dtype=torch.float64)
    for c in (slice(0, 3), slice(4, 7)):
        f[..., c] = torch.sigmoid(2.0 * torch.randn(R, N, 3, generator=gen)).double().clamp(1e-3, 1 - 1e-3)
    f[..., 3], f[..., 7] = density(), density()
    f[..., 8] = 10.0 ** (-2.0 + 2.5 * torch.rand(R, N, generator=gen).double())
    if not use_t:
        f[..., 4:] = 0.0
    noise = None
    if noisy:
        noise = torch.randint(-32, 33, (R, N), generator=gen).double() / 64.0
        k = torch.arange(N)
        noise[:, k % 8 == 3] = -f[..., 3][:, k % 8 == 3]
        noise[:, k % 8 == 6] = -f[..., 3][:, k % 8 == 6] - 1.0 / 64
        assert torch.equal((f[..., 3].float() + noise.float()).double(), f[..., 3] + noise)
        noise = noise.float()
    f32 = f.float().view(R * N, 9)
    return f32, z.float(), noise


def draw_upstream(R, N, use_t, present, seed):
    """The eight upstream gradients in UP_NAMES order; `present`: which of them are tensors (the others None)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    shapes = dict(weights=(R, N), opacity=(R,), rgb=(R, 3), depth=(R,), transient_sigmas=(R, N), beta=(R,), rgb_static=(R, 3),
                  rgb_transient=(R, 3))
    out = []
    for k, name in enumerate(UP_NAMES):
        g = torch.randn(*shapes[name], generator=gen) * 1e-2
        out.append(g if name in present and (use_t or k < 4) else None)
    return out
