"""The references and comparisons of tests/test_compbwd_gpu.py and tests/test_dgrad_gpu.py, on the CPU with no kernel
involved: the references agree with autograd, and every comparison rejects a candidate that is the reference with one defect
of the kind those tests exist to catch."""
import pytest
import torch

import compbwd_ref as cr
import stash_codec as sc


# ---- compositing backward ----------------------------------------------------------------------------------------------
def comp_case(use_t, noisy, R=5, N=129, seed=3):
    f, z, noise = cr.draw_inputs(R, N, use_t, noisy, seed)
    kw = dict(noise=noise, noise_std=1.0 if noisy else 0.0, use_t=use_t, white_back=True,
              grads=cr.draw_upstream(R, N, use_t, cr.UP_NAMES, seed), go=0.37, g_tsig_const=1e-3)
    return f, z, kw


@pytest.mark.parametrize("use_t,noisy", [(True, False), (False, True), (False, False)])
def test_closed_form_is_the_autograd_gradient(use_t, noisy):
    """The formulas the bound is built on are the derivative: float64 against float64, a million times below the bound."""
    f, z, kw = comp_case(use_t, noisy)
    ref = cr.reference(f, z, **kw)
    cf = cr.closed_form(f, z, **kw)
    E, floor = cr.error_units(f, z, **kw)
    assert float(ref.abs().max()) > 0
    assert bool(((ref - cf).abs() <= 1e-6 * cr.U * E + floor).all())
    if not use_t:
        assert not ref[:, 4:].any()
        pre = f.view(*z.shape, 9)[..., 3] + (kw["noise"] if noisy else 0.0)
        assert not ref.view(*z.shape, 9)[..., 3][pre <= 0].any()            # exact zeros and gated samples: both 0
        assert not noisy or int((pre == 0).sum()) > 0


@pytest.mark.parametrize("N", [65, 129])
@pytest.mark.parametrize("use_t,noisy", [(True, False), (False, True), (False, False)])
def test_compbwd_bound_is_a_small_multiple_of_the_value(use_t, noisy, N):
    """How tight the bound is where nothing is ill-conditioned: on the moderate ray (ray 0, alpha 1e-2 .. 0.5, T alive) its
    median over the non-zero elements is a small multiple of (N + 40) u of the VALUE.  Each factor 1 - alpha_k carries about
    5 u and enters T_j j-fold, the upstream sums 6 .. 9 u, the suffix 8 + N / 64: about 6 N u on a colour, and a few times
    that on a density, where T_{i+1} g_i and the suffix partly cancel.  Measured: 2.3 .. 3.1 (colours), 18 .. 21 (densities)."""
    f, z, kw = comp_case(use_t, noisy, N=N)
    ref = cr.reference(f, z, **kw).view(5, N, 9)[0]
    E, floor = cr.error_units(f, z, **kw)
    rel = ((cr.U * E + floor).view(5, N, 9)[0] / ref.abs().clamp(min=1e-300)) / ((N + 40) * cr.U)
    colour, density = rel[:, 0:3][ref[:, 0:3] != 0].median(), rel[:, 3][ref[:, 3] != 0].median()
    print(f"bound / |value| on the moderate ray, units of (N + 40) u: colours {float(colour):.2f}, density {float(density):.2f}")
    assert float(colour) <= 8 and float(density) <= 40


@pytest.mark.parametrize("N", [129, 1024])
@pytest.mark.parametrize("use_t,noisy,defects", [(True, False, ("T_i", "suffix64", "last_delta", "block")),
                                                 (False, False, ("T_i", "suffix64", "last_delta", "block")),
                                                 # +-1/2 of noise on the last density: exp(-1e2 x) is 0 like exp(-1e10 x)
                                                 (False, True, ("T_i", "suffix64", "block"))])
def test_compbwd_comparison_accepts_fp32_and_rejects_defects(use_t, noisy, defects, N):
    """At N = 129 and at NFL_CB_MAXN, where the bound is widest.  "block": a relative error of 1e-3 in the samples 64 .. 127
    of every ray.  Measured margins (largest error / bound): T_i 6e5 .. 1.7e6, suffix64 1.6e4 .. 3.6e4, last_delta 12 (static,
    N = 1024: one thin ray's last sample) .. 2.9e4, block 44 (static) .. 3300 (transient), in nearly every element of the block."""
    f, z, kw = comp_case(use_t, noisy, N=N)
    R = z.shape[0]
    ref = cr.reference(f, z, **kw)
    E, floor = cr.error_units(f, z, **kw)
    # the reference rounded to fp32 is a result the kernel may return
    assert float(cr.error_ratio(ref.float(), ref, E, floor).max()) <= 1.0
    for defect in defects:
        if defect == "block":
            bad = ref.clone().view(R, N, 9)
            bad[:, 64:128] *= 1.001
            least = int((bad[:, 64:128] != 0).sum()) // 2          # more than half of what the block holds
            bad = bad.reshape(R * N, 9)
        else:
            bad = cr.closed_form(f, z, defect=defect, **kw)
            least = 1 if defect == "last_delta" else R               # the last sample of a ray whose T is still alive
        ratio = cr.error_ratio(bad.float(), ref, E, floor)
        worst, where = cr.worst(ratio, N)
        print(f"{defect}: worst ratio {worst:.3g} at {where}; {int((ratio > 1).sum())} elements beyond the bound")
        assert worst > 10.0 and int((ratio > 1).sum()) >= least, (defect, worst, where)
    nan = ref.float().clone()
    nan[7, 3] = float("nan")
    assert float(cr.error_ratio(nan, ref, E, floor).max()) == float("inf")


# ---- dgrad -------------------------------------------------------------------------------------------------------------
import test_dgrad_gpu as dg          # noqa: E402  (its helpers; the module's tests themselves need the GPU)


@pytest.mark.parametrize("widths,kind,R,N,gmax_value", dg.HOST_CASES,
                         ids=[f"{'x'.join(map(str, c[0]))}-{c[1]}-R{c[2]}N{c[3]}-{c[4]}" for c in dg.HOST_CASES])
def test_integer_exactness_conditions_hold(widths, kind, R, N, gmax_value):
    """The committed seeds and sparsity: every scaled delta an integer within 2048, something non-zero in every feature tile
    of every layer, latent sums below 2^24."""
    masks, ints, scale, deltas, lat_rows = dg.host_case(widths, kind, R, N, gmax_value)
    assert not dg.exactness_violations(deltas, R, N)
    for v in dg.latent_sums(lat_rows, R, N, 1.0).values():
        assert torch.equal(v, v.round()) and float(v.abs().max()) < 2.0 ** 24 and bool(v.any())
    # some samples do have an all-zero and an all-one layer
    assert not masks["h3"][3].any() and bool(masks["h6"][5].all())


def test_reference_chain_is_the_autograd_gradient():
    """The chain against autograd on the model itself (float64, dense random weights): masks are the relu's, deltas the
    gradients of the pre-activations, the latent terms the gradients of the codes."""
    from oracle import nerfw_oracle as orc
    torch.manual_seed(4)
    widths = (3, 1, 5, 4)
    spec = orc.FieldSpec("fine", n_emb_xyz=3, n_emb_dir=1, encode_appearance=True, n_a=5, encode_transient=True, n_tau=4)
    P = {k: v.double() for k, v in orc.make_field_params(spec, 5, "sharp").items()}
    n, cx, cd = 32, 21, 9
    pe, tau = torch.randn(n, cx).double().requires_grad_(True), torch.randn(n, 4).double().requires_grad_(True)
    dirs, a = torch.randn(n, cd).double(), torch.randn(n, 5).double().requires_grad_(True)
    pre = {}

    def lin(name, x, key):
        y = torch.nn.functional.linear(x, P[name + ".weight"], P[name + ".bias"])
        y.retain_grad()
        pre[key] = y
        return y

    h = pe
    for l in range(1, 9):
        h = torch.relu(lin(f"xyz_encoding_{l}.0", torch.cat([pe, h], 1) if l == 5 else h, f"delta{l}"))
    sigma = lin("static_sigma.0", h, "heads0")
    feat = torch.nn.functional.linear(h, P["xyz_encoding_final.weight"], P["xyz_encoding_final.bias"])
    rgb = lin("static_rgb.0", torch.relu(lin("dir_encoding.0", torch.cat([feat, dirs, a], 1), "delta_dirh")), "heads1")
    g = torch.cat([feat, tau], 1)
    for m, j in enumerate((0, 2, 4, 6)):
        g = torch.relu(lin(f"transient_encoding.{j}", g, f"delta_g{m + 1}"))
    outs = [rgb, sigma, lin("transient_rgb.0", g, "heads3"), lin("transient_sigma.0", g, "heads2"), lin("transient_beta.0", g, "heads4")]
    head = torch.randn(n, 9).double()
    (torch.cat(outs, 1) * head).sum().backward()
    masks = {"dirh": pre["delta_dirh"] > 0}
    masks.update({f"h{l}": pre[f"delta{l}"] > 0 for l in range(1, 9)})
    masks.update({f"g{m}": pre[f"delta_g{m}"] > 0 for m in range(1, 5)})
    deltas, lat = dg.reference_chain(P, widths, masks, head, True, True)
    for name, v in deltas.items():
        assert torch.allclose(v, pre[name].grad, rtol=1e-10, atol=1e-12), name
    assert torch.allclose(lat["a"], a.grad, rtol=1e-10, atol=1e-12) and torch.allclose(lat["t"], tau.grad, rtol=1e-10, atol=1e-12)


def test_dgrad_comparison_rejects_defects():
    """The exact comparison, fed the reference with one defect at a time."""
    widths, kind, R, N = dg.WIDTHS[0], "nerfw_t", 9, 40
    masks, ints, scale, deltas, lat_rows = dg.host_case(widths, kind, R, N, 32.0)
    params = {k: v.detach() for k, v in dg.make_model(widths, kind).named_parameters()}
    clean = {k: v.clone() for k, v in deltas.items()}
    assert not dg.mismatches(clean, deltas, R, N) and not dg.mismatches(clean, deltas, R, N, lo={k: torch.zeros_like(v) for k, v in clean.items()})
    live = dg.padded_rows(R, N)

    def rerun(m):
        return dg.reference_chain(params, widths, m, ints, True, True)[0]

    # one mask bit flipped, where the value behind it is not zero
    pre = rerun(dict(masks, h5=torch.ones_like(masks["h5"])))["delta5"]
    row, col = [(r, c) for r, c in pre.nonzero().tolist() if r in set(live.tolist())][0]
    flipped = {k: v.clone() for k, v in masks.items()}
    flipped["h5"][row, col] ^= True
    msg = dg.mismatches(rerun(flipped), deltas, R, N)
    assert "delta5" in msg and f"feature {col} " in msg["delta5"], msg

    # the mask words of tile t + 1 used for tile t
    shifted = dict(masks, h2=torch.roll(masks["h2"], -32, 1))
    msg = dg.mismatches(rerun(shifted), deltas, R, N)
    assert "delta2" in msg and "delta1" in msg and "delta3" not in msg, msg

    # one segment's delta duplicated into its neighbour
    dup = {k: v.clone() for k, v in deltas.items()}
    dup["delta7"][64:96] = dup["delta7"][32:64]
    msg = dg.mismatches(dup, deltas, R, N)
    assert list(msg) == ["delta7"] and "segment 2 " in msg["delta7"], msg

    # a padded lane that is not zero (ray 0, second segment: samples 40 .. 63 do not exist)
    pad = {k: v.clone() for k, v in deltas.items()}
    pad["delta_g3"][32 + 20, 7] = 1.0
    msg = dg.mismatches(pad, deltas, R, N)
    assert list(msg) == ["delta_g3"] and "padded" in msg["delta_g3"], msg
    # a residual record that is not zero
    lo = {k: torch.zeros_like(v) for k, v in deltas.items()}
    lo["heads1"][3, 1] = 2.0 ** -12
    assert list(dg.mismatches(clean, deltas, R, N, lo=lo)) == ["heads1 (lo record)"]

    # a latent row counted twice, per ray and in the table
    latent_row = torch.tensor([3, 0, 3, 3, 1, 0, 4, 3, 1])
    for lr, nv in ((None, None), (latent_row, 5)):
        exp = dg.latent_sums(lat_rows, R, N, scale, lr, nv)
        assert not dg.latent_mismatches({k: v.float() for k, v in exp.items()}, exp)
        twice = {k: v.float().clone() for k, v in exp.items()}
        twice["a"][1] *= 2
        assert list(dg.latent_mismatches(twice, exp)) == ["g_a"]
    # duplicates in latent_row do add up
    assert torch.equal(dg.latent_sums(lat_rows, R, N, scale, latent_row, 5)["t"][3],
                       dg.latent_sums(lat_rows, R, N, scale)["t"][[0, 2, 3, 7]].sum(0))
