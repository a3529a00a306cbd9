"""The training forward on its own: nfl_render_kernel in NFL_MODE_STASH / NFL_MODE_STASH2 (csrc/nfl_render_impl.h with the
MLP engine of csrc/nfl_mlp.h), launched through _pack_streams, so nfl_pack_fields and the fold of nfl_compose_forward are held
where their output is consumed.  References, runner and comparisons are in tests/forward_ref.py (tests/test_forward_refs_cpu.py
holds them to an emulation and to deliberate defects); the stash formats come from tests/stash_codec.py.

Part A  every record of every layer EQUAL to a float64 reference on a field and inputs on which everything is exact.
Part B  real weights, layer by layer from the DECODED operands, so that no error compounds.
Part C  the composited outputs from the field outputs the same pass wrote, at shapes whose rays cross tiles.

Every pass runs with its activation stash inside a sentinel-filled arena: the guards stay untouched, every position a field
names is written in every segment (padded lanes included, and finite there), every mask word of a layer the pass evaluates
is written.  The mask words of layers the pass does NOT evaluate (g1 .. g4 without the transient head) are left untouched,
like the records of those layers; that is asserted too.  Nothing is asserted about unnamed positions or the 4 KiB tail pad."""
import functools

import pytest
import torch

import forward_ref as fr
import stash_codec as sc

pytestmark = pytest.mark.gpu


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=4)
def int_field(widths, lat):
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    model = gpu_util.module_from(fr.spec_of(widths, lat), fr.int_params(widths, lat))
    return model, rnd._field(model, widths[0], widths[1], torch.device(gpu_util.DEV), pack=False, prec=rnd._PREC["f16x3"])


@functools.lru_cache(maxsize=None)
def int_case(variant, R, N):
    """Inputs, reference and exactness of one Part A case, on the CPU."""
    widths, kind = fr.VARIANTS[variant]
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    P = fr.int_params(widths, lat)
    inp = fr.int_inputs(R, N, widths, lat)
    ref, pre = fr.int_reference(P, inp, widths, lat, use_t, N)
    return inp, ref, pre, fr.exactness_violations(P, inp, ref, pre, widths, lat, use_t, N)


def run_int(variant, R, N, split):
    import gpu_util
    widths, kind = fr.VARIANTS[variant]
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    inp = int_case(variant, R, N)[0]
    f = int_field(widths, lat)[1]
    on = lambda t: None if t is None else t.float().contiguous().to(gpu_util.DEV)
    zero_w = (torch.zeros(widths[0], device=gpu_util.DEV), torch.zeros(widths[1], device=gpu_util.DEV))
    out = fr.run_forward(f, on(inp["rays"]), on(inp["z"]), N, split=split, a_emb=on(inp["a"]), t_emb=on(inp["t"]) if use_t else None,
                         view_dir=on(inp["view"]), pe_w=zero_w)
    lay = fr.layout_of(widths, lat, use_t)
    n_seg = R * ((N + 31) // 32)
    mult = 2 if split else 1
    assert lay.nkp == sc.nkp_of_plan(f.wgrad_plan(use_t)[0])
    assert out["stash"].numel() == sc.mask_offset(n_seg, lay.nkp, mult) + n_seg * sc.MSK_WORDS * 256
    return out, lay, n_seg, mult


def raw_violations(field_raw, pre, R, N):
    """field_raw against float64 sigmoid / softplus of the exact head pre-activations: within 8 ulp of the result; exactly 0
    in the columns of heads the pass does not have.  Returns (complaints, largest error in ulp)."""
    have = ~torch.isnan(pre[0])
    exp = fr.head_activation(pre)[:, have]
    got = field_raw.double()
    ulps = (got[:, have] - exp).abs() / fr.ulp32(exp)
    bad = []
    if not float(ulps.max()) <= 8.0:
        k, col = (ulps == ulps.max()).nonzero()[0].tolist()
        bad.append(f"field_raw column {have.nonzero().flatten()[col].item()} is {float(ulps.max()):.2f} ulp off at {fr.locate(k, N, n_cu(), R)}")
    if bool(got[:, ~have].any()):
        bad.append("field_raw is not zero in the columns of a head the pass does not have")
    return bad, float(ulps.max())


def absent_untouched(out, lay, widths, n_seg, mult):
    """A NeRF-W field run without the transient head: tau and g1 .. g4 are not written."""
    full = fr.layout_of(widths, True, True)
    rec = sc.Layout._records(out["stash"].cpu(), n_seg, lay.act_slots, mult)
    got = sc.Layout._get(rec.reshape(n_seg * mult, 1, lay.act_slots, 32, 16)[:, 0],
                         {k: full.act[k] for k in ("tau", "g1", "g2", "g3", "g4")})
    return [f"{k} written by a pass without the transient head" for k, v in got.items()
            if not bool((v.contiguous().view(torch.int16) == fr.SENT16).all())]


@pytest.mark.parametrize("variant,R,N", fr.A_CASES, ids=[f"{v}-R{R}N{N}" for v, R, N in fr.A_CASES])
def test_forward_exact_on_integers(variant, R, N):
    """Ternary sparse weights and integer biases in every layer (xyz_encoding_final too: the fold is an exact integer matrix),
    BARF weights 0 so that only the raw coordinates of both encodings are non-zero, rays, depths, view directions and codes
    on dyadic grids: every pre-activation is an exact dyadic number in every arithmetic.  The conditions -- every stashed
    value one fp16, partial sums below 2^24 steps, both mask values in every 32-feature tile of every masked layer among the
    live samples, no layer all zero, head pre-activations within +-8 -- are checked on the CPU before anything is launched,
    and so is the launch geometry the shape is here for (forward_ref.situation_violations, from the device's CU count).

    Then, for the split (STASH2) run: every hi record of pe, h1 .. h8, dir_side, dirh, tau and g1 .. g4 EQUALS the reference
    (-0 == 0), every lo record is zero, every mask bit is value > 0; field_raw is float64 sigmoid / softplus of the exact
    head pre-activation within 8 ulp (expf, log1pf and the division at 2 ulp each); and the hi-only (STASH) run of the same
    case gives bit-identical hi records, mask words and field_raw.

    This part cannot see a lost lo product: every lo operand is zero here.  That is Part B's job.

    Measured on the MI355X (printed per case): largest field_raw error 0.83 ulp on the base field at every shape (the
    2 n_cu + 1 rays of the case below included), 0.76 .. 1.46 ulp on the NeRF-W variants (1.46: R = 3, N = 300); no record,
    mask word or field_raw bit differs between the two modes."""
    widths, kind = fr.VARIANTS[variant]
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    inp, ref, pre, violations = int_case(variant, R, N)
    assert not violations, violations
    assert not fr.situation_violations(R, N, n_cu())

    out2, lay, n_seg, _ = run_int(variant, R, N, True)
    assert out2["guards_ok"], "the pass wrote outside its activation stash"
    dec2 = fr.decode(out2["stash"].cpu(), lay, n_seg, 2, use_t)
    bad = fr.unwritten(dec2, use_t, N)
    bad += [f"{k}: {v}" for k, v in fr.mismatches(dec2, ref, R, N, n_cu(), use_t).items()]
    raw_bad, ulps = raw_violations(out2["field_raw"].cpu(), pre, R, N)
    bad += raw_bad
    if variant == "narrow":
        bad += fr.beyond_width(dec2["rec"], lay, widths)
    if kind == "nerfw_not":
        bad += absent_untouched(out2, lay, widths, n_seg, 2)

    out1, _, _, _ = run_int(variant, R, N, False)
    assert out1["guards_ok"], "the hi-only pass wrote outside its activation stash"
    dec1 = fr.decode(out1["stash"].cpu(), lay, n_seg, 1, use_t)
    bad += ["hi-only: " + b for b in fr.unwritten(dec1, use_t, N)]
    bad += [f"{k}: {v}" for k, v in fr.same_bits(dec1, dec2).items()]
    if not torch.equal(out1["field_raw"].view(torch.int32), out2["field_raw"].view(torch.int32)):
        bad.append("field_raw differs between the hi-only and the split run")
    print(f"forward exact {variant} R={R} N={N}: field_raw within {ulps:.2f} ulp")
    assert not bad, "\n".join(bad)


def test_forward_exact_on_integers_two_full_tiles_per_workgroup():
    """R = 2 n_cu + 1, N = 33 on the base field, hi-only: four rays = two full tiles per workgroup with two rays per tile,
    one ray in the last workgroup, one live lane in every ray's second segment.  The stash is about 180 MB, so it is decoded
    and compared on the device.  Same assertions as above (no lo records)."""
    R, N = fr.big_shape(n_cu())
    inp, ref, pre, violations = int_case("base", R, N)
    assert not violations, violations
    assert not fr.situation_violations(R, N, n_cu())
    out, lay, n_seg, _ = run_int("base", R, N, False)
    assert out["guards_ok"], "the pass wrote outside its activation stash"
    dec = fr.decode(out["stash"], lay, n_seg, 1, False)
    bad = fr.unwritten(dec, False, N)
    bad += [f"{k}: {v}" for k, v in fr.mismatches(dec, ref, R, N, n_cu(), False).items()]
    raw_bad, ulps = raw_violations(out["field_raw"].cpu(), pre, R, N)
    print(f"forward exact base R={R} N={N}: field_raw within {ulps:.2f} ulp")
    assert not bad + raw_bad, "\n".join(bad + raw_bad)


# ---- Part B ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("barf", [False, True], ids=["plain", "barf"])
@pytest.mark.parametrize("lat", [False, True], ids=["base", "nerfw"])
@pytest.mark.parametrize("R,N", fr.B_SHAPES)
def test_forward_layer_by_layer_on_real_weights(R, N, lat, barf):
    """The oracle's `sharp` weights, exact_rays, random fp32 codes, BARF weights absent or != 1, split stash.  The decoded
    hi + lo of a layer's inputs ARE the operands its MFMAs read; the weight operands are the test's own split of the fp32
    matrices (hi = W.half(), lo = (W - hi).half()); for dir_encoding.0 / transient_encoding.0 these are the folded matrices
    and biases read back from the field, so nfl_compose_forward's rounding is not part of any bound.  For every layer, with K
    input columns (forward_ref.check_layers; the product plan is read from csrc/nfl_prods.h):
      prediction      pre = b + (w_hi + w_lo) x_hi + w_hi x_lo in float64 -- the three products the kernel issues
      hard bound      |h^ - relu(pre)| <= (3 K + 1) 2^-24 (|b| + sum|terms|) + 2^-22 |relu(pre)| + 2^-24
      mask            bit == (h^_hi != 0), exactly
      split           h^_hi is an fp16 nearest to h^_hi + h^_lo (either neighbour when hi + lo is an exact tie: x - hi rounded
                      UP to half a step of hi)
      discrimination  over the live, mask-set elements rms(h^ - full) <= rms(full - mutant) / 8 for the mutant predictions
                      without w_lo x_hi and without w_hi x_lo, and rms(full - mutant) > 0
    The codes in dir_side and tau are bit-exact (hi = code.half(), lo = (code - hi).half()); pe and dir_side's direction
    columns are within 1e-6 + 2^-22 |v| of the float64 encoding of the exact point times the BARF weight, the raw columns
    exact.  field_raw is float64 sigmoid / softplus of the layer-local head pre-activation within the accumulation bound
    times the activation's slope (1/4, 1) plus 8 ulp.  The hi-only run gives bit-identical hi records, masks and field_raw.

    Measured on the MI355X, per layer the worst of the eight cases (printed per case and layer): error / hard bound, then
    rms(h^ - full) / rms(full - mutant) without w_lo x_hi and without w_hi x_lo (allowed: 1/8; a lost product reads 1):
        h1   2.0e-2  7.0e-4  6.8e-4      h5   7.3e-3  1.6e-3  1.7e-3      dirh 5.0e-3  1.3e-3  1.6e-3
        h2   6.6e-3  1.3e-3  1.2e-3      h6   6.8e-3  2.2e-3  2.0e-3      g1   5.3e-3  8.3e-4  8.2e-4
        h3   5.7e-3  2.3e-3  2.0e-3      h7   8.1e-3  4.2e-3  3.5e-3      g2   1.1e-2  1.8e-3  1.7e-3
        h4   9.2e-3  5.4e-3  4.4e-3      h8   1.0e-2  6.6e-3  5.9e-3      g3   1.8e-2  3.5e-3  3.4e-3
                                                                          g4   1.7e-2  3.3e-3  3.7e-3
    heads, error / bound: sigma 4.0e-4, rgb 4.5e-2, sigma_t 7.3e-4, rgb_t 3.8e-2, beta 1.3e-2.  The issue's estimate that a
    lost product sits near a third of the hard bound is not borne out: the worst-case bound is 50 to 200 times the error of
    a correct kernel, and only the rms rule tells a lost product from rounding."""
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    dev = gpu_util.DEV
    widths, spec, P, inp = fr.real_inputs(R, N, lat)
    model = gpu_util.module_from(spec, P)
    f = rnd._field(model, widths[0], widths[1], torch.device(dev), pack=False, prec=rnd._PREC["f16x3"])
    on = lambda t: None if t is None else t.to(dev)
    pe_w = fr.BARF if barf else None
    kw = dict(a_emb=on(inp["a"]), t_emb=on(inp["t"]), pe_w=None if pe_w is None else tuple(on(w) for w in pe_w))
    out2 = fr.run_forward(f, on(inp["rays"]), on(inp["z"]), N, split=True, **kw)
    out1 = fr.run_forward(f, on(inp["rays"]), on(inp["z"]), N, split=False, **kw)
    assert out2["guards_ok"] and out1["guards_ok"], "a pass wrote outside its activation stash"
    F = {k: v.detach().float().cpu() for k, v in model.named_parameters()}
    for name, (w, b) in f.fold.items():
        F[name + ".weight"], F[name + ".bias"] = w.cpu(), b.cpu()
    lay = fr.layout_of(widths, lat, lat)
    n_seg = R * ((N + 31) // 32)
    dec2 = fr.decode(out2["stash"].cpu(), lay, n_seg, 2, lat)
    dec1 = fr.decode(out1["stash"].cpu(), lay, n_seg, 1, lat)
    bad = fr.unwritten(dec2, lat, N) + ["hi-only: " + b for b in fr.unwritten(dec1, lat, N)]
    more, report = fr.check_layers(dec2, out2["field_raw"].cpu(), F, widths, lat, lat, R, N, n_cu())
    bad += more + fr.check_sides(dec2, inp, widths, lat, lat, R, N, pe_w)
    bad += [f"{k}: {v}" for k, v in fr.same_bits(dec1, dec2).items()]
    if not torch.equal(out1["field_raw"].view(torch.int32), out2["field_raw"].view(torch.int32)):
        bad.append("field_raw differs between the hi-only and the split run")
    fmt = lambda x: "-" if x is None else f"{x:.2e}"
    print(f"forward layer by layer R={R} N={N} {'nerfw' if lat else 'base'} {'barf' if barf else 'plain'} "
          f"(error / bound, rms ratio without w_lo x_hi, without w_hi x_lo): "
          + "; ".join(f"{k} {fmt(v[0])} {fmt(v[1])} {fmt(v[2])}" for k, v in report.items()))
    assert not bad, "\n".join(bad)


# ---- Part C ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white_back", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("lat", [False, True], ids=["base_noise", "nerfw"])
@pytest.mark.parametrize("R,N", [(2, 160), (3, 300)])
def test_forward_composites_its_own_field_outputs_across_tiles(R, N, lat, white_back):
    """One ray per workgroup, two and three tiles: the compositing carry (carry_in / carry_out, m0 < 0) is taken.  weights,
    opacity, rgb, depth (and beta, rgb_static, rgb_transient) against a float64 composite of the field_raw the SAME pass
    wrote (forward_ref.composite_ref; last delta 1e2), the base field with density noise.  Bounds from the project's own
    numbers (tests/test_compbwd_gpu.py grants alpha 3 u and each factor 1 - alpha 5 u absolute, u = 2^-24): a weight of
    sample i gets (5 i + 3) u, a per-ray sum of N terms N u sum|terms| more, every further rounded addition u of its result.
    transient_sigmas equals field_raw[:, 7] bit for bit.

    Measured on the MI355X, largest error / bound (printed per case): weights 0.056 (R = 2, N = 160) and 0.060 (R = 3,
    N = 300) on the base field with noise, 0.13 and 0.14 on NeRF-W; over all eight cases opacity 7.5e-5, depth 8.6e-5,
    rgb 8.4e-5, rgb_static 9.4e-5, rgb_transient 7.9e-5, beta 6.3e-5; transient_sigmas bit-identical."""
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    dev = gpu_util.DEV
    assert not fr.situation_violations(R, N, n_cu())
    widths, spec, P, inp = fr.real_inputs(R, 1, lat)
    model = gpu_util.module_from(spec, P)
    f = rnd._field(model, widths[0], widths[1], torch.device(dev), pack=False, prec=rnd._PREC["f16x3"])
    z = fr.sorted_depths(R, N, 11 * R + N)
    noise = None if lat else 0.1 * torch.randn(R, N, generator=torch.Generator().manual_seed(N))     # of the densities' own size
    on = lambda t: None if t is None else t.to(dev)
    out = fr.run_forward(f, on(inp["rays"]), on(z), N, split=True, a_emb=on(inp["a"]), t_emb=on(inp["t"]), noise=on(noise),
                         noise_std=0.0 if lat else 1.0, white_back=white_back)
    assert out["guards_ok"]
    raw = out["field_raw"].cpu()
    assert bool(torch.isfinite(raw).all())
    ref = fr.composite_ref(raw, z, noise=noise, noise_std=0.0 if lat else 1.0, use_t=lat, white_back=white_back,
                           beta_min=spec.beta_min)
    bad, report = [], []
    for name, (v, b) in ref.items():
        got = out[name].cpu().double().view_as(v)
        ratio = (got - v).abs() / b
        ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
        report.append(f"{name} {float(ratio.max()):.2e}")
        assert float(v.abs().max()) > 0, name
        if not float(ratio.max()) <= 1.0:
            k = (ratio == ratio.max()).nonzero()[0].tolist()
            bad.append(f"{name}: {float(ratio.max()):.3f} of its bound at {k} (ray first; a weight's second index is its sample): "
                       f"got {got[tuple(k)].item()!r} float64 {v[tuple(k)].item()!r}")
    if lat and not torch.equal(out["transient_sigmas"].cpu().view(torch.int32).flatten(), raw[:, 7].contiguous().view(torch.int32)):
        bad.append("transient_sigmas is not field_raw[:, 7]")
    # the rays do reach their later tiles: some weight beyond sample 128 is not negligible
    assert float(ref["weights"][0][:, 128:].max()) > 1e-2
    print(f"forward compositing R={R} N={N} {'nerfw' if lat else 'base+noise'} white={white_back}: error / bound " + ", ".join(report))
    assert not bad, "\n".join(bad)
