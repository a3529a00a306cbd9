"""The inference passes on their own: nfl_render_kernel in NFL_MODE_RENDER (every rendered image) and NFL_MODE_EMBED
(NeRF.forward on encoded inputs), of the three-product kernels (`f16x3`: nfl_render_x3.hip, nfl_render_x3w.hip) and of the
single-product ones (`f16`: nfl_render_x1.hip), held to the training forward that tests/test_forward_gpu.py holds to float64.
Runners, references and comparisons are in tests/forward_ref.py; tests/test_forward_refs_cpu.py holds them to stand-ins and to
deliberate defects.

Part A  the integer field, on which every arithmetic gives the same bits: RENDER and EMBED of both kernels EQUAL STASH2.
Part B  real weights, three-product kernel: RENDER EQUALS STASH2 of the same inputs.
Part C  real weights, single-product kernel: nearer to its own arithmetic (float64 accumulation of the fp16 operands) than
        that arithmetic is to the unrounded network; composites from its own field outputs.

Every output buffer lies in a NaN-filled arena with guards on either side (forward_ref.Arena): the guards stay untouched
and no NaN is left inside."""
import functools

import pytest
import torch

import forward_ref as fr
from test_forward_gpu import n_cu, raw_violations

pytestmark = pytest.mark.gpu

PRECS = ("f16x3", "f16")


def outputs(use_t):
    return ["field_raw", "weights", "opacity", "rgb", "depth"] + (["beta", "rgb_static", "rgb_transient", "transient_sigmas"] if use_t else [])


def field_of(model, widths, prec):
    import gpu_util
    from nerf_fl_amd import rendering as rnd
    return rnd._field(model, widths[0], widths[1], torch.device(gpu_util.DEV), pack=False, prec=rnd._PREC[prec])


def kernel_name(widths, prec):
    from nerf_fl_amd import _lib, rendering as rnd
    return _lib.lib().nfl_render_kernel_name(rnd._PREC[prec], widths[0]).decode()


@functools.lru_cache(maxsize=4)
def int_model(widths, lat):
    import gpu_util
    return gpu_util.module_from(fr.spec_of(widths, lat), fr.int_params(widths, lat))


@functools.lru_cache(maxsize=None)
def int_case(variant, R, N):
    """Inputs, reference and exactness of one Part A case, on the CPU: the conditions of the training forward's test and the
    one the single-product kernel adds."""
    widths, kind = fr.VARIANTS[variant]
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    P = fr.int_params(widths, lat)
    inp = fr.int_inputs(R, N, widths, lat)
    ref, pre = fr.int_reference(P, inp, widths, lat, use_t, N)
    return inp, pre, fr.exactness_violations(P, inp, ref, pre, widths, lat, use_t, N) + fr.fp16_weight_violations(P)


def clean(out, what):
    """Guards intact, nothing left unwritten."""
    bad = [f"{what}: wrote outside {k}" for k, ok in out["guards"].items() if not ok]
    return bad + [f"{what}: NaN left in {k}" for k in out["nan_left"]]


@pytest.mark.parametrize("variant,R,N", fr.A_CASES, ids=[f"{v}-R{R}N{N}" for v, R, N in fr.A_CASES])
def test_inference_exact_on_integers(variant, R, N):
    """The field and inputs of tests/test_forward_gpu.py::test_forward_exact_on_integers, on which every pre-activation is an
    exact dyadic number in every arithmetic -- in the single-product one too, because every weight, the folded matrices as
    read back from the fields included, is exactly one fp16 (checked before anything renders).  The anchor is the STASH2 pass
    of the three-product kernel, which that test holds to float64 record by record.  Then
      RENDER f16x3, RENDER f16   field_raw, weights, opacity, rgb, depth (and beta, rgb_static, rgb_transient,
                                 transient_sigmas with the transient head) bit-identical to the anchor's: same field values,
                                 same compositing code, so the carry across tiles at N = 160 and N = 300 comes with it;
                                 field_raw of the f16x3 pass within 8 ulp of float64 sigmoid / softplus;
      EMBED f16x3, EMBED f16     on forward_ref.int_embedded (row stride = width + 3, NaN in the stride columns): the columns
                                 NeRF.forward returns bit-identical to the anchor's on all R N points, on the first 33 and on
                                 the first one (R N = 120: a partial last segment);
      the NeRF-W field           also with output_transient=False (rows without the transient code) and sigma_only=True
                                 (rows of the encoded position alone).
    Every buffer's guards are intact and no NaN is left in any; the launch geometry is the one the shape is in the suite for;
    the `wide` field runs nfl_render_kernel<3, 1, 15, 0> / <1, 1, 15, 0>, the others <., 1, 10, 0>.

    Measured on the MI355X (printed per case): no bit differs in any of the fourteen cases, over both RENDER passes and the
    2 (one point), 6 or 10 (the NeRF-W field) EMBED runs of each; field_raw of the f16x3 RENDER pass is within 0.83 ulp of
    float64 on the base field and 0.76 .. 1.46 ulp on the others, as the anchor's is."""
    from nerf_fl_amd import rendering as rnd
    import gpu_util
    widths, kind = fr.VARIANTS[variant]
    lat, use_t = kind != "coarse", kind == "nerfw_t"
    inp, pre, violations = int_case(variant, R, N)
    assert not violations, violations
    assert not fr.situation_violations(R, N, n_cu())
    nfx = 15 if variant == "wide" else 10
    assert kernel_name(widths, "f16x3") == f"nfl_render_kernel<3, 1, {nfx}, 0>"
    assert kernel_name(widths, "f16") == f"nfl_render_kernel<1, 1, {nfx}, 0>"

    model = int_model(widths, lat)
    fields = {prec: field_of(model, widths, prec) for prec in PRECS}
    rnd._pack_streams(list(fields.values()))
    P = fr.int_params(widths, lat)
    for prec, f in fields.items():
        folded = fr.fp16_weight_violations(P, f.fold)
        assert not folded, (prec, folded)

    on = lambda t: None if t is None else t.float().contiguous().to(gpu_util.DEV)
    kw = dict(a_emb=on(inp["a"]), t_emb=on(inp["t"]) if use_t else None, view_dir=on(inp["view"]),
              pe_w=(torch.zeros(widths[0], device=gpu_util.DEV), torch.zeros(widths[1], device=gpu_util.DEV)))
    rays, z = on(inp["rays"]), on(inp["z"])
    anchor = fr.run_forward(fields["f16x3"], rays, z, N, split=True, **kw)
    assert anchor["guards_ok"], "the anchor pass wrote outside its activation stash"
    bad, names = [], outputs(use_t)
    for prec, f in fields.items():
        out = fr.run_render(f, rays, z, N, **kw)
        bad += clean(out, f"RENDER {prec}")
        bad += [f"RENDER {prec} against STASH2, {k}: {v}" for k, v in fr.bit_differences(out, anchor, names).items()]
        if prec == "f16x3":
            raw_bad, ulps = raw_violations(out["field_raw"].cpu(), pre, R, N)
            bad += raw_bad

    X = fr.int_embedded(inp, widths, lat, use_t, N)
    cx, n_t = 6 * widths[0] + 3, widths[3] if use_t else 0
    runs = [(X, False, use_t, B) for B in sorted({R * N, min(33, R * N), 1})]
    if variant == "nerfw":
        runs += [(X[:, :X.shape[1] - n_t], False, False, R * N), (X[:, :cx], True, False, R * N)]
    n_embed = 0
    for prec, f in fields.items():
        for x, sigma_only, output_transient, B in runs:
            what = f"EMBED {prec} B={B}" + (" sigma_only" if sigma_only else "" if output_transient == use_t else " output_transient=False")
            out = fr.run_embed(f, x[:B], sigma_only=sigma_only, output_transient=output_transient)
            bad += clean(out, what)
            cols = fr.embed_columns(sigma_only, output_transient) if (sigma_only or output_transient != use_t) else list(range(9))
            diff = fr.bit_differences({"raw": out["raw"][:, cols]}, {"raw": anchor["field_raw"][:B, cols]}, ["raw"])
            bad += [f"{what} against STASH2, columns {cols}: {v}" for v in diff.values()]
            n_embed += 1
    print(f"inference exact {variant} R={R} N={N}: RENDER f16x3 / f16 and {n_embed} EMBED runs against STASH2, "
          f"{len(bad)} complaints; field_raw within {ulps:.2f} ulp of float64")
    assert not bad, "\n".join(bad)


# ---- Part B ------------------------------------------------------------------------------------------------------------
def real_fields(R, N, lat):
    import gpu_util
    widths, spec, P, inp = fr.real_inputs(R, N, lat)
    model = gpu_util.module_from(spec, P)
    return widths, spec, inp, model


def real_kw(inp, barf):
    import gpu_util
    on = lambda t: None if t is None else t.to(gpu_util.DEV)
    pe_w = fr.BARF if barf else None
    return on(inp["rays"]), on(inp["z"]), dict(a_emb=on(inp["a"]), t_emb=on(inp["t"]),
                                               pe_w=None if pe_w is None else tuple(on(w) for w in pe_w))


@pytest.mark.parametrize("barf", [False, True], ids=["plain", "barf"])
@pytest.mark.parametrize("lat", [False, True], ids=["base", "nerfw"])
@pytest.mark.parametrize("R,N", fr.B_SHAPES)
def test_render_equals_the_training_forward_on_real_weights(R, N, lat, barf):
    """The inputs of tests/test_forward_gpu.py::test_forward_layer_by_layer_on_real_weights (the oracle's `sharp` weights,
    exact_rays, random fp32 codes, BARF weights absent or != 1), three-product kernel: NFL_MODE_RENDER gives field_raw and
    every composited output bit-identical to the STASH2 pass of the same inputs, which that test holds layer by layer.  A
    product lost in the inference instantiation alone changes bits (tests/test_forward_refs_cpu.py shows it on the emulation).
    Guards intact, no NaN left."""
    widths, spec, inp, model = real_fields(R, N, lat)
    f = field_of(model, widths, "f16x3")
    rays, z, kw = real_kw(inp, barf)
    anchor = fr.run_forward(f, rays, z, N, split=True, **kw)
    out = fr.run_render(f, rays, z, N, **kw)
    assert anchor["guards_ok"], "the anchor pass wrote outside its activation stash"
    bad = clean(out, "RENDER f16x3")
    bad += [f"RENDER against STASH2, {k}: {v}" for k, v in fr.bit_differences(out, anchor, outputs(lat)).items()]
    assert bool(torch.isfinite(anchor["field_raw"]).all()) and bool(anchor["weights"].any())
    assert not bad, "\n".join(bad)


# ---- Part C ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("barf", [False, True], ids=["plain", "barf"])
@pytest.mark.parametrize("lat", [False, True], ids=["base", "nerfw"])
@pytest.mark.parametrize("R,N", fr.B_SHAPES)
def test_single_product_render_is_its_own_arithmetic(R, N, lat, barf):
    """The same inputs (`sharp` weights) through nfl_render_kernel<1, 1, 10, 0>.  Two float64 references on the float64
    encoding of the exact points (forward_ref.x1_forward), both with the folded layers as read back from the field:
      x1_64   the kernel's arithmetic restated: every layer b + half(W) half(x) accumulated in float64, activations fp32
              between layers;
      truth   the same network on unrounded operands.
    Rule, per head column of field_raw over the live samples: the kernel is nearer to its own arithmetic than that arithmetic
    is to the truth, rms(kernel - x1_64) <= rms(x1_64 - truth).  The bar is the reference gap; nothing measured on the kernel
    sets it.  The kernel differs from x1_64 by its fp32 accumulation, its fp32 encoding and head activations, and by the
    fp16 roundings these move across a boundary; a lost bias, k-step or a stale piece reads far above 1
    (tests/test_forward_refs_cpu.py: torch's fp32 matmul in the accumulator's place reads 0.04 .. 0.45, a lost bias 1.2 .. 1e5).
    Checked before the pass is launched: in every column rms(x1_64 - truth) >= 8 * 2^-24 * max|truth|.
    The composited outputs of the pass equal forward_ref.composite_ref of its own field_raw within that function's bounds.
    Guards intact, no NaN left.

    Measured on the MI355X, the worst of the eight cases per column (printed per case): rgb 0.111 0.177 0.135, sigma 0.351,
    rgb_t 0.329 0.274 0.149, sigma_t 0.211, beta 0.331 -- the stand-in's figures; the regime is `sharp`, no column came near
    the floor.  Composites, error / bound: weights 0.16, opacity 7.4e-4, depth 1.0e-3, rgb 3.9e-4, rgb_static 5.4e-4,
    rgb_transient 1.2e-3, beta 1.2e-3."""
    widths, spec, inp, model = real_fields(R, N, lat)
    from nerf_fl_amd import rendering as rnd
    assert kernel_name(widths, "f16") == "nfl_render_kernel<1, 1, 10, 0>"
    f = field_of(model, widths, "f16")
    rnd._pack_streams([f])
    F = {k: v.detach().float().cpu() for k, v in model.named_parameters()}
    for name, (w, b) in f.fold.items():
        F[name + ".weight"], F[name + ".bias"] = w.cpu(), b.cpu()
    pe_w = fr.BARF if barf else None
    val = fr.encoded_inputs(inp, widths, lat, lat, N, pe_w)
    x1 = fr.x1_forward(F, val, widths, lat, lat)
    truth = fr.x1_forward(F, val, widths, lat, lat, rounded=False)
    conditions = fr.x1_conditions(x1, truth, lat)
    assert not conditions, conditions

    rays, z, kw = real_kw(inp, barf)
    out = fr.run_render(f, rays, z, N, **kw)
    bad = clean(out, "RENDER f16")
    raw = out["field_raw"].cpu()
    more, report = fr.x1_rule(raw, x1, truth, lat)
    bad += more
    ref = fr.composite_ref(raw, inp["z"], noise=None, noise_std=0.0, use_t=lat, white_back=True, beta_min=spec.beta_min)
    more, comp = fr.composite_violations(out, ref)
    bad += more
    if lat and not torch.equal(out["transient_sigmas"].cpu().view(torch.int32).flatten(), raw[:, 7].contiguous().view(torch.int32)):
        bad.append("transient_sigmas is not field_raw[:, 7]")
    print(f"single-product render R={R} N={N} {'nerfw' if lat else 'base'} {'barf' if barf else 'plain'}: "
          f"rms(kernel - x1_64) / rms(x1_64 - truth) " + ", ".join(f"{k} {v:.3f}" for k, v in report.items())
          + "; composites, error / bound " + ", ".join(f"{k} {v:.2e}" for k, v in comp.items()))
    assert not bad, "\n".join(bad)
