"""The weight packer on its own: nfl_pack_kernel (csrc/nfl_pack.hip) through nfl_pack_field / nfl_pack_fields, with the test's
own tensors as parameters, against tests/pack_codec.py (the format written down from csrc/nfl_plan.h; test_pack_codec_cpu.py
holds its tile order to the built plans).

(a) every round-to-nearest stream EQUAL to the codec, byte for byte: hi, lo, bias table, padding (+0) and both guards;
(b) the drawn stream (dgrad NFL_PREC_F16), exact parts: every weight that is an fp16 value comes out itself, every other as one of
    its two fp16 neighbours, subnormal range included; two packs are identical; the forward stream is not drawn;
(c) the draws' statistics: zero mean (overall and per sign, layer, j, lane, normal / subnormal range), the rate at constant
    weights, and the redraw when a weight moves by one fp32 ulp.  Every bound is 6 sqrt(sum f_i (1 - f_i)), f_i the discarded
    fraction of weight i, known exactly from its bits; about 100 assertions, false-alarm probability below 1e-6.  The draws are a
    deterministic hash: a result is reproducible, and nothing here is re-seeded to pass;
(d) a batch of four (two) jobs writes what four single-job calls write, in either order;
(e) the status word of the job whose field holds a weight beyond fp16, and of no other;
(f) the Python layer re-packs exactly when (data_ptr, _version) of a parameter moves.

Every destination lies between two GUARD-byte guards and is pre-filled with 0xA5 like them."""
import ctypes as C
import functools
import math
import types

import pytest
import torch

import pack_codec as pc
from pack_codec import F16, F16W, F16X3, WIDTHS

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KINDS = list(pc.KINDS)                  # the layouts are pack_codec's: the ones test_pack_codec_cpu.py holds to the built plans
STATUS_RANGE = 2                        # NFL_STATUS_RANGE
GUARD = 4096
Z = 6.0


# ---- the test's own parameters ------------------------------------------------------------------------------------------
def hard_values(k, g):
    """k values of each class a conversion can get wrong (listed in make_params), signs at random."""
    sign = lambda n: torch.randint(0, 2, (n,), generator=g).float() * 2 - 1
    half = lambda bits: bits.to(torch.int16).view(torch.float16).float()
    b = torch.randint(0, 0x7BFF, (k,), generator=g)
    sub = 2.0 ** -24 + torch.rand(k, generator=g) * (2.0 ** -14 - 2.0 ** -24)
    sub[0::4], sub[1::4], sub[2::4] = 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -25
    return torch.cat([
        sign(k) * half(torch.randint(0, 0x7C00, (k,), generator=g)),                         # fp16 values, subnormal ones too
        sign(k) * (half(b) + half(b + 1)) / 2,                                               # ties, b even or odd
        sign(k) * 0.0,                                                                       # +0 and -0
        sign(k) * sub,                                                                       # below 2^-14
        sign(k) * torch.randint(1, 1 << 23, (k,), generator=g).to(torch.int32).view(torch.float32),      # fp32 denormals
        sign(k) * 65504.0])


@functools.lru_cache(maxsize=None)
def make_params(widths, kind, seed=0):
    """{NFL_P_* index: (weight, bias)}: weights randn x 10^U{-6..1} (a quarter of them below 2^-14, where fp16 is subnormal),
    with fp16 values, ties between fp16 neighbours (even and odd side), +-0, 2^-24, 2^-25, 3 2^-25 and other magnitudes in
    (2^-24, 2^-14), fp32 denormals and +-65504 scattered over every layer; biases random and all distinct."""
    g = torch.Generator().manual_seed(1000 * seed + 17)
    out = {}
    for l, (o, i) in pc.layer_shapes(widths, *pc.KINDS[kind]).items():
        w = torch.randn(o * i, generator=g) * 10.0 ** torch.randint(-6, 2, (o * i,), generator=g).float()
        hard = hard_values(max(4, o * i // 100), g)
        w[torch.randperm(o * i, generator=g)[:hard.numel()]] = hard
        assert float(w.abs().max()) <= 65504.0
        out[l] = (w.view(o, i).contiguous(), torch.randn(o, generator=g))
    biases = torch.cat([b for _, b in out.values()])
    assert biases.unique().numel() == biases.numel()
    return out


def const_params(widths, kind, c):
    return {l: (torch.full(s, c), torch.zeros(s[0])) for l, s in pc.layer_shapes(widths, *pc.KINDS[kind]).items()}


def upload(params):
    """(nfl_field_params, tensors to keep alive): INTEGRATION.md, section 2."""
    from nerf_fl_amd import _lib
    fp, keep = _lib.FieldParams(), []
    for l, (w, b) in params.items():
        keep += [w.to(DEV).contiguous(), b.to(DEV).contiguous()]
        fp.weight[l], fp.bias[l] = keep[-2].data_ptr(), keep[-1].data_ptr()
    return fp, keep


# ---- streams, arenas and launches -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stream(widths, kind, prec, rays_grad=None):
    """A built plan (host blob + device copy), its size and the codec's tiles.  rays_grad None: the forward stream."""
    h, plan = pc.build_plan(widths, kind, prec, rays_grad)
    has_a, has_t = pc.KINDS[kind]
    tiles = pc.forward_tiles(widths, has_a, has_t) if rays_grad is None else pc.dgrad_tiles(widths, has_a, has_t, bool(rays_grad))
    name = f"{kind} {widths} " + ("forward" if rays_grad is None else f"dgrad rays_grad={rays_grad}") + f" prec={prec}"
    return types.SimpleNamespace(h=h, d=torch.frombuffer(bytearray(h.raw), dtype=torch.uint8).to(DEV), nbytes=int(plan["packed_bytes"]),
                                 total_ks=int(plan["total_ks"]), tiles=tiles, split=int(plan["ks_bytes"]) == 2048, name=name)


def arena(s):
    return torch.full((GUARD + s.nbytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)


def job(s, fp, buf, status=None):
    from nerf_fl_amd import _lib
    return _lib.PackJob(C.cast(s.h, C.c_void_p), s.d.data_ptr(), C.pointer(fp), buf.data_ptr() + GUARD, s.nbytes, status)


def launch(jobs):
    from nerf_fl_amd import _lib
    rc = _lib.lib().nfl_pack_fields(len(jobs), (_lib.PackJob * len(jobs))(*jobs), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return rc


def pack_one(s, fp, status=None):
    """One nfl_pack_field call into a fresh arena; returns the arena on the host."""
    from nerf_fl_amd import _lib
    buf = arena(s)
    rc = _lib.lib().nfl_pack_field(s.h, s.d.data_ptr(), C.byref(fp), buf.data_ptr() + GUARD, s.nbytes, status,
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0, (s.name, rc)
    return buf.cpu()


def kept(s, host):
    """The packed bytes of an arena, after checking its guards."""
    assert bool((host[:GUARD] == 0xA5).all()), f"{s.name}: the guard in front of the destination was written"
    assert bool((host[GUARD + s.nbytes:] == 0xA5).all()), f"{s.name}: the guard behind the destination was written"
    return host[GUARD:GUARD + s.nbytes]


def images(s, packed):
    """(hi, lo or None, bias): int16 (total_ks, 64, 8) images and the fp32 (n_rt, 32) table of a packed buffer."""
    n = 2 if s.split else 1
    img = packed[:s.total_ks * n * 1024].view(torch.int16).view(s.total_ks, n, 64, 8)
    bias = packed[s.total_ks * n * 1024:].view(torch.float32).view(len(s.tiles), 32)
    return img[:, 0], (img[:, 1] if s.split else None), bias


def first_mismatch(s, name, got, exp):
    bad = (got != exp).flatten().nonzero().flatten()
    at = int(bad[0])
    ks, lane, j = at // 512, (at // 8) % 64, at % 8
    return (f"{s.name}: {bad.numel()} {name} positions differ, the first at {pc.locate(s.tiles, ks, lane, j)}: "
            f"got 0x{int(got.flatten()[at]) & 0xFFFF:04x}, expected 0x{int(exp.flatten()[at]) & 0xFFFF:04x}")


def assert_bias(s, bias, exp):
    if not torch.equal(bias.view(torch.int32), exp.view(torch.int32)):
        t, r = (bias.view(torch.int32) != exp.view(torch.int32)).nonzero()[0].tolist()
        pytest.fail(f"{s.name}: bias table row {r} of tile {t} (layer, row) = {tuple(pc.index(s.tiles)[1][t, r].tolist())}: "
                    f"got {float(bias[t, r])!r}, expected {float(exp[t, r])!r}")


def assert_equals_codec(s, host, params):
    """The kept bytes of an arena == pc.encode, as int32 bits; the first difference named by place."""
    packed = kept(s, host)
    e_hi, e_lo, e_bias, idx = pc.encode(s.tiles, params, s.split)
    hi, lo, bias = images(s, packed)
    pad = idx[..., 0] == pc.PAD
    for name, img in (("hi", hi), ("lo", lo)):
        if img is not None and bool((img[pad] != 0).any()):
            pytest.fail(first_mismatch(s, name + " padding", torch.where(pad, img, torch.zeros_like(img)), torch.zeros_like(img)))
    if torch.equal(packed.view(torch.int32), pc.assemble(e_hi, e_lo, e_bias).view(torch.int32)):
        return
    e_hi = e_hi.view(torch.int16).view(-1, 64, 8)
    if not torch.equal(hi, e_hi):
        pytest.fail(first_mismatch(s, "hi", hi, e_hi))
    if s.split and not torch.equal(lo, e_lo.view(torch.int16).view(-1, 64, 8)):
        pytest.fail(first_mismatch(s, "lo", lo, e_lo.view(torch.int16).view(-1, 64, 8)))
    assert_bias(s, bias, e_bias)
    pytest.fail(f"{s.name}: the buffers differ, the images and the table do not")


# ---- (a) round-to-nearest streams ----------------------------------------------------------------------------------------
RN_STREAMS = [(F16, None), (F16X3, None), (F16W, 0), (F16W, 1), (F16X3, 0), (F16X3, 1)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("widths", WIDTHS)
def test_round_to_nearest_streams_equal_the_codec(widths, kind):
    params = make_params(widths, kind)
    fp, keep = upload(params)
    for prec, rays_grad in RN_STREAMS:
        s = stream(widths, kind, prec, rays_grad)
        assert_equals_codec(s, pack_one(s, fp), params)


# ---- (b) the drawn stream, exact parts -----------------------------------------------------------------------------------
def drawn(s, host, params):
    """(got, toward, f, ulp, w, named) of a drawn stream after the checks that hold for every draw: guards, +0 padding, a zero
    bias table, fp16 values kept, every other weight on one of its two fp16 neighbours."""
    hi, _, bias = images(s, kept(s, host))
    idx = pc.index(s.tiles)[0]
    w = pc.gather_weights(s.tiles, params)
    toward, f, ulp = pc.fp16_neighbours(w)
    named = idx[..., 0] != pc.PAD
    assert not bool((hi[~named] != 0).any()), f"{s.name}: padding is not +0"
    assert_bias(s, bias, torch.zeros_like(bias))
    exact = named & (f == 0)
    if bool((hi[exact] != toward[exact]).any()):
        pytest.fail(first_mismatch(s, "fp16-valued", torch.where(exact, hi, toward), toward))
    up = hi == toward + 1
    if not bool(((hi == toward) | up)[named].all()):
        pytest.fail(first_mismatch(s, "drawn (neither neighbour; expected = the one toward zero)", torch.where(named & ~up, hi, toward), toward))
    return hi, toward, f, ulp, w, named


@pytest.mark.parametrize("rays_grad", [0, 1])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("widths", WIDTHS)
def test_drawn_stream_exact_parts(widths, kind, rays_grad):
    params = make_params(widths, kind)
    fp, keep = upload(params)
    s = stream(widths, kind, F16, rays_grad)
    host = pack_one(s, fp)
    hi, toward, f, _, _, named = drawn(s, host, params)
    moved = named & (f != 0)
    # it is drawn at all: the discarded fractions of these weights are spread evenly over (0, 1), so half of them move away from
    # zero; rounding toward zero gives 0, away from it 1 (the statistics proper are (c)'s)
    assert 0.2 < float((hi == toward + 1)[moved].float().mean()) < 0.8
    assert torch.equal(pack_one(s, fp), host), f"{s.name}: two packs of the same weights differ"
    sf = stream(widths, kind, F16, None)                                        # the draw touches transposed tiles only
    assert_equals_codec(sf, pack_one(sf, fp), params)


# ---- (c) the drawn stream, statistics -------------------------------------------------------------------------------------
def test_draws_have_zero_mean():
    """sum (hi_i - w_i) / ulp_i over a group of weights against 6 sqrt(sum f_i (1 - f_i)); the coarse stream with the ray
    gradient's tiles, so every weight takes part.

    Measured on the MI355X (sum in ulp / bound, weights):
      all -110.3 / 1748.4 (527872);  w > 0 +68.1 / 1237.2 (264099);  w < 0 -178.4 / 1235.5 (263773);
      normal range +143.9 / 1445.0 (355935);  subnormal range -254.2 / 984.4 (171937; mean -0.0015 ulp, bound 0.0057);
      layers 0..7: +88.2 / 305.3, +60.5 / 616.1, -127.0 / 616.3, -13.4 / 616.1, -207.7 / 687.5, -31.7 / 616.6, +33.2 / 615.9,
      +19.2 / 615.3;  layer 9 +41.5 / 458.7;  layer 10 +16.4 / 37.6 (256);  layer 11 +10.5 / 46.4 (384);
      j 0..7: -38.2, +66.3, -104.4, -37.6, -44.5, +82.9, -31.5, -3.4, each / 617 to 620 (about 66000 each);
      lanes 0..63: |sum| <= 78.4 (lane 45) / 214 to 220 (about 8250 each), the worst ratio 0.36.
    The instruction therefore draws over the bits an fp16 SUBNORMAL discards too (see also the 2^-16 rows of the rate test)."""
    widths, kind = WIDTHS[0], "coarse"
    params = make_params(widths, kind)
    fp, keep = upload(params)
    s = stream(widths, kind, F16, 1)
    hi, toward, f, ulp, w, named = drawn(s, pack_one(s, fp), params)
    idx = pc.index(s.tiles)[0]
    err = (hi.view(torch.float16).double() - w.double()) / ulp
    var = f * (1 - f)
    lane = torch.arange(64).view(1, 64, 1).expand_as(named)
    j = torch.arange(8).view(1, 1, 8).expand_as(named)
    sub = w.abs() < 2.0 ** -14
    groups = [("all", named), ("w > 0", named & ~torch.signbit(w)), ("w < 0", named & torch.signbit(w)),
              ("normal range", named & ~sub), ("subnormal range", named & sub)]
    groups += [(f"layer {l}", idx[..., 0] == l) for l in sorted(set(idx[..., 0].unique().tolist()) - {pc.PAD})]
    groups += [(f"j {k}", named & (j == k)) for k in range(8)] + [(f"lane {k}", named & (lane == k)) for k in range(64)]
    n_sub = int((named & sub & (f != 0)).sum())
    assert int(named.sum()) > 5e5 and n_sub >= 2e4 and len(groups) < 120
    failed = []
    for name, m in groups:
        total, bound, n = float(err[m].sum()), Z * math.sqrt(float(var[m].sum())), int(m.sum())
        print(f"zero mean, {name}: sum {total:+.1f} ulp over {n} weights, bound {bound:.1f} (mean {total / n:+.5f}, bound {bound / n:.5f})")
        if name == "subnormal range":
            assert bound / n < 0.05
        if not abs(total) <= bound:
            failed.append(name)
    assert not failed, failed


def one_constant(h, f):
    ulp = float(pc.fp16_neighbours(torch.tensor([h]))[2])
    return math.copysign(abs(h) + f * ulp, h)


@pytest.mark.parametrize("f", [1 / 8, 1 / 2, 7 / 8])
@pytest.mark.parametrize("h", [1.0, -0.37109375, 2.0 ** -16])
def test_draw_rate_at_a_constant(h, f):
    """Every weight of every layer = h + f ulp(h) (away from zero): the share of positions that moved away from zero is f within
    6 sqrt(f (1 - f) / N).  A draw that ignored the position would give 0 or 1.

    Measured on the MI355X, N = 527872 (bounds: f +- 0.00273 at 1/8 and 7/8, +- 0.00413 at 1/2):
      h = 1.0          0.12493  0.50150  0.87502
      h = -0.37109375  0.12520  0.50066  0.87470
      h = 2^-16        0.12468  0.50025  0.87537"""
    widths, kind = WIDTHS[0], "coarse"
    c = one_constant(h, f)
    params = const_params(widths, kind, c)
    fp, keep = upload(params)
    s = stream(widths, kind, F16, 1)
    hi, toward, fr, _, w, named = drawn(s, pack_one(s, fp), params)
    assert float(w[named].min()) == float(w[named].max()) == c and float(fr[named].min()) == float(fr[named].max()) == f
    assert float(toward[named].view(torch.float16)[0]) == h
    n = int(named.sum())
    share, bound = float((hi == toward + 1)[named].double().mean()), Z * math.sqrt(f * (1 - f) / n)
    print(f"rate at h = {h!r}, f = {f}: {share:.5f} of {n} positions moved away from zero, bound {f} +- {bound:.5f}")
    assert abs(share - f) <= bound


@pytest.mark.parametrize("direction", [math.inf, -math.inf])
@pytest.mark.parametrize("h", [1.0, -0.37109375, 2.0 ** -16])
def test_draw_is_redrawn_when_the_weight_moves(h, direction):
    """w = h + ulp / 2 everywhere, then w' = nextafter(w, +-inf), one fp32 ulp: f moves by 2^-13 or less, and the decisions of the
    two packs differ at 1/2 of the positions within 6 sqrt(1 / (4 N)).  A draw that ignored the weight's bits: about 0.

    Measured on the MI355X, N = 527872, bound 0.5 +- 0.00413 (toward +inf, toward -inf):
      h = 1.0  0.49998, 0.50110;  h = -0.37109375  0.50004, 0.49956;  h = 2^-16  0.50059, 0.49926"""
    widths, kind = WIDTHS[0], "coarse"
    s = stream(widths, kind, F16, 1)
    c = one_constant(h, 0.5)
    c2 = float(torch.nextafter(torch.tensor(c), torch.tensor(direction)))
    assert c2 != c
    ups = []
    for v in (c, c2):
        params = const_params(widths, kind, v)
        fp, keep = upload(params)
        hi, toward, fr, _, _, named = drawn(s, pack_one(s, fp), params)
        assert abs(float(fr[named][0]) - 0.5) <= 2.0 ** -13 and float(toward[named].view(torch.float16)[0]) == h
        ups.append((hi == toward + 1)[named])
    n = ups[0].numel()
    share, bound = float((ups[0] != ups[1]).double().mean()), Z * math.sqrt(1 / (4 * n))
    print(f"redraw at h = {h!r}, nextafter toward {direction}: {share:.5f} of {n} decisions differ, bound 0.5 +- {bound:.5f}")
    assert abs(share - 0.5) <= bound


# ---- (d) batching ----------------------------------------------------------------------------------------------------------
def batch_jobs(widths):
    """The four streams of a training step, all of different block counts: (stream, which field's parameters)."""
    return [(stream(widths, "coarse", F16X3, None), "coarse"), (stream(widths, "coarse", F16, 0), "coarse"),
            (stream(widths, "nerfw", F16X3, None), "nerfw"), (stream(widths, "nerfw", F16X3, 1), "nerfw")]


@pytest.mark.parametrize("widths", WIDTHS[:2])
def test_batches_equal_single_jobs(widths):
    jobs = batch_jobs(widths)
    assert len({s.total_ks + len(s.tiles) for s, _ in jobs}) == 4
    fps = {k: upload(make_params(widths, k)) for k in KINDS}
    single = [pack_one(s, fps[k][0]) for s, k in jobs]
    for s, host in zip((s for s, _ in jobs), single):
        kept(s, host)
    for order in ([0, 1, 2, 3], [3, 2, 1, 0], [1, 2], [2, 0]):
        bufs = {i: arena(jobs[i][0]) for i in order}
        assert launch([job(jobs[i][0], fps[jobs[i][1]][0], bufs[i]) for i in order]) == 0
        for i in order:
            host = bufs[i].cpu()
            kept(jobs[i][0], host)
            assert torch.equal(host, single[i]), f"batch {order}: job {order.index(i)} ({jobs[i][0].name}) differs from its single-job call"


# ---- (e) the status bit ----------------------------------------------------------------------------------------------------
BEYOND = [(1.0e5, pc.P_XYZ1, 0, 0), (math.inf, pc.P_T0 + 2, 5, 7), (math.nan, pc.P_TBETA, 0, 127), (65519.0, pc.P_DIR, 127, -1),
          (-1.0e5, pc.P_XYZ1 + 4, 255, 62)]


def test_status_word_of_the_job_with_a_weight_beyond_fp16():
    widths = WIDTHS[0]
    jobs = batch_jobs(widths)
    fps = {k: upload(make_params(widths, k)) for k in KINDS}

    def run(fp2, with_status=True):
        status = torch.zeros(4, dtype=torch.int32, device=DEV)
        bufs = [arena(s) for s, _ in jobs]
        rc = launch([job(s, fp2 if i == 2 else fps[k][0], bufs[i], status.data_ptr() + 4 * i if with_status else None)
                     for i, (s, k) in enumerate(jobs)])
        for (s, _), b in zip(jobs, bufs):
            kept(s, b.cpu())
        return rc, status.cpu().tolist()

    assert run(fps["nerfw"][0]) == (0, [0, 0, 0, 0])                # +-65504 is in every layer of make_params: inside the range
    for value, layer, r, c in BEYOND:
        p = dict(make_params(widths, "nerfw"))
        w = p[layer][0].clone()
        w[r, c] = value
        p[layer] = (w, p[layer][1])
        fp2, keep2 = upload(p)
        assert run(fp2) == (0, [0, 0, STATUS_RANGE, 0]), value
        assert run(fp2, with_status=False)[0] == 0, value             # no status word: NFL_OK, nothing to write to


# ---- (f) the Python layer's re-pack trigger --------------------------------------------------------------------------------
def test_python_layer_repacks_when_a_parameter_changes():
    from nerf_fl_amd import NeRF, _lib, train
    from nerf_fl_amd import rendering as rnd
    widths = WIDTHS[0]
    torch.manual_seed(3)
    model = NeRF("fine", in_channels_xyz=63, in_channels_dir=27, encode_appearance=True, in_channels_a=48, encode_transient=True,
                 in_channels_t=16).to(DEV)
    f = rnd._field(model, widths[0], widths[1], torch.device(DEV), pack=False, prec=F16X3)
    fwd, bwd = stream(widths, "nerfw", F16X3, None), stream(widths, "nerfw", F16X3, 0)
    pack = lambda: f.ensure_bwd_packed(False, F16X3)
    bp = pack()
    assert f.packed.numel() == fwd.nbytes and bp["packed"].numel() == bwd.nbytes
    pad = torch.full((GUARD,), 0xA5, dtype=torch.uint8)
    seen = []

    def check(what, changes=(True, True)):
        """Both streams == encode of the parameters as they are now (the two folded layers: the tensors the packer read), and
        the (forward, dgrad) bytes differ from the previous check's where `changes` says the step changes them."""
        torch.cuda.synchronize()
        named = dict(model.named_parameters())
        p = {l: (named[n + ".weight"].detach().cpu(), named[n + ".bias"].detach().cpu()) for l, n in enumerate(_lib.LAYER_NAMES)}
        for n in ("dir_encoding.0", "transient_encoding.0"):
            p[_lib.LAYER_NAMES.index(n)] = tuple(t.cpu() for t in f.fold[n])
        got = (f.packed.cpu(), bp["packed"].cpu())
        for s, g in zip((fwd, bwd), got):
            s = types.SimpleNamespace(**{**vars(s), "name": f"{s.name} after {what}"})
            assert_equals_codec(s, torch.cat([pad, g, pad]), p)
        for s, old, new, changed in zip((fwd, bwd), seen[-1] if seen else (), got, changes):
            assert torch.equal(old, new) != changed, f"{what}: {s.name} " + ("did not change" if changed else "changed")
        seen.append(got)

    check("the first pack")
    # nothing changed: nothing is launched
    f.packed.fill_(0xA5), bp["packed"].fill_(0xA5)
    pack()
    torch.cuda.synchronize()
    assert bool((f.packed == 0xA5).all()) and bool((bp["packed"] == 0xA5).all())
    f.key = bp["key"] = None
    pack()
    seen.clear()
    check("forgetting the keys")
    # an optimiser step of the package's own Adam (one launch that writes the parameters and bumps their versions)
    opt = train.Adam(model.parameters(), lr=1e-2)
    for q in model.parameters():
        q.grad = torch.randn_like(q)
    opt.step()
    pack()
    check("an Adam step")
    # one bias alone: its version is the only thing that moves, and only the forward stream's bias table shows it (a bias has no
    # place in the dgrad stream, which is packed again to the same bytes)
    with torch.no_grad():
        dict(model.named_parameters())["static_rgb.0.bias"].add_(0.25)
    pack()
    check("an in-place add_ on one bias", changes=(True, False))
    with torch.no_grad():
        dict(model.named_parameters())["xyz_encoding_3.0.weight"].add_(0.125)
    pack()
    check("an in-place add_ on one weight")
    model.load_state_dict({k: v + 0.01 * torch.randn_like(v) for k, v in model.state_dict().items()})
    pack()
    check("load_state_dict")
    model.static_sigma[0].weight = torch.nn.Parameter(0.1 * torch.randn(1, 256, device=DEV))
    model.transient_encoding[2].weight = torch.nn.Parameter(0.1 * torch.randn(128, 128, device=DEV))
    pack()
    check("re-assigning a Parameter")
